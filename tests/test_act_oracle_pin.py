"""Pin the CPU oracle at the activations 'relu6' and 'h-swish' -- what tests/test_gpu_acts.py and test_gpu_acts_derived.py then rely
on it for.

The oracle's ``_act`` knows 'relu' and 'swish' only; tests/_acts.wrapped_oracle() puts the other two over it for the duration of a
test.  oracle.MBConv (batch-statistic form) and oracle.DerivedBlock (affine BatchNorm, running statistics, drop-connect) under that
wrapper are compared with the reference's MBInvertedResBlock(act_func=...) built with the same weights: output, dx, every
parameter gradient and, for the derived form, the buffers; activation x stride 1 / 2 x SE 0 / 8 x k 3 / 5 at 2 x 16 x 9 x 13
(tests/_k7.PIN_GEOM), both sides in float64, with the comparison and tolerances of tests/test_k7_oracle_pin.py.  The reference's
side was recorded by tests/golden/make_golden_act.py (tests/golden/oracle_act_pin.npz) and is replayed here, so the test runs
anywhere; where a checkout of the reference is at hand (TFNAS_REFERENCE, tests/_refload.py) the reference itself is run as well and
must agree with what was recorded."""
import copy
import os

import numpy as np
import pytest
import torch

import _acts
import _golden
import _k7
import _refload

FWD = dict(atol=1e-5, rtol=1e-5)
GRAD = dict(atol=2e-6, rtol=1e-4)


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('oracle_act_pin.npz')


def _tol(key):
    return FWD if key == 'out' or key.startswith('b.') else GRAD


def _check(res, recorded, tag, k_size):
    want_keys = [k[len(tag) + 1:] for k in recorded.files if k.startswith(tag + '/')]
    assert list(res) == want_keys
    for k, v in res.items():
        want = recorded[tag + '/' + k]
        tol = _tol(k)
        if k == 'g.depth_conv.conv.weight':
            assert v.shape == want.shape == (_acts.PIN_GEOM['mc'], 1, k_size, k_size)
            assert np.allclose(v, want, **tol), (tag, k, float(abs(v - want).max()))
        else:
            t = torch.from_numpy(np.asarray(v))
            assert _golden.probe_close(_golden.probe(t), want, t.numel(), tol['atol'], tol['rtol']), (tag, k)


@pytest.mark.parametrize('case', _acts.PIN_CASES, ids=lambda c: '%s_s%d_se%d_k%d' % c)
@pytest.mark.parametrize('form', _acts.PIN_FORMS)
def test_wrapped_oracle_block_matches_reference(recorded, form, case):
    act, s, se, k = case
    blk, x, r, seed = _acts.pin_oracle_block(form, case)
    assert blk.act_func == act and blk.kernel_size == k
    state = copy.deepcopy(blk.state_dict())       # (before the step moves the running statistics)
    with _acts.wrapped_oracle():
        res = _k7.pin_run(blk, x, r, seed)
    assert res['out'].shape == (2, 16, (9 - 1) // s + 1, (13 - 1) // s + 1)
    _check(res, recorded, _acts.pin_tag(form, case), k)
    if _refload.available():                      # the reference itself, where it can be imported
        ref = _refload.import_reference()
        q = _acts.PIN_GEOM
        rb = ref.layers.MBInvertedResBlock(q['ic'], q['mc'], se, q['oc'], k, s, affine=(form == 'derived'), act_func=act)
        rb.load_state_dict(state)
        rb.drop_connect_rate = getattr(blk, 'drop_connect_rate', 0.0)
        live = _k7.pin_run(rb.double().train(), x, r, seed)
        _check(live, recorded, _acts.pin_tag(form, case), k)
        for kk in live:
            assert np.allclose(res[kk], live[kk], **_tol(kk)), (form, case, kk)


@pytest.mark.parametrize('act', _acts.NEW_ACTS)
@pytest.mark.parametrize('form', _acts.PIN_FORMS)
def test_pin_inputs_reach_every_branch(form, act):
    """the pinned cases are not ReLU / a linear function in disguise: over the cases of one activation every branch (below,
    between, above the two kinks) holds pre-activations at both sites of the derived form and after BN1 of the search form"""
    z1, z2 = [], []
    for case in _acts.PIN_CASES:
        if case[0] != act:
            continue
        blk, x, r, seed = _acts.pin_oracle_block(form, case)
        with torch.no_grad(), _acts.wrapped_oracle():
            if form == 'search':
                det = {}
                blk(x, det)
                z1.append(det['Eh']); z2.append(det['Dh'])
            else:
                a, b = _acts.derived_preacts(blk, x)
                z1.append(a); z2.append(b)
    assert min(_acts.branch_fractions(torch.cat([z.reshape(-1) for z in z1]), act)) >= 1e-3
    f2 = _acts.branch_fractions(torch.cat([z.reshape(-1) for z in z2]), act)
    assert min(f2 if form == 'derived' or act == 'h-swish' else f2[:2]) >= 1e-3, f2


def test_wrapper_is_removed_and_delegates():
    import tfnas_oracle as orc
    orig = orc._act
    x = torch.linspace(-8, 8, 41, dtype=torch.float64)
    with _acts.wrapped_oracle():
        assert orc._act is not orig
        assert torch.equal(orc._act(x, 'relu'), orig(x, 'relu')) and torch.equal(orc._act(x, 'swish'), orig(x, 'swish'))
        assert torch.equal(orc._act(x, 'relu6'), torch.nn.functional.relu6(x))
        assert torch.allclose(orc._act(x, 'h-swish'), torch.nn.functional.hardswish(x), atol=1e-15)
        with pytest.raises(ValueError):
            orc._act(x, 'gelu')
    assert orc._act is orig
    with pytest.raises(ValueError):
        orc._act(x, 'relu6')


def test_fixture_holds_arrays_only_and_is_small():
    path = os.path.join(_golden.GOLDEN, 'oracle_act_pin.npz')
    fx = np.load(path, allow_pickle=False)
    assert os.path.getsize(path) <= 364324        # the largest fixture committed before it (cell_k7_s1_swish_res.npz)
    assert len({k.split('/')[0] for k in fx.files}) == len(_acts.PIN_FORMS) * len(_acts.PIN_CASES) == 32
    for k in fx.files:
        assert fx[k].dtype.kind == 'f', (k, fx[k].dtype)
