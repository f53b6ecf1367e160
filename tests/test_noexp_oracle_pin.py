"""Pin the CPU oracle on MBConv blocks WITHOUT an expand convolution -- the blocks tests/test_gpu_noexp*.py then rely on it for.

oracle.MBConv (batch-statistic form) and oracle.DerivedBlock (affine BatchNorm, running statistics, drop-connect) built with
mid_channels 16 and 8 at 16 input channels (both: no inverted_bottleneck, mid normalised to 16) are compared with the reference's
MBInvertedResBlock built with the same arguments and weights: forward and all gradients, stride 1 and 2, ReLU and swish, SE on
and off, at 2 x 16 x 9 x 13, both sides in float64.  The reference's side was recorded by tests/golden/make_golden_noexp.py
(tests/golden/oracle_noexp_pin.npz: the depthwise weight gradient whole, _golden.probe of every other tensor) and is replayed
here, so the test runs anywhere; where a checkout of the reference is at hand (TFNAS_REFERENCE, tests/_refload.py) the reference
itself is run as well and must agree with what was recorded.  Tolerances: those of the existing oracle pins
(test_k7_oracle_pin.py: 1e-5 / 1e-5 forward and buffers, 2e-6 / 1e-4 gradients)."""
import copy
import os

import numpy as np
import pytest
import torch

import _golden
import _noexp
import _refload

FWD = dict(atol=1e-5, rtol=1e-5)
GRAD = dict(atol=2e-6, rtol=1e-4)


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('oracle_noexp_pin.npz')


def _tol(key):
    return FWD if key == 'out' or key.startswith('b.') else GRAD


def _check(res, recorded, tag, k):
    want_keys = [n[len(tag) + 1:] for n in recorded.files if n.startswith(tag + '/')]
    assert list(res) == want_keys
    assert not any('inverted_bottleneck' in n for n in want_keys)
    for n, v in res.items():
        want = recorded[tag + '/' + n]
        tol = _tol(n)
        if n == 'g.depth_conv.conv.weight':
            assert v.shape == want.shape == (_noexp.PIN_GEOM['ic'], 1, k, k)
            assert np.allclose(v, want, **tol), (tag, n, float(abs(v - want).max()))
        else:
            t = torch.from_numpy(np.asarray(v))
            assert _golden.probe_close(_golden.probe(t), want, t.numel(), tol['atol'], tol['rtol']), (tag, n)


@pytest.mark.parametrize('case', _noexp.PIN_CASES, ids=lambda c: 'm%d_s%d_%s_se%d' % c)
@pytest.mark.parametrize('form', _noexp.PIN_FORMS)
def test_oracle_block_without_expand_matches_reference(recorded, form, case):
    blk, x, r, seed = _noexp.pin_oracle_block(form, case)
    assert blk.inverted_bottleneck is None and blk.mid_channels == _noexp.PIN_GEOM['ic']       # mid 8 and 16 normalise to 16
    state = copy.deepcopy(blk.state_dict())       # (before the step moves the running statistics)
    res = _noexp.pin_run(blk, x, r, seed)
    assert res['out'].shape == (2, 16, (9 - 1) // case[1] + 1, (13 - 1) // case[1] + 1)
    _check(res, recorded, _noexp.pin_tag(form, case), _noexp.pin_k(case))
    if _refload.available():                      # the reference itself, where it can be imported
        ref = _refload.import_reference()
        q = _noexp.PIN_GEOM
        rb = ref.layers.MBInvertedResBlock(q['ic'], case[0], case[3], q['oc'], _noexp.pin_k(case), case[1],
                                           affine=(form == 'derived'), act_func=case[2])
        rb.load_state_dict(state)
        rb.drop_connect_rate = getattr(blk, 'drop_connect_rate', 0.0)
        live = _noexp.pin_run(rb.double().train(), x, r, seed)
        _check(live, recorded, _noexp.pin_tag(form, case), _noexp.pin_k(case))
        for n in live:
            assert np.allclose(res[n], live[n], **_tol(n)), (form, case, n)


def test_derived_pin_exercises_drop_connect_and_running_statistics():
    """the recorded derived cases are not trivial: running statistics moved, and a residual block's images were both kept and
    dropped across the cases"""
    moved, kept = 0, set()
    for case in _noexp.PIN_CASES:
        blk, x, r, seed = _noexp.pin_oracle_block('derived', case)
        before = blk.depth_conv.bn.running_mean.clone()
        _noexp.pin_run(blk, x, r, seed)
        moved += int(not torch.equal(before, blk.depth_conv.bn.running_mean))
        if case[1] == 1:
            kept.update(bool(v) for v in torch.floor(1.0 - _noexp.PIN_DROP + blk.drop_u))
    assert moved == len(_noexp.PIN_CASES) and kept == {True, False}


def test_fixture_holds_data_only_and_is_small():
    path = os.path.join(_golden.GOLDEN, 'oracle_noexp_pin.npz')
    fx = np.load(path, allow_pickle=False)
    assert os.path.getsize(path) <= 1 << 19
    for n in fx.files:
        assert fx[n].dtype.kind == 'f', (n, fx[n].dtype)
    assert len({n.split('/')[0] for n in fx.files}) == len(_noexp.PIN_FORMS) * len(_noexp.PIN_CASES)
