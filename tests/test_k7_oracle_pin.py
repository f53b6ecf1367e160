"""Pin the CPU oracle at depthwise kernel size 7 -- the size tests/test_gpu_k7.py then relies on it for.

oracle.MBConv(k=7) (batch-statistic form) and oracle.DerivedBlock(k=7) (affine BatchNorm, running statistics, drop-connect) are
compared with the reference's MBInvertedResBlock(kernel_size=7) built with the same weights: forward and all gradients, stride
1 and 2, ReLU and swish, SE on and off, at 2 x 16 x 9 x 13, both sides in float64 (tests/test_oracle_vs_reference.py: in float32
gradients differ with the host and its thread count).  The reference's side was recorded by tests/golden/make_golden_k7.py
(tests/golden/oracle_k7_pin.npz: the depthwise weight gradient whole, _golden.probe of every other tensor) and is replayed here,
so the test runs anywhere; where a checkout of the reference is at hand (TFNAS_REFERENCE, tests/_refload.py) the reference
itself is run as well and must agree with what was recorded.  Tolerances: those of the existing oracle pins
(test_oracle_vs_reference.py: 1e-5 / 1e-5 forward, 2e-6 / 1e-4 gradients; test_oracle_golden.py for the float32 cell vectors).

The same generator writes tests/golden/cell_k7_s1_swish_res.npz and cell_k7_s2_relu_odd.npz -- mixed cells with candidates of
kernel sizes 3 / 3 / 5 / 5 / 7 / 7 / 3 / 7 run by the reference -- which the oracle replays here and the HIP path replays in
tests/test_gpu_k7.py."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import _golden
import _k7
import _refload

FORMS = ('search', 'derived')
FWD = dict(atol=1e-5, rtol=1e-5)
GRAD = dict(atol=2e-6, rtol=1e-4)


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('oracle_k7_pin.npz')


def _tol(key):
    return FWD if key == 'out' or key.startswith('b.') else GRAD


def _check(res, recorded, tag):
    want_keys = [k[len(tag) + 1:] for k in recorded.files if k.startswith(tag + '/')]
    assert list(res) == want_keys
    for k, v in res.items():
        want = recorded[tag + '/' + k]
        tol = _tol(k)
        if k == 'g.depth_conv.conv.weight':
            assert v.shape == want.shape == (_k7.PIN_GEOM['mc'], 1, 7, 7)
            assert np.allclose(v, want, **tol), (tag, k, float(abs(v - want).max()))
        else:
            t = torch.from_numpy(np.asarray(v))
            assert _golden.probe_close(_golden.probe(t), want, t.numel(), tol['atol'], tol['rtol']), (tag, k)


@pytest.mark.parametrize('case', _k7.PIN_CASES, ids=lambda c: 's%d_%s_se%d' % c)
@pytest.mark.parametrize('form', FORMS)
def test_oracle_block_k7_matches_reference(recorded, form, case):
    blk, x, r, seed = _k7.pin_oracle_block(form, case)
    assert blk.kernel_size == 7 and tuple(blk.depth_conv.conv.padding) == (3, 3)
    state = copy.deepcopy(blk.state_dict())       # (before the step moves the running statistics)
    res = _k7.pin_run(blk, x, r, seed)
    assert res['out'].shape == (2, 16, (9 - 1) // case[0] + 1, (13 - 1) // case[0] + 1)
    _check(res, recorded, _k7.pin_tag(form, case))
    if _refload.available():                      # the reference itself, where it can be imported
        ref = _refload.import_reference()
        q = _k7.PIN_GEOM
        rb = ref.layers.MBInvertedResBlock(q['ic'], q['mc'], case[2], q['oc'], 7, case[0], affine=(form == 'derived'),
                                           act_func=case[1])
        rb.load_state_dict(state)
        rb.drop_connect_rate = getattr(blk, 'drop_connect_rate', 0.0)
        live = _k7.pin_run(rb.double().train(), x, r, seed)
        _check(live, recorded, _k7.pin_tag(form, case))
        for k in live:
            assert np.allclose(res[k], live[k], **_tol(k)), (form, case, k)


def test_derived_pin_exercises_drop_connect_and_running_statistics(recorded):
    """the recorded derived cases are not trivial: running statistics moved, and a residual block's images were both kept and
    dropped across the cases (the drop decides whether dx equals the cotangent on that image)"""
    moved, kept = 0, set()
    for case in _k7.PIN_CASES:
        blk, x, r, seed = _k7.pin_oracle_block('derived', case)
        before = blk.depth_conv.bn.running_mean.clone()
        _k7.pin_run(blk, x, r, seed)
        moved += int(not torch.equal(before, blk.depth_conv.bn.running_mean))
        if case[0] == 1:
            kept.update(bool(v) for v in torch.floor(1.0 - _k7.PIN_DROP + blk.drop_u))
    assert moved == len(_k7.PIN_CASES) and kept == {True, False}


@pytest.mark.parametrize('name', _k7.K7_CELL_NAMES)
def test_fixture_holds_data_only_and_is_small(name):
    path = os.path.join(_golden.GOLDEN, 'cell_%s.npz' % name)
    fx = np.load(path, allow_pickle=False)
    biggest = max(os.path.getsize(os.path.join(_golden.GOLDEN, 'cell_%s.npz' % n)) for n in _golden.CELL_NAMES)
    assert os.path.getsize(path) <= biggest
    for k in fx.files:
        assert fx[k].dtype.kind in 'fi' or (k == 'act' and fx[k].dtype.kind == 'U'), (k, fx[k].dtype)
    assert [int(k) for k in fx['ks']] == list(_k7.SOFT_KS)
    old = _golden.load('cell_%s.npz' % _golden.CELL_NAMES[0])
    layout = lambda names: {re.sub(r'\d+', '#', n) for n in names}      # noqa: E731  (candidate / layer indices aside)
    assert layout(fx.files) - {'ks'} == layout(old.files)


@pytest.mark.parametrize('name', _k7.K7_CELL_NAMES)
def test_oracle_replays_k7_cell_soft_mode(name):
    fx = _golden.load('cell_%s.npz' % name)
    cell = _k7.oracle_cell_from(fx)
    assert [op.kernel_size for op in cell.m_ops] == list(_k7.SOFT_KS)
    x = torch.from_numpy(fx['x']).requires_grad_(True)
    out, lat = cell(x, False, None, exp_noise=torch.from_numpy(fx['e']))
    assert np.allclose(out.detach().numpy(), fx['soft_out'], atol=2e-5, rtol=1e-4)
    assert abs(float(lat.detach()) - float(fx['soft_lat'])) < 1e-6
    ((out * torch.from_numpy(fx['r'])).sum() + 3.0 * lat).backward()
    assert np.allclose(x.grad.numpy(), fx['soft_dx'], atol=2e-5, rtol=1e-3)
    assert np.allclose(cell.log_alphas.grad.numpy(), fx['soft_dalpha'], atol=2e-4, rtol=1e-3)
    for k, p in cell.named_parameters():
        if k != 'log_alphas':
            got, want = _golden.probe(p.grad), fx['softg.' + k]
            assert np.allclose(got, want, atol=1e-4 + 1e-4 * abs(want).max(), rtol=1e-3), k
    assert cell.get_lookup_latency(int(fx['geom'][4])) == [float(v) for v in fx['lats']]


@pytest.mark.parametrize('name', _k7.K7_CELL_NAMES)
@pytest.mark.parametrize('idx', _k7.K7_SAMPLED)
def test_oracle_replays_k7_cell_sampled_candidate(name, idx):
    fx = _golden.load('cell_%s.npz' % name)
    cell = _k7.oracle_cell_from(fx)
    assert cell.m_ops[idx].kernel_size == 7
    x = torch.from_numpy(fx['x']).requires_grad_(True)
    out = cell.m_ops[idx](x)
    assert np.allclose(out.detach().numpy(), fx['samp%d_out' % idx], atol=2e-5, rtol=1e-4)
    (out * torch.from_numpy(fx['r'])).sum().backward()
    assert np.allclose(x.grad.numpy(), fx['samp%d_dx' % idx], atol=2e-5, rtol=1e-3)
    for k, p in cell.m_ops[idx].named_parameters():
        want = fx['samp%d_g.%s' % (idx, k)]
        assert np.allclose(p.grad.numpy(), want, atol=1e-4 + 1e-4 * abs(want).max(), rtol=1e-3), k


def test_macs_and_params_of_k7_blocks():
    """parsing.count_macs_in_M / count_params_in_MB of a config with 7 x 7 blocks against formulas written out by hand
    (_k7.hand_macs_in_M / hand_params_in_MB), and the 7 x 7 blocks' share: 49 / 25 of the depthwise term of the 5 x 5 network."""
    from tfnas_amd import parsing
    cfg = _k7.k7_network_config()
    assert [c['kernel_size'] for st in ('stage3', 'stage5') for c in cfg[st]] == [7, 7, 7, 7]
    for size in (64, 224):
        assert abs(parsing.count_macs_in_M(cfg, size) - _k7.hand_macs_in_M(cfg, size)) < 1e-9
    assert abs(parsing.count_params_in_MB(cfg) - _k7.hand_params_in_MB(cfg)) < 1e-12
    cfg5 = _k7.k7_network_config()
    for st in ('stage3', 'stage5'):
        for c in cfg5[st]:
            c['kernel_size'] = 5
    extra = sum((49 - 25) * c['mid_channels'] for st in ('stage3', 'stage5') for c in cfg[st])
    assert abs((parsing.count_params_in_MB(cfg) - parsing.count_params_in_MB(cfg5)) * 1e6 - extra) < 1e-3
