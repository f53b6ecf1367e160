"""Pin the CPU restatement of the Fused-MBConv block (tests/_fused.FusedRef) -- what tests/test_gpu_fused*.py compare the HIP
path with.

The reference has no fused block, so the pin is a composition of the reference's own classes: ConvLayer(in, mid, 3, stride), the
squeeze-excite arithmetic of MBInvertedResBlock.forward, ConvLayer(mid, out, 1, 1, act_func=None), the residual with the
reference's drop-connect.  tests/golden/make_golden_fused.py ran that composition in float64 on stride {1, 2} x {relu, swish,
relu6, h-swish} x SE {0, 8} x {search, derived} at 2 x 16 x 9 x 13, mid 40, out 16, and recorded outputs and gradients
(tests/golden/oracle_fused_pin.npz: _golden.probe of every tensor, corner and centre taps of the dense weight gradient whole).  The
restatement must reproduce them to 1e-12 relative.  Also asserted here, on the CPU: every seed the GPU tests use keeps every
float64 pre-activation at least KINK_TAU from a kink of the activation."""
import os

import numpy as np
import pytest
import torch

import _fused
import _golden

RTOL = 1e-12


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('oracle_fused_pin.npz')


@pytest.mark.parametrize('case', _fused.PIN_CASES, ids=lambda c: 's%d_%s_se%d' % c)
@pytest.mark.parametrize('form', _fused.PIN_FORMS)
def test_restatement_reproduces_the_composition_of_reference_classes(recorded, form, case):
    blk, x, r, seed = _fused.pin_block(form, case)
    s = case[0]
    res = _fused.pin_run(blk, x, r, seed)
    assert res['out'].shape == (2, 16, (9 - 1) // s + 1, (13 - 1) // s + 1)
    assert res['g.fused_conv.conv.weight'].shape == (40, 16, 3, 3)
    tag = _fused.pin_tag(form, case)
    rec = _fused.pin_record(res)
    assert sorted(rec) == sorted(n[len(tag) + 1:] for n in recorded.files if n.startswith(tag + '/'))
    assert ('b.fused_conv.bn.running_var' in rec) == (form == 'derived')
    for n, v in rec.items():
        want = recorded[tag + '/' + n]
        assert v.shape == want.shape
        if n.endswith('.taps'):
            scale = float(np.abs(want).max())
            assert float(np.abs(v - want).max()) <= RTOL * scale, (tag, n)
        else:           # (sum, sum of magnitudes, 24 sampled elements)
            assert abs(v[0] - want[0]) <= RTOL * want[1] and abs(v[1] - want[1]) <= RTOL * want[1], (tag, n)
            scale = max(float(np.abs(want[2:]).max()), 1e-300)
            assert float(np.abs(v[2:] - want[2:]).max()) <= RTOL * scale, (tag, n)


def test_derived_pin_exercises_drop_connect_and_running_statistics():
    moved, kept = 0, set()
    for case in _fused.PIN_CASES:
        blk, x, r, seed = _fused.pin_block('derived', case)
        before = blk.fused_conv.bn.running_mean.clone()
        _fused.pin_run(blk, x, r, seed)
        moved += int(not torch.equal(before, blk.fused_conv.bn.running_mean))
        if case[0] == 1:
            kept.update(bool(v) for v in torch.floor(1.0 - _fused.PIN_DROP + blk.drop_u))
    assert moved == len(_fused.PIN_CASES) and kept == {True, False}


def test_fixture_holds_data_only_and_is_small():
    path = os.path.join(_golden.GOLDEN, 'oracle_fused_pin.npz')
    fx = np.load(path, allow_pickle=False)
    assert os.path.getsize(path) <= 300 * 1024
    for n in fx.files:
        assert fx[n].dtype == np.float64, (n, fx[n].dtype)
    assert len({n.split('/')[0] for n in fx.files}) == len(_fused.PIN_FORMS) * len(_fused.PIN_CASES)


@pytest.mark.parametrize('geom', _fused.GEOMS, ids=_fused.geom_id)
def test_seeds_of_the_gpu_tests_stay_clear_of_the_kinks_search_form(geom):
    o, x, r, seed = _fused.case_data(*geom)
    assert _fused.kink_distance(o, x) >= _fused.KINK_TAU
    if o.act_func != 'swish':
        assert _fused.kink_distance(o, x) < float('inf')


@pytest.mark.parametrize('mode', ['train', 'train_drop', 'eval'])
@pytest.mark.parametrize('geom', _fused.DERIVED_GEOMS, ids=_fused.geom_id)
def test_seeds_of_the_gpu_tests_stay_clear_of_the_kinks_derived_form(geom, mode):
    o, x, r, seed = _fused.derived_case(geom, mode)
    assert _fused.kink_distance(o, x) >= _fused.KINK_TAU


def test_raw_abi_case_stays_clear_of_the_kinks():
    o, x, r, seed = _fused.case_data(*_fused.RAW_GEOM, base=300)
    assert _fused.kink_distance(o, x) >= _fused.KINK_TAU
