"""CPU checks of the restatement tests/test_gpu_kinds.py compares the mixed-cell launches with (tests/_kinds.py: the weighted sum
of the oracle's MBConv blocks and _fused.FusedRef).  Pinned in float64 against tests/golden/kinds_pin.npz, which
tests/golden/make_golden_kinds.py recorded from the REFERENCE's own MixedOP.forward (soft branch) with its m_ops entries replaced
-- the reference's MBInvertedResBlock for plain and expand-free candidates, _fused.FusedRef for Fused-MBConv ones: probes of out,
dx, d log_alphas and every parameter gradient, one 3-candidate cell per activation x stride and one 8-candidate swish cell.  And:
every kinked case of the GPU suite finds, within 200 tries, a seed whose float64 pre-activations of EVERY candidate stay KINK_TAU
from every kink -- chosen from the restatement alone, so that no element is ever exempted -- and the float32 restatement agrees
with a float64 run of itself far inside the GPU gate at those seeds."""
import copy
import os

import numpy as np
import pytest
import torch

import _golden
import _kinds

RTOL = 1e-11


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('kinds_pin.npz')


@pytest.mark.parametrize('case', _kinds.PIN_CASES, ids=_kinds.pin_tag)
def test_restatement_reproduces_the_reference_mixedop_over_replaced_candidates(recorded, case):
    o, x, r, la, seed = _kinds.pin_case(case)
    res = _kinds.pin_run(o, x, r, la, seed)
    tag = _kinds.pin_tag(case)
    rec = _kinds.pin_record(res)
    assert sorted(rec) == sorted(n[len(tag) + 1:] for n in recorded.files if n.startswith(tag + '/'))
    assert res['dla'].shape == (len(case[0]),) and float(np.abs(res['dla']).max()) > 0
    kinds = {c[0] for c in case[0]}
    assert kinds == {'M', 'N', 'F'}
    assert any(k.endswith('fused_conv.conv.weight') for k in rec) and any(k.endswith('inverted_bottleneck.conv.weight') for k in rec)
    for n, v in rec.items():                     # (sum, sum of magnitudes, 24 sampled elements)
        want = recorded[tag + '/' + n]
        assert v.shape == want.shape
        assert abs(v[0] - want[0]) <= RTOL * want[1] and abs(v[1] - want[1]) <= RTOL * want[1], (tag, n)
        scale = max(float(np.abs(want[2:]).max()), 1e-300)
        assert float(np.abs(v[2:] - want[2:]).max()) <= RTOL * scale, (tag, n)


def test_fixture_holds_data_only_and_is_small():
    path = os.path.join(_golden.GOLDEN, 'kinds_pin.npz')
    fx = np.load(path, allow_pickle=False)
    assert os.path.getsize(path) <= 200 * 1024
    for n in fx.files:
        assert fx[n].dtype == np.float64, (n, fx[n].dtype)
    assert {n.split('/')[0] for n in fx.files} == {_kinds.pin_tag(c) for c in _kinds.PIN_CASES}


@pytest.mark.parametrize('act', _kinds.KINKED_ACTS)
@pytest.mark.parametrize('stride', (1, 2))
def test_kinked_cases_find_a_kink_clear_seed(act, stride):
    N, ic, oc, H, W = _kinds.SMALL_SHAPE
    o, x, r, w, seed = _kinds.case_data(_kinds.THREE, N, ic, oc, H, W, stride, act)          # (AssertionError after 200 tries)
    assert 300 <= seed < 500 and _kinds.kink_distance(o, x) >= _kinds.KINK_TAU
    # the same call gives the same case: the GPU tests and this one see one seed
    assert _kinds.case_data(_kinds.THREE, N, ic, oc, H, W, stride, act)[4] == seed
    # float32 against float64 of the restatement itself: out, dx, d w and every gradient inside 1/10 of the GPU gate
    ref32 = _kinds.ref_run(o, x, r, w)
    o64 = copy.deepcopy(o).double()
    ref64 = _kinds.ref_run(o64, x.double(), r.double(), w.double())
    flat32 = [ref32[0], ref32[1], ref32[2]] + list(ref32[3].values())
    flat64 = [ref64[0], ref64[1], ref64[2]] + list(ref64[3].values())
    for a, b in zip(flat32, flat64):
        assert float((a.double() - b).abs().max()) <= 0.1 * (2e-5 + 1e-4 * float(b.abs().max()))


def test_swish_cases_take_their_base_seed():
    for geom in _kinds.EIGHT_SHAPES:
        assert _kinds.case_data(_kinds.EIGHT, *geom, 'swish')[4] == 300
        assert _kinds.kink_distance(_kinds.make_ref(_kinds.EIGHT, geom[1], geom[2], geom[5], 'swish', 300), torch.zeros(1)) == float('inf')
