"""CPU checks of the restatement the skip-candidate GPU tests compare with (tests/_skip.py: _kinds.MixedRef with an identity module
in the skip slots).  Pinned in float64 against tests/golden/skip_pin.npz, which tests/golden/make_golden_skip.py recorded from the
REFERENCE's own MixedOP.forward (soft branch) with the reference's own IdentityLayer in the skip slots: probes of out, dx,
d log_alphas and every parameter gradient, the expected latency and the looked-up latency row (the identity costs 0), for
[M, N, F, S] under each activation, the 8-candidate swish cell ending in a skip, and [M, S, S] -- all 2 x 8 x 7 x 9, stride 1,
T = 2.5.  And: every kinked case of the GPU suite finds, within 200 tries, a seed whose float64 pre-activations stay KINK_TAU from
every kink, chosen from the restatement alone (a skip has no pre-activation)."""
import os

import numpy as np
import pytest
import torch

import _golden
import _kinds
import _skip

RTOL = 1e-11          # (tests/test_kinds_oracle_pin.py's)


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('skip_pin.npz')


@pytest.mark.parametrize('case', _skip.PIN_CASES, ids=_skip.pin_tag)
def test_restatement_reproduces_the_reference_mixedop_with_its_identity_layer(recorded, case):
    o, x, r, la, seed = _skip.pin_case(case)
    res = _skip.pin_run(o, x, r, la, seed)
    tag = _skip.pin_tag(case)
    rec = _kinds.pin_record(res)
    assert sorted(rec) == sorted(n[len(tag) + 1:] for n in recorded.files if n.startswith(tag + '/'))
    nskip = sum(_skip.is_skip(c) for c in case[0])
    assert nskip >= 1 and res['dla'].shape == (len(case[0]),)
    assert float(np.abs(res['dla'][-nskip:]).min()) > 0                      # the skip slots get a gradient
    assert list(res['lats'][-nskip:]) == [0.0] * nskip and float(res['lats'][:-nskip].min()) > 0
    assert not any(k.startswith('g%d.' % g) for g in range(len(case[0]) - nskip, len(case[0])) for k in rec)
    for n, v in rec.items():                     # (sum, sum of magnitudes, 24 sampled elements)
        want = recorded[tag + '/' + n]
        assert v.shape == want.shape
        assert abs(v[0] - want[0]) <= RTOL * want[1] and abs(v[1] - want[1]) <= RTOL * want[1], (tag, n)
        scale = max(float(np.abs(want[2:]).max()), 1e-300)
        assert float(np.abs(v[2:] - want[2:]).max()) <= RTOL * scale, (tag, n)


def test_fixture_holds_data_only_and_is_small():
    path = os.path.join(_golden.GOLDEN, 'skip_pin.npz')
    fx = np.load(path, allow_pickle=False)
    assert os.path.getsize(path) <= 200 * 1024
    for n in fx.files:
        assert fx[n].dtype == np.float64, (n, fx[n].dtype)
    assert {n.split('/')[0] for n in fx.files} == {_skip.pin_tag(c) for c in _skip.PIN_CASES}


@pytest.mark.parametrize('cands,geom,act', _skip.KINKED_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_kinked_gpu_cases_find_a_kink_clear_seed(cands, geom, act):
    o, x, r, w, seed = _skip.case_data(cands, *geom, act)                # (AssertionError after 200 tries)
    assert 300 <= seed < 500 and _kinds.kink_distance(o, x) >= _kinds.KINK_TAU
    assert _skip.case_data(cands, *geom, act)[4] == seed                 # the GPU tests see the same seed
    # the skip adds nothing to the distance: it is that of the cell without it
    assert _kinds.kink_distance(_skip.without_skips(o), x) == _kinds.kink_distance(o, x)


def test_identity_candidate_is_the_input_and_the_residual_identity_holds():
    """out = sum_{computing} w_g (BN3_g(...) + x) + w_skip x: the restatement with a skip equals the restatement without it
    plus w_skip x -- the arithmetic the library's launch sequence relies on."""
    o, x, r, w, _ = _skip.case_data(_skip.MNFS, *_skip.SMALL_GEOM, 'swish')
    o64, x64, w64 = o.double(), x.double(), w.double()
    with torch.no_grad():
        full = o64(x64, w64)
        part = _skip.without_skips(o64)(x64, w64[:3])
    assert float((full - (part + w64[3] * x64)).abs().max()) <= 1e-13 * float(full.abs().max())
    assert o64.m_ops[3](x64) is x64 and not list(o64.m_ops[3].parameters())
