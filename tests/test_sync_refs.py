"""CPU checks of the two-rank model the sync-stats GPU tests rest on (tests/_syncref.py, tests/test_gpu_sync_cells.py).  For every
case: the float32 restatement on the joint batch sits within a quarter of the gate (2e-5 + 1e-4 max|ref|) of the float64 one, so
the gate measures the kernels and not the reference; the chosen seed keeps every float64 pre-activation KINK_TAU from every kink
of the cell's activation, so nothing is masked at all (the suite's cap on masked elements is 2 %); and the shards differ enough:
shard a normalised with its OWN statistics misses the gate by at least 10x -- the twin, for the cell as a whole, of the GPU
file's "every site matters".  The call sequence a descriptor implies is checked against tables written out by hand."""
import ctypes as C
import os

import pytest

import _kinds
import _syncref as sr


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _distinct():
    """cases that differ in their route bits alone share data and reference: one of each"""
    seen, out = set(), []
    for name, case in sr.CASES.items():
        if case.key not in seen:
            seen.add(case.key)
            out.append(name)
    return out


@pytest.mark.parametrize('name', _distinct())
def test_reference_is_tight_clear_of_kinks_and_the_shards_differ(name):
    case = sr.CASES[name]
    dt, ref = sr.case_data(case), sr.reference(case)
    y, dx, dw, grads = sr.f32_joint(case)
    res = dict(out=sr.ratio(y, ref.y), dx=sr.ratio(dx, ref.dx), dwmix=sr.ratio(dw, ref.dwmix))
    assert sorted(grads) == sorted(ref.grads)
    res.update({k: sr.ratio(grads[k], ref.grads[k]) for k in grads})
    bad = {k: v for k, v in res.items() if not v <= 0.25}
    assert not bad, bad
    # no element is masked: the kink distance of the JOINT run (which every launch of the case shares) clears KINK_TAU
    if name in sr.KINKED:
        assert sr.kink_distance(case, dt.o, dt.x) >= _kinds.KINK_TAU and sr.branches_ok(case, dt.o, dt.x)
    assert dt.x.shape[0] == 2 * sr.N_RANK and dt.r.shape[0] == 2 * sr.N_RANK
    # per-channel statistics of the two shards differ in EVERY input channel
    xa, xb = dt.x[:dt.n], dt.x[dt.n:]
    assert float((xa.mean((0, 2, 3)) - xb.mean((0, 2, 3))).abs().min()) > 0.1
    # the per-shard sums the forward tables are held to: D and P of every computing candidate, E of the plain ones alone
    want = set()
    for g, c in enumerate(sr._skip.computing(case.cands)):
        want |= {'g%d.%s' % (g, t) for t in (('E', 'D', 'P') if c[0] == 'M' else ('D', 'P'))}
    assert set(ref.shard[0]) == set(ref.shard[1]) == want
    # shard a with its own statistics is far from its half of the joint run
    miss = sr.ratio(sr.local_stats_first_half(case), ref.y[:dt.n])
    assert miss >= 10.0, miss


def test_kinked_cases_cover_relu_relu6_and_hard_swish():
    assert sorted((sr.CASES[n].act, sr.CASES[n].style) for n in sr.KINKED) == [
        ('h-swish', None), ('relu', None), ('relu6', None), ('swish', ('relu', 'h-sigmoid'))]


def test_route_words_of_the_cases():
    from tfnas_amd import _lib
    assert sr.CASES['plain_res_9x11_foldoff'].route == _lib.ROUTE_FOLD_OFF == sr.CASES['three_s1_foldoff'].route
    assert sr.CASES['plain_ring_14x14_tiled'].route == _lib.ROUTE_DW['tiled']


# hand-written: (case, M, forward calls, backward calls).  Offsets in doubles: stats = stats1[M][2] | stats2[M][2] | stats3[G oc][2],
# red = red3[G oc][2] | resdot[oc] | red2[M][2] | red1[M][2] (include/tfnas_hip.h); groups start at multiples of 32 columns.
HAND = [
    # two plain groups, mids 22 and 24 -> columns 0.. and 32..: M = 64; oc = 8: stats3 / red3 2 * 2 * 8 = 32, resdot 8
    ('relu_plain', 64, [('stats', 0, 128), ('stats', 128, 128), ('stats', 256, 32)],
     [('red', 0, 32), ('red', 40, 128), ('red', 168, 128)]),
    # plain + expand-free + fused at stride 2, oc = 12: M = 96, 2 * 3 * 12 = 72, resdot 12; the plain group brings site 0
    ('three_s2', 96, [('stats', 0, 192), ('stats', 192, 192), ('stats', 384, 72)],
     [('red', 0, 72), ('red', 84, 192), ('red', 276, 192)]),
    # the same three kinds and a skip group: the tables are the three computing groups' (2 * 3 * 8 = 48)
    ('mnfs', 96, [('stats', 0, 192), ('stats', 192, 192), ('stats', 384, 48)],
     [('red', 0, 48), ('red', 56, 192), ('red', 248, 192)]),
    # one expand-free group: no BatchNorm site 0 -- no stats1 and no red1 call; stats2 keeps its offset
    ('N_s1', 32, [('stats', 64, 64), ('stats', 128, 16)], [('red', 0, 16), ('red', 24, 64)]),
]


@pytest.mark.parametrize('name,M,fwd,bwd', HAND, ids=[h[0] for h in HAND])
def test_expected_call_sequence_matches_a_hand_written_table(lib, name, M, fwd, bwd):
    from tfnas_amd import _lib
    case = sr.CASES[name]
    ic, oc, H, W, s = case.geom
    d = sr.cell_desc(case.cands, sr.N_RANK, H, W, ic, oc, s, case.act, sr.Hook('record'), case.route, case.style)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    ws = _lib.TfnasCellWs()
    assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == 0
    G, has_plain = sr.groups_of(case.cands)
    assert d.M == M
    assert sr.expected_calls(G, has_plain, d.M, d.oc, ws) == (fwd, bwd)
    assert sr.expected_calls(G, has_plain, d.M, d.oc, ws, want_dx=False, need_wgrad=True) == (fwd, bwd)
    assert sr.expected_calls(G, has_plain, d.M, d.oc, ws, want_dx=True, need_wgrad=False) == (fwd, bwd)
    # d wmix alone: the backward returns after the BN3 sums
    assert sr.expected_calls(G, has_plain, d.M, d.oc, ws, want_dx=False, need_wgrad=False) == (fwd, bwd[:1])
    # with a hook a cell with a plain group needs its E buffer, whatever need_wgrad says
    assert (ws.E > 0) == has_plain


def test_head_reference_is_tight_and_its_shards_differ():
    import copy
    dt, ref = sr.head_data(), sr.head_reference()
    f32 = sr.head_run(copy.deepcopy(dt.o), dt.x, dt.r)
    bad = {k: sr.ratio(f32[k], ref.res[k]) for k in f32}
    assert all(v <= 0.25 for v in bad.values()), bad
    own = sr.head_run(copy.deepcopy(dt.o).double(), dt.x[:dt.n].double(), dt.r[:dt.n].double())
    assert sr.ratio(own['pooled'], ref.res['pooled'][:dt.n]) >= 10.0
    assert sr.HEAD_GEOM[1] % 4 == 0 and ref.shard[0].shape == (sr.HEAD_GEOM[1], 2)
