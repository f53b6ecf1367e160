"""Residual cells with a skip (identity) candidate (TFNAS_CELL_SKIP: TFNAS_GROUP_SKIP groups after the computing ones) against the
float32 CPU restatement of tests/_skip.py -- _kinds.MixedRef with an identity module in the skip slots: out, dx, every entry of
d wmix (the skip entries included) and every weight gradient, with need_wgrad 0 and 1, through MixedOpFn and through the raw ABI.

Shapes are the smallest that reach each way the launch sequence can go wrong: every kind beside a skip under every activation; one
and two skips behind seven and six computing groups; ic = oc = 40 (another row-lane split of the BN3-backward sums than oc = 8) with
one plain group and with two -- all-plain computing groups must still take the mixed route, where the residual gradient is added
once over ALL mix weights; the late cell the fused per-image route would take without the skip.  Bit for bit: the bit without a
skip group changes nothing, and a skip of weight 0 changes no bit of anything but its own d wmix entry.
Gate: _hipcheck.worst (atol 2e-5 + rtol 1e-4 * max|ref|), no element exempted; kinked activations at seeds that keep every float64
pre-activation KINK_TAU from a kink (tests/test_skip_oracle_pin.py asserts they are found)."""
import pytest
import torch

import _hipcheck as hc
import _kinds
import _skip
from _skip import S

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(cands, geom, act='swish'):
    """case_data and the restatement's results, computed once and shared (never changed) by the tests that need them"""
    key = (tuple(cands), tuple(geom), act)
    if key not in _CACHE:
        o, x, r, w, seed = _skip.case_data(cands, *geom, act)
        if act != 'swish':
            assert _kinds.kink_distance(o, x) >= _kinds.KINK_TAU
        _CACHE[key] = (o, x, r, w, _kinds.ref_run(o, x, r, w))
    return _CACHE[key]


def _report(tag, res):
    print(tag, ' '.join('%s=%.2e/%.2e' % (k, v[0], v[1]) for k, v in res.items()))


def _check(tag, cands, geom, act='swish', wgrad=(0, 1)):
    from tfnas_amd import _lib
    o, x, r, w, ref = _case(cands, geom, act)
    plan = _skip.hip_plan(o)
    d, ws = plan.desc(geom[0], geom[3], geom[4])
    nskip = sum(_skip.is_skip(c) for c in cands)
    assert d.flags & _lib.CELL_KINDS and d.flags & _lib.CELL_SKIP and d.G == len(cands)
    assert ws.Pr == (len(cands) - nskip) * geom[0] * geom[3] * geom[4] * geom[2]            # no Pr slot for a skip
    for need_w in wgrad:
        got = _kinds.hip_run(plan, x, r, w, bool(need_w))
        assert got[2].shape == (len(cands),)
        res = _kinds.compare(ref, got)
        res['dwmix_skip'] = hc.err(got[2][-nskip:], ref[2][-nskip:])
        _report('%s w%d' % (tag, need_w), res)
        assert (len(res) > 4) == bool(need_w)
        bad = hc.worst(res)
        assert not bad, bad


@pytest.mark.parametrize('act', _kinds.PIN_ACTS)
def test_every_kind_beside_a_skip(act):
    _check('MNFS %s' % act, _skip.MNFS, _skip.SMALL_GEOM, act)


@pytest.mark.parametrize('cands', [_skip.EIGHT_S, _skip.EIGHT_SS], ids=('seven_and_a_skip', 'six_and_two_skips'))
def test_eight_candidates_ending_in_skips(cands):
    _check('eight', cands, _skip.SMALL_GEOM)


@pytest.mark.parametrize('cands', _skip.WIDE_CASES, ids=('one_plain', 'two_plain'))
def test_all_plain_computing_groups_take_the_mixed_route(cands):
    _check('wide', cands, _skip.WIDE_GEOM)


def test_late_cell_with_a_skip_gives_up_the_fused_per_image_route():
    import ctypes as C
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan
    o, x, r, w, ref = _case(_skip.FX_CANDS + [S], _skip.FX_GEOM)
    blocks = _skip.hip_blocks_like(o)
    plain = CellPlan(80, 80, 1, 'swish', blocks[:2], mixed_kinds=True)
    assert _lib.lib().tfnas_fx_supported(C.byref(plain.desc(8, 14, 14)[0])) == 1          # frozen weights, without the skip
    plan = _skip.hip_plan(o, blocks)
    assert _lib.lib().tfnas_fx_supported(C.byref(plan.desc(8, 14, 14)[0])) == 0
    _check('late', _skip.FX_CANDS + [S], _skip.FX_GEOM, wgrad=(0,))


# ------------------------------------------------------------------------------------------------ bit for bit
def _run_plan(plan, x, r, w):
    from tfnas_amd.functions import MixedOpFn
    params = plan.params()
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wm = w.cuda().requires_grad_(True)
    y = MixedOpFn.apply(plan, xm, wm, *params)
    (y * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    return [y.detach().clone(), xm.grad.clone(), wm.grad.clone()] + [p.grad.clone() for p in params]


@pytest.mark.parametrize('cands', [_kinds.THREE, _kinds.EIGHT], ids=('three', 'eight'))
def test_the_bit_without_a_skip_group_changes_no_bit(cands):
    from tfnas_amd import _lib
    o, x, r, w, _ = _case(cands, _skip.SMALL_GEOM)
    blocks = _kinds.hip_blocks_like(o)
    old, new = _kinds.hip_plan(o, blocks), _kinds.hip_plan(o, blocks)
    mark = new._mark

    def with_bit(d):
        mark(d)
        d.flags |= _lib.CELL_SKIP
    new._mark = with_bit
    dn, do = new.desc(2, 7, 9)[0], old.desc(2, 7, 9)[0]
    assert dn.flags == do.flags | _lib.CELL_SKIP and do.flags & _lib.CELL_KINDS
    a, b = _run_plan(old, x, r, w), _run_plan(new, x, r, w)
    assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize('cands', [_skip.MNFS, _skip.EIGHT_S], ids=('MNFS', 'eight'))
def test_a_skip_of_weight_zero_changes_no_bit_but_its_own_dwmix(cands):
    """trailing + 0.f terms change no bit of the sum of the mix weights; the computing groups differ in kind, so the cell without
    its skip is a mixed launch too"""
    o, x, r, w, _ = _case(cands, _skip.SMALL_GEOM)
    blocks = _skip.hip_blocks_like(o)
    G1 = len(cands) - 1
    w0 = w.clone()
    w0[G1] = 0.0
    with_skip = _run_plan(_skip.hip_plan(o, blocks), x, r, w0)
    without = _run_plan(_kinds.hip_plan(_skip.without_skips(o), blocks[:G1]), x, r, w0[:G1])
    assert torch.equal(with_skip[0], without[0]) and torch.equal(with_skip[1], without[1])
    assert torch.equal(with_skip[2][:G1], without[2])
    assert len(with_skip) == len(without) and all(torch.equal(s, t) for s, t in zip(with_skip[3:], without[3:]))
    dot = (r.double() * x.double()).sum()
    res = dict(dwmix_skip=hc.err(with_skip[2][G1:], dot.reshape(1)))
    _report('w0', res)
    assert not hc.worst(res), hc.worst(res)


# ------------------------------------------------------------------------------------------------ raw ABI
def _raw(cands=_skip.EIGHT_S):
    o, x, r, w, ref = _case(cands, _skip.SMALL_GEOM)
    return o, x, r, w, ref, _skip.RawSkip(o, x, w)


def _raw_res(ref, out, dx, dw, grads):
    res = dict(out=hc.err(out, ref[0]), dwmix=hc.err(dw, ref[2]))
    if dx is not None:
        res['dx'] = hc.err(dx, ref[1])
    if grads is not None:
        assert sorted(grads) == sorted(ref[3])
        res.update({k: hc.err(grads[k], ref[3][k]) for k in grads})
    return res


@pytest.mark.parametrize('cands', [_skip.EIGHT_S, _skip.MSS], ids=('eight', 'MSS'))
def test_raw_launch_guard_bands_with_buffers_sized_for_the_computing_groups(cands):
    o, x, r, w, ref, cell = _raw(cands)
    Gc = len(_skip.computing(cands))
    assert cell.ws.Pr == Gc * 2 * 7 * 9 * 8 and cell.ws.stats == 4 * cell.d.M + 2 * Gc * 8 and cell.d.G == len(cands)
    out = cell.forward()
    assert all(cell.guards_ok().values()), cell.guards_ok()
    rc, dx, dw, g = cell.backward(r)
    assert rc == 0 and all(cell.guards_ok().values()), cell.guards_ok()
    assert dw.shape == (len(cands),)
    res = _raw_res(ref, out, dx, dw, g)
    _report('raw', res)
    assert not hc.worst(res), hc.worst(res)
    # two identical launches: bit-identical results
    keep = [dx.clone(), dw.clone()] + [t.clone() for t in g.values()]
    out2 = cell.forward()
    rc, dx2, dw2, g2 = cell.backward(r)
    assert rc == 0 and torch.equal(out2, out)
    assert all(torch.equal(s, t) for s, t in zip(keep, [dx2, dw2] + list(g2.values())))


def test_raw_accumulation_adds_exactly_what_the_plain_launch_stores():
    o, x, r, w, ref, cell = _raw()
    cell.forward()
    rc, _, _, g1 = cell.backward(r)
    assert rc == 0
    base = [torch.full_like(t, 0.25) for t in g1.values()]
    rc, _, _, g2 = cell.backward(r, accum_into=base)
    assert rc == 0
    res = {k: hc.err(g2[k], b + g1[k]) for k, b in zip(g1, base)}           # (the stores of the plain launch, added)
    res.update({'ref.' + k: hc.err(g1[k], ref[3][k]) for k in g1})
    _report('accum', res)
    assert not hc.worst(res), hc.worst(res)


def test_raw_dx_null_and_dwmix_only_fill_the_skip_entry():
    o, x, r, w, ref, cell = _raw()
    out = cell.forward()
    rc, dx, dw, g = cell.backward(r, want_dx=False)                  # dx == NULL: weight gradients and d wmix all the same
    assert rc == 0 and dx is None
    res = _raw_res(ref, out, None, dw, g)
    assert not hc.worst(res), hc.worst(res)
    rc, dx, dw, g = cell.backward(r, need_wgrad=False)               # frozen weights: dx and d wmix
    assert rc == 0 and g is None
    res = _raw_res(ref, out, dx, dw, None)
    assert not hc.worst(res), hc.worst(res)
    rc, dx, dw, g = cell.backward(r, need_wgrad=False, want_dx=False)   # only d wmix: returns after the BN3 sums
    assert rc == 0 and all(cell.guards_ok().values())
    res = dict(dwmix=hc.err(dw, ref[2]), dwmix_skip=hc.err(dw[-1:], ref[2][-1:]))
    assert not hc.worst(res), hc.worst(res)
