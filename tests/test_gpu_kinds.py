"""Cells whose candidates differ in kind (TFNAS_CELL_KINDS: plain MBConv, expand-free and Fused-MBConv groups in ONE launch) against
the float32 CPU restatement of tests/_kinds.py -- the weighted sum of the oracle's MBConv blocks and _fused.FusedRef: out, dx,
d wmix and every weight gradient of every candidate, with need_wgrad 0 and 1.

Shapes are the smallest that reach each way the launch sequence can go wrong: every kind beside every other (the kinds' fronts
write their own columns of D and stats2, their tails their own columns of dEh, and dx is summed over the branches); ragged widths
and a fused block of mid == in; 7 x 9 images at both strides and an even width; 588 rows (four full 128-row GEMM tiles and a ragged
fifth) with the residual gradient added once; K = 180 (a tap boundary inside a chunk); no plain group (no E buffer); eight fused
groups.  ReLU, ReLU6 and hard-swish on 3-candidate cells whose seeds keep every float64 pre-activation KINK_TAU from a kink
(asserted below on the CPU restatement alone); everything larger is swish.
Gate: _hipcheck.worst (atol 2e-5 + rtol 1e-4 * max|ref|), no element exempted."""
import pytest
import torch

import _hipcheck as hc
import _kinds

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(cands, N, ic, oc, H, W, stride, act='swish', base=300):
    """case_data and the restatement's results, computed once and shared (never changed) by the tests that need them"""
    key = (tuple(cands), N, ic, oc, H, W, stride, act, base)
    if key not in _CACHE:
        o, x, r, w, seed = _kinds.case_data(cands, N, ic, oc, H, W, stride, act, base)
        if act != 'swish':
            assert _kinds.kink_distance(o, x) >= _kinds.KINK_TAU
        _CACHE[key] = (o, x, r, w, _kinds.ref_run(o, x, r, w))
    return _CACHE[key]


def _report(tag, res):
    print(tag, ' '.join('%s=%.2e/%.2e' % (k, v[0], v[1]) for k, v in res.items()))


def _check(tag, cands, geom, act='swish'):
    o, x, r, w, ref = _case(cands, *geom, act=act)
    plan = _kinds.hip_plan(o)
    assert plan.group_kinds is not None
    for need_w in (0, 1):
        got = _kinds.hip_run(plan, x, r, w, bool(need_w))
        res = _kinds.compare(ref, got)
        _report('%s w%d' % (tag, need_w), res)
        assert (len(res) > 3) == bool(need_w)
        bad = hc.worst(res)
        assert not bad, bad


@pytest.mark.parametrize('geom', _kinds.EIGHT_SHAPES, ids=lambda g: 'n%d_ic%d_oc%d_%dx%d_s%d' % g)
def test_eight_candidates_of_three_kinds(geom):
    _check('eight', _kinds.EIGHT, geom)


@pytest.mark.parametrize('act', _kinds.KINKED_ACTS)
@pytest.mark.parametrize('stride', (1, 2))
def test_three_candidates_with_kinked_activations(act, stride):
    _check('three %s s%d' % (act, stride), _kinds.THREE, _kinds.SMALL_SHAPE + (stride,), act)


@pytest.mark.parametrize('cands,geom', [(_kinds.TILE5, (3, 24, 24, 14, 14, 1)), (_kinds.TILE5, (3, 24, 24, 7, 7, 2)),
                                        ([('M', 36, 3, 0), ('F', 36, 0)], (2, 20, 20, 9, 13, 1))],
                         ids=('tiles_s1_res', 'tiles_s2', 'tap_k180'))
def test_tile_and_tap_boundaries(cands, geom):
    _check('tiles', cands, geom)


@pytest.mark.parametrize('cands', [[('F', 22, 8), ('N', 5, 0)], [('N', 3, 8), ('N', 5, 0), ('F', 10, 0)],
                                   [('F', m, 8 if m == 22 else 0) for m in (5, 9, 22, 31, 8, 13, 50, 7)]],
                         ids=('fused_noexp', 'noexp_noexp_fused', 'eight_fused'))
@pytest.mark.parametrize('stride', (1, 2))
def test_sets_without_a_plain_group(cands, stride):
    o, x, r, w, ref = _case(cands, *_kinds.SMALL_SHAPE, stride)
    d, ws = _kinds.hip_plan(o).desc(2, 7, 9)
    assert ws.E == 0                                              # no E buffer at all
    _check('noE s%d' % stride, cands, _kinds.SMALL_SHAPE + (stride,))


# ------------------------------------------------------------------------------------------------ canonical forms: bit for bit
def _run_plan(plan, x, r, w):
    from tfnas_amd.functions import MixedOpFn
    params = plan.params()
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wm = None if w is None else w.cuda().requires_grad_(True)
    y = MixedOpFn.apply(plan, xm, wm, *params)
    (y * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    return [y.detach().clone(), xm.grad.clone()] + ([] if wm is None else [wm.grad.clone()]) + [p.grad.clone() for p in params]


def _force_kinds(plan):
    """the same plan handing the library TFNAS_CELL_KINDS descriptors (every group names its block's own kind)"""
    from tfnas_amd import _lib
    plan.group_kinds = tuple(b.kind for b in plan.blocks)
    if len(plan.blocks) == 1:                                     # (the one-block bit must be clear beside TFNAS_CELL_KINDS)
        plan.kind, plan._kind_arg = _lib.MBCONV, (_lib.MBCONV,)
    plan._desc_cache = {}
    return plan


@pytest.mark.parametrize('cand', [('M', 22, 5, 8), ('N', 5, 8), ('F', 22, 8)], ids=lambda c: c[0])
@pytest.mark.parametrize('stride', (1, 2))
def test_one_group_flagged_cell_equals_its_one_block_flag_bitwise(cand, stride):
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan
    o, x, r, w, _ = _case([cand], *_kinds.SMALL_SHAPE, stride)
    blocks = _kinds.hip_blocks_like(o)
    old = CellPlan(8, 8, stride, 'swish', blocks)
    new = _force_kinds(CellPlan(8, 8, stride, 'swish', blocks))
    dn, do = new.desc(2, 7, 9)[0], old.desc(2, 7, 9)[0]
    assert dn.flags & _lib.CELL_KINDS and not do.flags & _lib.CELL_KINDS and dn.g[0].kind == _lib.group_kind_id(blocks[0].kind)
    a, b = _run_plan(old, x, r, None), _run_plan(new, x, r, None)
    assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def test_all_plain_flagged_cell_equals_the_unflagged_launch_bitwise():
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan
    cands = [('M', m, k, se) for m, k, se in ((22, 3, 0), (44, 3, 0), (24, 5, 0), (36, 5, 0), (22, 3, 8), (50, 3, 16), (30, 5, 8),
                                              (41, 5, 16))]
    o, x, r, w, ref = _case(cands, 2, 8, 8, 7, 9, 1)
    blocks = _kinds.hip_blocks_like(o)
    old = CellPlan(8, 8, 1, 'swish', blocks, mixed_kinds=True)
    assert old.group_kinds is None                                # (all plain: the product sets no flag)
    new = _force_kinds(CellPlan(8, 8, 1, 'swish', blocks))
    assert new.desc(2, 7, 9)[0].flags & _lib.CELL_KINDS
    a, b = _run_plan(old, x, r, w), _run_plan(new, x, r, w)
    assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


# ------------------------------------------------------------------------------------------------ raw ABI
def _raw(stride=1):
    o, x, r, w, ref = _case(_kinds.EIGHT, 2, 8, 8, 7, 9, stride)
    return o, x, r, w, ref, _kinds.RawMixed(o, x, w)


def _raw_res(ref, out, dx, dw, grads):
    res = dict(out=hc.err(out, ref[0]), dwmix=hc.err(dw, ref[2]))
    if dx is not None:
        res['dx'] = hc.err(dx, ref[1])
    if grads is not None:
        assert sorted(grads) == sorted(ref[3])            # (hip_params() order there, named_parameters() order here)
        res.update({k: hc.err(grads[k], ref[3][k]) for k in grads})
    return res


@pytest.mark.parametrize('stride', (1, 2))
def test_raw_launch_guard_bands_and_reproducibility(stride):
    o, x, r, w, ref, cell = _raw(stride)
    out = cell.forward()
    assert all(cell.guards_ok().values()), cell.guards_ok()
    rc, dx, dw, g = cell.backward(r)
    assert rc == 0 and all(cell.guards_ok().values()), cell.guards_ok()
    res = _raw_res(ref, out, dx, dw, g)
    _report('raw s%d' % stride, res)
    assert not hc.worst(res), hc.worst(res)
    # two identical launches: dx is summed over the branches in a fixed order, so every result is bit-identical
    keep = [dx.clone(), dw.clone()] + [t.clone() for t in g.values()]
    out2 = cell.forward()
    rc, dx2, dw2, g2 = cell.backward(r)
    assert rc == 0 and torch.equal(out2, out)
    assert all(torch.equal(s, t) for s, t in zip(keep, [dx2, dw2] + list(g2.values())))


def test_raw_accumulation_over_two_backward_passes():
    o, x, r, w, ref, cell = _raw()
    ref2 = _kinds.ref_run(o, x, 0.5 * r, w)
    cell.forward()
    rc, _, _, g1 = cell.backward(r)
    assert rc == 0
    rc, _, _, g12 = cell.backward(0.5 * r, accum_into=list(g1.values()))
    assert rc == 0
    res = {k: hc.err(g12[k], ref[3][k] + ref2[3][k]) for k in g12}
    _report('accum', res)
    assert not hc.worst(res), hc.worst(res)


def test_raw_dx_null_and_dwmix_only():
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
    rc, dx, dw, g = cell.backward(r, need_wgrad=False, want_dx=False)   # only d wmix: returns after the BN3 sums (4-float dZ / dEh)
    assert rc == 0 and all(cell.guards_ok().values())
    res = dict(dwmix=hc.err(dw, ref[2]))
    assert not hc.worst(res), hc.worst(res)


# ------------------------------------------------------------------------------------------------ module level
def test_mixedop_with_primitives_soft_and_sampled():
    from tfnas_amd.functions import ArchFn  # noqa: F401  (the soft forward goes through it)
    import tfnas_oracle as orc
    cands = [('M', 22, 3, 0), ('F', 22, 8), ('N', 5, 0), ('M', 44, 5, 8), ('F', 36, 0), ('N', 3, 8), ('M', 24, 7, 0), ('F', 8, 0)]
    o, x, r, _, _ = _case(cands, 2, 8, 8, 7, 9, 1)
    m = _kinds.hip_mixedop_like(o)
    gen = torch.Generator().manual_seed(11)
    la = torch.log_softmax(torch.randn(8, generator=gen) * 0.5, -1)
    e = torch.empty(8).exponential_(generator=gen)
    with torch.no_grad():
        m.log_alphas.copy_(la)
    for p in m.parameters():
        p.requires_grad_(False)
    m.log_alphas.requires_grad_(True)
    # restatement: gumbel-softmax weights from the same noise, the weighted sum, d log_alphas by autograd
    la_o = la.clone().requires_grad_(True)
    xo = x.clone().requires_grad_(True)
    w_o = orc.gumbel_softmax(la_o, m.T, e)
    y_o = o(xo, w_o)
    lats = torch.tensor(m.get_lookup_latency(9))
    lat_o = (w_o * lats).sum()
    ((y_o * r).sum() + 0.3 * lat_o).backward()
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y_m, lat_m = m(xm, False, None, exp_noise=e.cuda())
    ((y_m * r.cuda()).sum() + 0.3 * lat_m).backward()
    res = dict(out=hc.err(y_m, y_o), dx=hc.err(xm.grad, xo.grad), dla=hc.err(m.log_alphas.grad, la_o.grad),
               lat=hc.err(lat_m, lat_o))
    _report('mixedop', res)
    assert not hc.worst(res), hc.worst(res)
    # the sampled forward of each kind equals that candidate alone
    for idx in (0, 1, 2):
        m._pre = idx
        y, lat = m(xm.detach(), True, 'random')
        want = o.m_ops[idx](x)
        assert lat == 0 and not hc.worst(dict(y=hc.err(y, want)))
