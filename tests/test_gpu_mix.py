"""GPU parity of MixConv candidates (a packed TfnasGroup.k under TFNAS_CELL_MIXK: the LDS tile kernels take their channel chunk
from a SEGMENT): cells with MixConv candidates (sampled launches with weight gradients, soft launches that mix k3, k5, k7, k35,
k357 and a dilated k3), expand-free MixConv cells, a cell of several kinds, the derived-network block and a derived network,
against the CPU restatement of tests/_mix.py (pinned to the reference in tests/test_mix_oracle_pin.py).

Cells of plain candidates: every stage is compared with _hipcheck.check_cell at its default gate (abs err <= 2e-5 + 1e-4 *
max|ref| per tensor), ReLU decisions replayed, no kink exemption (a cell with a packed group never takes the E-free route).
Expand-free and mixed-kind cells: the same gate on out, dx, dwmix and every gradient, with seeds whose float64 pre-activations
stay 1e-4 from every kink (chosen from the restatement alone, nothing exempted).  Shapes: the table of tests/test_gpu_dil.py (the
largest extent here is 7: its small cases bracket it), with mids whose SEGMENT widths are no multiple of 16, 32 or 64 (44 -> 24 |
20 and 20 | 12 | 12, 53 -> 28 | 25 and 24 | 16 | 13, 107 -> 56 | 51 and 36 | 36 | 35) and one cell whose MixConv candidates have
exactly one channel quad per segment.  The affine block is held to the gate of tests/test_gpu_affine_f64.py against a float64 run
of the restatement.

Segment identity (derived, not measured): the per-channel arithmetic of the depthwise tile kernel does not depend on which chunk
holds the channel, so the forward's D columns of a k35 group equal BIT FOR BIT those of a plain k3 and a plain k5 group of the same
width built from the same expand and depthwise weights (likewise k357).  A wrong segment bound shows here: the overhanging lanes of
a segment's last chunk are the next segment's columns, which another launch writes."""
import copy
import ctypes as C
from collections import OrderedDict

import pytest
import torch

import _affineref as ar
import _hipcheck as hc
import _kinds
import _mix
import _rawcell
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [
    # name, N, ic, oc, H, W, stride, act, mids
    ('img_1x1', 5, 16, 16, 1, 1, 1, 'swish', [20, 33, 24, 40, 17, 35, 28, 44]),
    ('img_smaller_than_7_res', 2, 16, 16, 3, 5, 1, 'swish', [20, 33, 24, 40, 17, 35, 28, 44]),
    ('img_equals_7', 3, 32, 48, 7, 7, 1, 'swish', [41, 72, 36, 67, 45, 80, 53, 70]),
    ('s2_swish_odd', 2, 24, 40, 9, 13, 2, 'swish', [36, 72, 40, 60, 33, 66, 44, 71]),
    ('s2_relu_even', 2, 16, 24, 12, 10, 2, 'relu', [24, 40, 20, 36, 29, 44, 24, 50]),
    ('s1_relu_two_column_tiles_res', 2, 24, 24, 10, 22, 1, 'relu', [32, 52, 28, 56, 37, 60, 40, 62]),
    ('s2_relu_ragged_tiles_cc16', 1, 16, 24, 37, 41, 2, 'relu', [48, 96] * 4),
    ('s1_swish_odd_widths_res', 3, 40, 40, 8, 6, 1, 'swish', [53, 107, 44, 88, 61, 96, 48, 79]),
]
_BY_NAME = {c[0]: c for c in SHAPES}
_IDS = [c[0] for c in SHAPES]


def _inputs(cfg, specs=_mix.SOFT):
    name, N, ic, oc, H, W, s, act, mids = cfg
    o, m = _mix.make_cell_pair(ic, oc, s, act, mids, specs=specs, seed=len(name))
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, ic, H, W, generator=g)
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=g)
    e = torch.empty(8).exponential_(generator=g)
    return o, m, x, r, e


def _check_segments(o, m, res_params, idx):
    """every g_dw segment against its own slice of the restatement's gradient (gate per SEGMENT, not per packed tensor)"""
    op = o.m_ops[idx]
    got, want = res_params
    ks, mc = _mix.mix_of(op), op.mid_channels
    out = OrderedDict()
    for s, (a, b) in enumerate(zip(_mix.segments(got, mc, ks), _mix.segments(want, mc, ks))):
        out['g%d.grad_dw.seg%d' % (idx, s)] = hc.err(a, b)
    return out


def _run(m, x, r, e, idxs, modes, want_dx=True, need_wgrad=True):
    from tfnas_amd import functions as F
    from tfnas_amd.functions import MixedOpFn
    F.adopt_modes(m, modes)
    plan = m._plan(tuple(idxs))
    ps = plan.params()
    for p in ps:
        p.requires_grad_(need_wgrad)
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(want_dx)
    w = torch.softmax(-e.log(), 0).cuda().requires_grad_(True) if len(idxs) > 1 else None
    MixedOpFn.debug_sink, MixedOpFn.fwd_sink = [], []
    try:
        out = MixedOpFn.apply(plan, xm, w, *ps)
        (out * r.cuda()).sum().backward()
        torch.cuda.synchronize()
        dbg, frec = MixedOpFn.debug_sink[0], MixedOpFn.fwd_sink[0]
    finally:
        MixedOpFn.debug_sink = MixedOpFn.fwd_sink = None
    got = OrderedDict(out=out.detach().clone())
    if want_dx:
        got['dx'] = xm.grad.clone()
    if need_wgrad:
        for i, p in enumerate(ps):
            got['p%d' % i] = p.grad.clone()
    if w is not None:
        got['dwmix'] = w.grad.clone()
    for p in ps:
        p.grad = None
    return got, dbg, frec


@pytest.mark.parametrize('cfg', SHAPES, ids=_IDS)
@pytest.mark.parametrize('idx', [4, 7], ids=['k35_se', 'k357_se'])
def test_sampled_mixconv_candidate_with_weight_grads(cfg, idx):
    """one MixConv candidate with squeeze-excite (G = 1), weight gradients wanted; every g_dw segment against its own slice"""
    from tfnas_amd import _lib
    o, m, x, r, e = _inputs(cfg)
    ks = _mix.SOFT[idx]
    assert _mix.mix_of(o.m_ops[idx]) == ks == m.m_ops[idx].mix_kernels and o.m_ops[idx].se_channels
    res = hc.check_cell(o, m, x, r, e, [idx], need_wgrad=True)
    assert 'g%d.grad_dw' % idx in res and 'g%d.dEh' % idx in res and 'kink_fraction' not in res
    d = m._plan((idx,)).desc(x.shape[0], x.shape[2], x.shape[3])[0]
    assert d.flags & _lib.CELL_MIXK and d.g[0].k == _mix.WORDS[ks]
    # (the packed gradients once more, segment by segment: replayed ReLU decisions as check_cell replays them are not needed for
    # swish; for ReLU the packed comparison above already ran under them, so the per-segment gate is taken on swish cells)
    if cfg[7] == 'swish':
        from tfnas_amd import functions as F
        got, _, _ = _run(m, x, r, e, (idx,), F.HipModes())
        xo = x.clone().requires_grad_(True)
        o.zero_grad()
        (o.m_ops[idx](xo) * r).sum().backward()
        seg = _check_segments(o, m, (got['p1'], o.m_ops[idx].depth_conv.conv.weight.grad), idx)
        assert len(seg) == len(ks) and not hc.worst(seg), hc.worst(seg)


@pytest.mark.parametrize('cfg', [_BY_NAME[n] for n in ('img_smaller_than_7_res', 's2_swish_odd', 's2_relu_ragged_tiles_cc16',
                                                       's1_relu_two_column_tiles_res')], ids=lambda c: c[0])
@pytest.mark.parametrize('idx', [1, 5], ids=['k35', 'k357_se2'])
def test_sampled_mixconv_candidate_k35_without_se_and_k357_wide_se(cfg, idx):
    o, m, x, r, e = _inputs(cfg)
    assert _mix.mix_of(o.m_ops[idx]) == _mix.SOFT[idx] and bool(o.m_ops[idx].se_channels) == (idx == 5)
    res = hc.check_cell(o, m, x, r, e, [idx], need_wgrad=True)
    assert 'kink_fraction' not in res


@pytest.mark.parametrize('cfg', SHAPES, ids=_IDS)
def test_soft_mode_mixing_k3_k5_k7_k35_k357_and_a_dilated_k3(cfg):
    o, m, x, r, e = _inputs(cfg)
    assert [(b.kernel_size, b.dilation, b.mix_kernels) for b in m.m_ops] == [
        (3, 1, None), (5, 1, (3, 5)), (5, 1, None), (7, 1, None), (5, 1, (3, 5)), (7, 1, (3, 5, 7)), (3, 2, None), (7, 1, (3, 5, 7))]
    res = hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=False)
    assert any(k.endswith('.dEh') for k in res) and 'kink_fraction' not in res      # materialised route, nothing exempted


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_relu_two_column_tiles_res'],
                                 _BY_NAME['s1_swish_odd_widths_res']], ids=lambda c: c[0])
def test_soft_mode_weight_grads_share_one_partial_row_matrix(cfg):
    """all eight candidates' depthwise weight gradients from one pass: the launches fill the same partial rows, a packed group's
    block of the row holds its segments back to back"""
    o, m, x, r, e = _inputs(cfg)
    res = hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=True)
    assert all('g%d.grad_dw' % i in res for i in range(8)) and 'kink_fraction' not in res


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_swish_odd_widths_res']], ids=lambda c: c[0])
def test_soft_cell_without_dx_and_without_weight_grads(cfg):
    """dx == NULL (the input wants no gradient) and need_wgrad = 0: what remains equals, bit for bit, the full launch's"""
    from tfnas_amd import functions as F
    o, m, x, r, e = _inputs(cfg)
    idxs = tuple(range(8))
    full, _, _ = _run(m, x, r, e, idxs, F.HipModes())
    nodx, _, _ = _run(m, x, r, e, idxs, F.HipModes(), want_dx=False)
    assert 'dx' not in nodx and set(nodx) == set(full) - {'dx'}
    for k in nodx:
        assert torch.equal(nodx[k], full[k]), k
    frozen, _, _ = _run(m, x, r, e, idxs, F.HipModes(), need_wgrad=False)
    assert set(frozen) == {'out', 'dx', 'dwmix'}
    for k in frozen:
        assert torch.equal(frozen[k], full[k]), k


def test_one_quad_per_segment():
    """q == n: the MixConv candidates have exactly one channel quad per segment (k35: mid 8 -> 4 | 4 and mid 7 -> 4 | 3; k357:
    mid 9 -> 4 | 4 | 1 and mid 12 -> 4 | 4 | 4), sampled with weight gradients and in the soft cell"""
    mids = [20, 8, 24, 40, 7, 9, 28, 12]
    cfg = ('q_eq_n', 3, 4, 4, 6, 7, 1, 'swish', mids)
    o, m, x, r, e = _inputs(cfg)
    assert [b.depth_conv.conv.splits for b in (m.m_ops[1], m.m_ops[4], m.m_ops[5], m.m_ops[7])] == [[4, 4], [4, 3], [4, 4, 1], [4, 4, 4]]
    for idx in _mix.MIX_IDX:
        hc.check_cell(o, m, x, r, e, [idx], need_wgrad=True)
    hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=True)


# ------------------------------------------------------------------------------------------------ segment identity
def _forward_D(blk, x, route):
    """the D tensor [N, Ho, Wo, mc] of one sampled forward of ``blk`` on the materialised tile route (weight gradients wanted: no
    E-free and no fused per-image route; TFNAS_ROUTE_DW tiled: a plain 3 x 3 / 5 x 5 block on the tile kernels too)"""
    from tfnas_amd import functions as F
    from tfnas_amd.functions import CellPlan, MixedOpFn
    F.adopt_modes(blk, F.HipModes(route=route))
    plan = CellPlan(blk.in_channels, blk.out_channels, blk.stride, blk.act_func, [blk])
    ps = plan.params()
    for p in ps:
        p.requires_grad_(True)
    xm = x.cuda().contiguous(memory_format=torch.channels_last)
    MixedOpFn.fwd_sink = []
    try:
        MixedOpFn.apply(plan, xm, None, *ps)
        torch.cuda.synchronize()
        rec = MixedOpFn.fwd_sink[0]
    finally:
        MixedOpFn.fwd_sink = None
    d = rec['d']
    N = x.shape[0]
    assert d.G == 1 and d.g[0].off == 0
    return rec['D'][:N * d.Ho * d.Wo * d.M].view(N, d.Ho, d.Wo, d.M)[..., :d.g[0].mc].clone(), d


IDENTITY = [
    # name, N, ic, oc, H, W, stride, act, mid
    ('s1_44', 2, 24, 24, 10, 22, 1, 'swish', 44),
    ('s2_53', 2, 24, 40, 9, 13, 2, 'relu', 53),
    ('s1_107', 3, 40, 40, 8, 6, 1, 'swish', 107),
    ('s2_cc16_96', 1, 16, 24, 37, 41, 2, 'relu', 100),
    ('q_eq_n_12', 2, 8, 8, 5, 6, 1, 'swish', 12),
]


@pytest.mark.parametrize('case', IDENTITY, ids=lambda c: c[0])
@pytest.mark.parametrize('ks', [(3, 5), (3, 5, 7), (5, 7), (3, 7)], ids=lambda k: 'k' + ''.join(map(str, k)))
def test_segment_identity_with_plain_groups_of_the_same_weights(case, ks):
    from tfnas_amd import _lib, functions as F
    from tfnas_amd.layers import MBInvertedResBlock
    name, N, ic, oc, H, W, s, act, mid = case
    torch.manual_seed(len(name) + sum(ks))
    mix = MBInvertedResBlock(ic, mid, 0, oc, stride=s, act_func=act, mix_kernels=ks).cuda()
    x = torch.randn(N, ic, H, W, generator=torch.Generator().manual_seed(3))
    tiled = F.route_bits(dw='tiled')
    Dm, dm = _forward_D(mix, x, F.route_bits())
    assert dm.flags & _lib.CELL_MIXK and dm.g[0].k == _mix.WORDS[ks]
    c0 = 0
    for c, k, w in zip(_mix.split(mid, len(ks)), ks, mix.depth_conv.conv.segment_weights()):
        plain = MBInvertedResBlock(ic, mid, 0, oc, k, s, act_func=act).cuda()
        with torch.no_grad():
            plain.inverted_bottleneck.conv.weight.copy_(mix.inverted_bottleneck.conv.weight)
            plain.point_linear.conv.weight.copy_(mix.point_linear.conv.weight)
            plain.depth_conv.conv.weight[c0:c0 + c].copy_(w)
        Dp, dp = _forward_D(plain, x, tiled)
        assert not dp.flags & _lib.CELL_MIXK and dp.g[0].k == k and (dp.M, dp.g[0].mcp) == (dm.M, dm.g[0].mcp)
        assert torch.equal(Dm[..., c0:c0 + c], Dp[..., c0:c0 + c]), (k, c0, c)
        assert float(Dm[..., c0:c0 + c].abs().max()) > 0
        c0 += c
    assert c0 == mid


# ------------------------------------------------------------------------------------------------ the bit, the route word
@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_relu_two_column_tiles_res'], _BY_NAME['img_1x1']],
                         ids=lambda c: c[0])
@pytest.mark.parametrize('idxs', [(6,), tuple(range(8))], ids=['sampled', 'soft'])
def test_unmixed_cells_are_bit_identical_with_and_without_the_bit(cfg, idxs):
    """the default cell (kernel sizes 3 3 5 5 3 3 5 5) launched by a caller that sets TFNAS_CELL_MIXK on every descriptor: same
    kernels, same bits -- out, dx, every weight gradient, dwmix"""
    from tfnas_amd import _lib, functions as F

    class WithBit(F.HipModes):
        def apply(self, d, *kind):
            super().apply(d, *kind)
            d.flags |= _lib.CELL_MIXK
    o, m, x, r, e = _inputs(cfg, specs=list(orc.OP_KERNEL))
    assert all(b.mix_kernels is None and b.dilation == 1 for b in m.m_ops)
    base, dbg0, _ = _run(m, x, r, e, idxs, F.HipModes())
    assert not dbg0['d'].flags & _lib.CELL_MIXK
    got, dbg1, _ = _run(m, x, r, e, idxs, WithBit())
    assert dbg1['d'].flags & _lib.CELL_MIXK
    assert list(got) == list(base)
    for k in base:
        assert torch.equal(got[k], base[k]), k


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_relu_two_column_tiles_res']], ids=lambda c: c[0])
@pytest.mark.parametrize('idxs', [(7,), tuple(range(8))], ids=['sampled', 'soft'])
def test_route_word_cannot_move_a_mixconv_cell(cfg, idxs):
    """TFNAS_ROUTE_DW_* and the two weight-gradient route bits: a cell with a packed group runs the tile kernels, its depthwise
    weight gradient in its own launch, whatever the route asks -- every value gives the bits of the default route"""
    from tfnas_amd import functions as F
    o, m, x, r, e = _inputs(cfg)
    base, _, _ = _run(m, x, r, e, idxs, F.HipModes(route=F.route_bits()))
    for kw in (dict(dw='direct'), dict(dw='lds'), dict(dw='tiled'), dict(dwwg=False), dict(dwwg2=False)):
        got, _, _ = _run(m, x, r, e, idxs, F.HipModes(route=F.route_bits(**kw)))
        assert list(got) == list(base)
        for k in base:
            assert torch.equal(got[k], base[k]), (kw, k)


def test_path_level_refuses_a_packed_cell():
    """tfnas_path_plan on a cell that carries the bit with a packed group is TFNAS_EINVAL; the same cell with plain kernel sizes
    under the bit plans as it does without the bit (tfnas_path_create makes streams and events: it needs a device; nothing is
    launched)"""
    from tfnas_amd import _lib
    lib = _lib.lib()
    ctx = C.c_void_p(None)
    assert lib.tfnas_path_create(C.byref(ctx)) == 0
    try:
        beta = C.c_void_p(256)
        for ks, flags, want in (((3, 5, 3, 5, 3, 5, 3, 5), 0, 0), ((3, 5, 3, 5, 3, 5, 3, 5), _lib.CELL_MIXK, 0),
                                ((3, 0x53, 3, 5, 3, 5, 3, 5), _lib.CELL_MIXK, -1), ((3, 5, 3, 5, 3, 5, 3, 0x753), _lib.CELL_MIXK | _lib.CELL_K7, -1)):
            src = _kinds.mixed_desc([('M', 22 + 4 * i, 3, 0) for i in range(8)], 2, 9, 13, 16, 16, flags=flags)
            for g, k in enumerate(ks):
                src.g[g].k = k
            pd = _lib.TfnasPathDesc()
            pd.ncell, pd.nstage, pd.soft, pd.need_dx0 = 1, 1, 1, 1
            pd.stage[0].ncell, pd.stage[0].start_res, pd.stage[0].betas = 1, 0, beta
            C.memmove(C.byref(pd.cell[0]), C.byref(src), C.sizeof(src))
            ws = _lib.TfnasPathWs()
            assert lib.tfnas_path_plan(ctx, C.byref(pd), C.byref(ws)) == want, (ks, flags)
    finally:
        lib.tfnas_path_destroy(ctx)


# ------------------------------------------------------------------------------------------------ expand-free and mixed kinds
NOEXP_CASES = OrderedDict([
    # name: (N, ic, oc, H, W, ks, stride, act, se)
    ('res_k35_swish', (2, 20, 20, 10, 22, (3, 5), 1, 'swish', 0)),           # DS_k35: residual folded into the dx store; 12 | 8
    ('res_k357_swish_se', (2, 28, 28, 7, 9, (3, 5, 7), 1, 'swish', 28)),     # DS_k357_se: 12 | 8 | 8
    ('s2_k35_relu_odd', (2, 20, 24, 9, 13, (3, 5), 2, 'relu', 0)),
    ('s2_k357_swish_se_ragged_cc16', (1, 72, 40, 37, 41, (3, 5, 7), 2, 'swish', 72)),   # 24 | 24 | 24 in the 16-channel regime
    ('res_k357_relu_1x1_q_eq_n', (5, 12, 12, 1, 1, (3, 5, 7), 1, 'relu', 0)),
])


def _noexp_case(name):
    N, ic, oc, H, W, ks, s, act, se = NOEXP_CASES[name]
    o, x, r, w, seed = _mix.case_data([('N', max(ks), se)], (ks,), N, ic, oc, H, W, s, act, base=500)
    return o, x, r


class _MixRawCell(_rawcell.RawCell):
    """_rawcell.RawCell of an expand-free MixConv block whose D and dx buffers are filled with NaN before every launch"""

    def __init__(self, o, x):
        lb = _rawcell._lib()
        super().__init__(o, x, lb.NOEXPAND, _rawcell.param_names(lb.NOEXPAND, o.se_channels))
        self.d.g[0].k = _mix.WORDS[_mix.mix_of(o)]
        self.d.flags |= lb.CELL_MIXK
        lb.check(self.lib.tfnas_cell_plan(C.byref(self.d)), 'tfnas_cell_plan')
        assert self.w[0].dim() == 1 and self.w[0].numel() == _mix.packed_size(o.mid_channels, _mix.mix_of(o))

    def _buf(self, n, guard=0, dtype=torch.float32):
        t = super()._buf(n, guard, dtype)
        if guard:
            t[:int(n)] = float('nan')
        return t


@pytest.mark.parametrize('name', list(NOEXP_CASES))
def test_expand_free_mixconv_cell(name):
    """through the module (sampled launch) and through the raw ABI on NaN-filled, guard-banded buffers"""
    from tfnas_amd import _lib
    o, x, r = _noexp_case(name)
    blk = o.m_ops[0]
    assert blk.inverted_bottleneck is None and _mix.mix_of(blk) == NOEXP_CASES[name][5]
    assert _kinds.kink_distance(o, x) >= _kinds.KINK_TAU
    xo = x.clone().requires_grad_(True)
    yo = blk(xo)
    (yo * r).sum().backward()
    m = _mix.hip_blocks_like(o)[0]
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ym = m(xm)
    (ym * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    d = m._plan.desc(x.shape[0], x.shape[2], x.shape[3])[0]
    assert d.flags & _lib.CELL_NOEXPAND and d.flags & _lib.CELL_MIXK and d.g[0].k == _mix.WORDS[_mix.mix_of(blk)]
    res = OrderedDict(out=hc.err(ym, yo), dx=hc.err(xm.grad, xo.grad))
    for (kk, po), (_, pm) in zip(blk.named_parameters(), m.named_parameters()):
        res['g.' + kk] = hc.err(pm.grad, po.grad)
    mc, ks = blk.mid_channels, _mix.mix_of(blk)
    for s, (a, b) in enumerate(zip(_mix.segments(m.depth_conv.conv.weight.grad, mc, ks),
                                   _mix.segments(blk.depth_conv.conv.weight.grad, mc, ks))):
        res['g.dw.seg%d' % s] = hc.err(a, b)
    assert not hc.worst(res), hc.worst(res)
    cell = _MixRawCell(blk, x)
    out = cell.forward()
    rc, dx, grads = cell.backward(r)
    dd = cell.d
    assert rc == 0 and cell.guard_ok(cell.dx_raw, dd.N * dd.H * dd.W * dd.ic) and cell.guard_ok(cell.D, cell.ws.D)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(cell.D[:cell.ws.D].view(-1, dd.M)[:, :dd.g[0].mc]).all())
    raw = OrderedDict(out=hc.err(out, yo), dx=hc.err(dx, xo.grad))
    for kk, po in blk.named_parameters():
        raw['g.' + kk] = hc.err(grads[kk], po.grad)
    assert not hc.worst(raw), hc.worst(raw)


@pytest.mark.parametrize('name', ['res_k357_swish_se', 's2_k35_relu_odd'])
def test_accumulated_weight_grads_two_backwards_equal_twice_one(name):
    """TFNAS_CELL_ACCUM_WGRAD: the second backward adds its gradients to the first one's -- g + g, bit for bit; dx unchanged"""
    o, x, r = _noexp_case(name)
    cell = _MixRawCell(o.m_ops[0], x)
    cell.forward()
    rc, dx0, g0 = cell.backward(r)
    assert rc == 0
    rc, dx1, g1 = cell.backward(r, accum_into=list(g0.values()))
    assert rc == 0 and torch.equal(dx1, dx0)
    for kk in g0:
        assert torch.equal(g1[kk], g0[kk] + g0[kk]), kk
        assert float(g0[kk].abs().max()) > 0


def test_accumulated_weight_grads_of_a_plain_mixconv_cell():
    """the same through the module path of a plain (expand) MixConv candidate: two raw backwards with the bit equal twice one"""
    from tfnas_amd import _lib, functions as F
    cfg = _BY_NAME['s1_swish_odd_widths_res']
    o, m, x, r, e = _inputs(cfg)

    class Accum(F.HipModes):
        def apply(self, d, *kind):
            super().apply(d, *kind)
            d.flags |= _lib.CELL_ACCUM_WGRAD
    one, _, _ = _run(m, x, r, e, (7,), F.HipModes())
    # (MixedOpFn hands the kernels fresh torch.empty gradients: accumulate into zeros of our own through grad_targets)
    plan = m._plan((7,))
    ps = plan.params()
    tg = [torch.zeros_like(p) for p in ps]
    F.adopt_modes(m, Accum())
    for _ in range(2):
        for p in ps:
            p.requires_grad_(True)
        plan.grad_targets = tg
        try:
            xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
            out = F.MixedOpFn.apply(plan, xm, None, *ps)
            (out * r.cuda()).sum().backward()
            torch.cuda.synchronize()
        finally:
            plan.grad_targets = None
    for i, t in enumerate(tg):
        assert torch.equal(t, one['p%d' % i] + one['p%d' % i]), i


KINDS_CANDS = [('M', 44, 5, 0), ('F', 22, 8), ('N', 7, 8), ('N', 5, 0), ('S',)]
KINDS_MIXES = ((3, 5), None, (3, 5, 7), (3, 5), None)


@pytest.mark.parametrize('act', ['swish', 'relu'])
@pytest.mark.parametrize('need_wgrad', [False, True], ids=['frozen', 'wgrad'])
def test_kinds_cell_with_an_mbi_k35_an_fmb_a_ds_k357_a_ds_k35_and_a_skip(act, need_wgrad):
    """the expand-free MixConv groups are LATER branches of the cell: their dx is accumulated onto the earlier branches'"""
    from tfnas_amd import _lib
    o, x, r, w, seed = _mix.case_data(KINDS_CANDS, KINDS_MIXES, 2, 16, 16, 7, 9, 1, act, base=600)
    plan = _mix.hip_plan(o)
    d = plan.desc(2, 7, 9)[0]
    assert d.flags & _lib.CELL_KINDS and d.flags & _lib.CELL_SKIP and d.flags & _lib.CELL_MIXK and d.flags & _lib.CELL_K7
    assert [d.g[g].k for g in range(5)] == [0x53, 3, 0x753, 0x53, 0]
    ref = _kinds.ref_run(o, x, r, w)
    got = _kinds.hip_run(plan, x, r, w, need_wgrad)
    res = _kinds.compare(ref if need_wgrad else ref[:3] + (None,), got)
    assert not hc.worst(res), hc.worst(res)


# ------------------------------------------------------------------------------------------------ derived form
AFFINE = OrderedDict([
    # name: (ic, mc, se, oc, ks, stride, act, N, H, W, mode)
    ('res_k35_drop', (24, 76, 24, 24, (3, 5), 1, 'swish', 5, 9, 11, 'drop')),
    ('s2_k357_train', (40, 131, 0, 80, (3, 5, 7), 2, 'swish', 2, 13, 9, 'train')),
    ('res_k357_eval', (32, 100, 32, 32, (3, 5, 7), 1, 'swish', 3, 7, 7, 'eval')),
    ('res_k35_eval', (32, 100, 32, 32, (3, 5), 1, 'swish', 3, 7, 7, 'eval')),
    ('noexp_s2_k35_relu_train', (20, 20, 8, 24, (3, 5), 2, 'relu', 2, 9, 13, 'train')),
    ('noexp_res_k357_drop', (28, 28, 16, 28, (3, 5, 7), 1, 'swish', 5, 7, 9, 'drop')),
])


def _affine_case(name):
    ic, mc, se, oc, ks, s, act, N, H, W, mode = AFFINE[name]
    for seed in range(64):
        gen = torch.Generator().manual_seed(1900 + seed)
        torch.manual_seed(1900 + seed)
        o = _mix.mix_block(orc.DerivedBlock, ic, mc, se, oc, ks, s, act)
        ar.randomise(o, gen)
        _mix.randomise_packed(o, gen)
        x, r = ar.inputs(gen, N, ic, H, W, (N, oc, (H - 1) // s + 1, (W - 1) // s + 1))
        u = ar.drop_u(mode, N)
        if not ar.conditioned(o):
            continue
        ref = ar.run_block(copy.deepcopy(o).double(), x.double(), r.double(), mode, None if u is None else u.double())
        if ar.kink_clear(ref['_taps'], act, 2 if mc > ic else 1):
            return o, x, r, u, mode, ref
    raise AssertionError('no qualifying seed for %s' % name)


@pytest.mark.parametrize('name', list(AFFINE))
def test_affine_mixconv_block_matches_float64_restatement(name):
    """tfnas_mbconv_fwd/bwd through layers.MBInvertedResBlock(affine=True, mix_kernels=...): y, dx, every conv / SE / BatchNorm
    gradient within 2e-5 + 1e-4 max|ref|, every running buffer within 1e-6 + 1e-5 |ref|, of the float64 restatement; training
    mode with drop-connect (images kept and dropped) and eval mode (running buffers untouched)"""
    from tfnas_amd.layers import MBInvertedResBlock
    ic, mc, se, oc, ks, s, act = AFFINE[name][:7]
    o, x, r, u, mode, ref = _affine_case(name)
    m = MBInvertedResBlock(ic, mc, se, oc, max(ks), s, affine=True, act_func=act, mix_kernels=ks)
    m.load_state_dict(o.state_dict())
    for bn in m.bn_modules():
        bn.momentum = ar.MOMENTUM
    m = m.cuda()
    m.train(mode != 'eval')
    if u is not None:
        m.drop_connect_rate, m.drop_u = 1.0 - ar.KEEP, u
        assert {bool(v) for v in torch.floor(ar.KEEP + u)} == {True, False}
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = m(xm)
    (y * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = OrderedDict(y=y.detach(), dx=xm.grad)
    for kk, p in m.named_parameters():
        got['g.' + kk] = p.grad
    for kk, b in m.named_buffers():
        if 'running' in kk:
            got['b.' + kk] = b.detach().clone()
    assert set(got) == {kk for kk in ref if not kk.startswith('_')}
    ratios = ar.compare(got, ref)
    print('MIX_AFFINE %-26s %s' % (name, '  '.join('%s %.4f' % kv for kv in ar.classes(ratios).items())))
    bad = {kk: v for kk, v in ratios.items() if not v <= 1.0}
    assert not bad, bad
    if mode == 'eval':
        for kk, b in o.named_buffers():
            if 'running' in kk:
                assert torch.equal(got['b.' + kk].cpu(), b), kk


def test_networkcfg_with_mixconv_stage4_and_stage5_blocks_matches_the_derived_restatement():
    """model_eval.NetworkCfg from a config whose stage-4 and stage-5 blocks are MixConv blocks against oracle.DerivedNetwork with
    the same blocks rebuilt by _mix.mix_network, at 2 x 3 x 64 x 64: eval-mode and train-mode logits within the tolerance of
    tests/test_gpu_derived.py (1e-3 + 1e-3 |ref|)"""
    from tfnas_amd import model_eval as me
    cfg = _mix.mix_network_config(20)
    arch = {st: {'block%d' % (i + 1): (j * 3 + i) % 8 for i in range(2)} for j, st in enumerate(orc.STAGE_CFG)}
    arch['stage6'] = {'block1': 7}
    torch.manual_seed(5)
    o = _mix.mix_network(orc.DerivedNetwork(20, arch, orc.initial_mc_num_dddict()))
    gen = torch.Generator().manual_seed(6)
    ar.randomise(o, gen)
    _mix.randomise_packed(o, gen)
    with torch.no_grad():
        o.classifier.linear.weight.copy_(torch.randn(o.classifier.linear.weight.shape, generator=gen) * 0.05)
    m = me.NetworkCfg(20, cfg)
    assert [b.mix_kernels for b in m.stage4] == list(_mix.MIX_STAGES['stage4'])
    m.load_state_dict(o.state_dict())
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = ar.MOMENTUM
    m = m.cuda()
    x = torch.randn(2, 3, 64, 64, generator=gen)
    for mode in ('eval', 'train'):
        o.train(mode == 'train'); m.train(mode == 'train')
        with torch.no_grad():
            yo = o(x)
            ym = m(x.cuda()).cpu()
        # (the gate tests/test_gpu_derived.py holds whole-network logits to)
        assert torch.allclose(ym, yo, atol=1e-3, rtol=1e-3), (mode, float((ym - yo).abs().max()))


def test_latency_measurement_of_a_mixconv_block():
    import math
    from tfnas_amd import lut_builder
    t = lut_builder.Measurer(torch.device('cuda:0'))
    for mode in ('inference', 'search'):
        ms = t.measure(24, 72, 0, 24, 5, 1, 'relu', 28, batch=4, iters=2, reps=1, mode=mode, mix_kernels=(3, 5))
        assert math.isfinite(ms) and ms > 0
