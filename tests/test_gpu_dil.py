"""GPU parity of dilated depthwise candidates (TfnasGroup.dil = 2 under TFNAS_CELL_DILATION: the LDS tile kernels with their taps
two pixels apart): cells with dilated candidates (sampled launches with weight gradients, soft launches that mix k3, k5, k7,
dilated k3 and dilated k5), expand-free dilated cells, a cell of several kinds, the derived-network block and a derived network,
against the CPU restatement of tests/_dil.py (pinned to the reference in tests/test_dil_oracle_pin.py).

Cells of plain candidates: every stage is compared with _hipcheck.check_cell at its default gate (abs err <= 2e-5 + 1e-4 *
max|ref| per tensor), ReLU decisions replayed, no kink exemption (a cell with a dilated group never takes the E-free route).
Expand-free and mixed-kind cells: the same gate on out, dx, dwmix and every gradient, with seeds whose float64 pre-activations
stay 1e-4 from every kink (chosen from the restatement alone, nothing exempted).  Shapes: those of tests/test_gpu_k7.py moved to
the effective extents 5 and 9 -- a 1 x 1 image, an image smaller than both extents, one equal to the larger, odd and even sizes
at stride 2, two column tiles (the 4-pixel halo of the dilated 5 x 5 crosses the 16-column tile), ragged tiles in the 16-channel
regime of the stride-2 forward, widths that are no multiple of 4.  The affine block is held to the gate of
tests/test_gpu_affine_f64.py against a float64 run of the restatement."""
import copy
import ctypes as C
from collections import OrderedDict

import pytest
import torch

import _affineref as ar
import _dil
import _hipcheck as hc
import _kinds
import _rawcell
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [
    # name, N, ic, oc, H, W, stride, act, mids
    ('img_1x1', 5, 16, 16, 1, 1, 1, 'swish', [20, 33, 24, 40, 17, 35, 28, 44]),
    ('img_smaller_than_both_extents_res', 2, 16, 16, 3, 5, 1, 'swish', [20, 33, 24, 40, 17, 35, 28, 44]),
    ('img_equals_larger_extent', 3, 32, 48, 9, 9, 1, 'swish', [41, 72, 36, 67, 45, 80, 53, 70]),
    ('s2_swish_odd', 2, 24, 40, 9, 13, 2, 'swish', [36, 72, 40, 60, 33, 66, 44, 71]),
    ('s2_relu_even', 2, 16, 24, 12, 10, 2, 'relu', [24, 40, 20, 36, 29, 44, 24, 50]),
    ('s1_relu_two_column_tiles_res', 2, 24, 24, 10, 22, 1, 'relu', [32, 52, 28, 56, 37, 60, 40, 62]),
    ('s2_relu_ragged_tiles_cc16', 1, 16, 24, 37, 41, 2, 'relu', [48, 96] * 4),
    ('s1_swish_odd_widths_res', 3, 40, 40, 8, 6, 1, 'swish', [53, 107, 44, 88, 61, 96, 48, 79]),
]
_BY_NAME = {c[0]: c for c in SHAPES}
_IDS = [c[0] for c in SHAPES]


def _inputs(cfg, kds=_dil.SOFT):
    name, N, ic, oc, H, W, s, act, mids = cfg
    o, m = _dil.make_cell_pair(ic, oc, s, act, mids, kds=kds, seed=len(name))
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, ic, H, W, generator=g)
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=g)
    e = torch.empty(8).exponential_(generator=g)
    return o, m, x, r, e


def _is(op, k, d):
    return op.kernel_size == k and _dil.dilation_of(op) == d


@pytest.mark.parametrize('cfg', SHAPES, ids=_IDS)
@pytest.mark.parametrize('idx', [7, 5], ids=['k5d2_se', 'k3d2_se'])
def test_sampled_dilated_candidate_with_weight_grads(cfg, idx):
    """one dilated candidate with squeeze-excite (G = 1), weight gradients wanted"""
    o, m, x, r, e = _inputs(cfg)
    k, d = _dil.SOFT[idx]
    assert d == 2 and _is(o.m_ops[idx], k, d) and _is(m.m_ops[idx], k, d) and o.m_ops[idx].se_channels
    res = hc.check_cell(o, m, x, r, e, [idx], need_wgrad=True)
    assert 'g%d.grad_dw' % idx in res and 'g%d.dEh' % idx in res and 'kink_fraction' not in res


@pytest.mark.parametrize('cfg', [_BY_NAME[n] for n in ('img_smaller_than_both_extents_res', 's2_swish_odd', 's2_relu_ragged_tiles_cc16',
                                                       's1_relu_two_column_tiles_res')], ids=lambda c: c[0])
@pytest.mark.parametrize('idx', [3, 1], ids=['k5d2', 'k3d2'])
def test_sampled_dilated_candidate_without_se(cfg, idx):
    o, m, x, r, e = _inputs(cfg)
    assert _is(o.m_ops[idx], *_dil.SOFT[idx]) and _dil.SOFT[idx][1] == 2 and not o.m_ops[idx].se_channels
    res = hc.check_cell(o, m, x, r, e, [idx], need_wgrad=True)
    assert 'kink_fraction' not in res


@pytest.mark.parametrize('cfg', SHAPES, ids=_IDS)
def test_soft_mode_mixing_k3_k5_k7_and_both_dilated_pairs(cfg):
    o, m, x, r, e = _inputs(cfg)
    assert [(op.kernel_size, op.dilation) for op in m.m_ops] == list(_dil.SOFT)
    assert {(3, 1), (5, 1), (7, 1), (3, 2), (5, 2)} == set(_dil.SOFT)
    res = hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=False)
    assert any(k.endswith('.dEh') for k in res) and 'kink_fraction' not in res      # materialised route, nothing exempted


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_relu_two_column_tiles_res']], ids=lambda c: c[0])
def test_soft_mode_weight_grads_share_one_partial_row_matrix(cfg):
    """all eight candidates' depthwise weight gradients from one pass: the five launches fill the same partial rows"""
    o, m, x, r, e = _inputs(cfg)
    res = hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=True)
    assert all('g%d.grad_dw' % i in res for i in range(8)) and 'kink_fraction' not in res


def _run(m, x, r, e, idxs, modes):
    from tfnas_amd import functions as F
    from tfnas_amd.functions import MixedOpFn
    F.adopt_modes(m, modes)
    plan = m._plan(tuple(idxs))
    ps = plan.params()
    for p in ps:
        p.requires_grad_(True)
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = torch.softmax(-e.log(), 0).cuda().requires_grad_(True) if len(idxs) > 1 else None
    MixedOpFn.debug_sink = []
    try:
        out = MixedOpFn.apply(plan, xm, w, *ps)
        (out * r.cuda()).sum().backward()
        torch.cuda.synchronize()
        dbg = MixedOpFn.debug_sink[0]
    finally:
        MixedOpFn.debug_sink = None
    got = [out.detach().clone(), xm.grad.clone()] + [p.grad.clone() for p in ps] + ([w.grad.clone()] if w is not None else [])
    for p in ps:
        p.grad = None
    return got, dbg


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_relu_two_column_tiles_res']], ids=lambda c: c[0])
@pytest.mark.parametrize('idxs', [(7,), tuple(range(8))], ids=['sampled', 'soft'])
def test_route_word_cannot_move_a_dilated_cell(cfg, idxs):
    """TFNAS_ROUTE_DW_* and the two weight-gradient route bits: a cell with a dilated group runs the tile kernels, its depthwise
    weight gradient in its own launch, whatever the route asks -- every value gives the bits of the default route (on these
    shapes an undilated cell takes the register-window kernels at stride 2 and the ring kernels at 22 columns)"""
    from tfnas_amd import functions as F
    o, m, x, r, e = _inputs(cfg)
    base, _ = _run(m, x, r, e, idxs, F.HipModes(route=F.route_bits()))
    for kw in (dict(dw='direct'), dict(dw='lds'), dict(dw='tiled'), dict(dwwg=False), dict(dwwg2=False)):
        got, _ = _run(m, x, r, e, idxs, F.HipModes(route=F.route_bits(**kw)))
        assert len(got) == len(base)
        for i, (a, b) in enumerate(zip(got, base)):
            assert torch.equal(a, b), (kw, i)


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_relu_two_column_tiles_res'], _BY_NAME['img_1x1']],
                         ids=lambda c: c[0])
@pytest.mark.parametrize('idxs', [(6,), tuple(range(8))], ids=['sampled', 'soft'])
def test_undilated_cells_are_bit_identical_with_and_without_the_bit(cfg, idxs):
    """the default cell (kernel sizes 3 3 5 5 3 3 5 5, every dil word 0) launched by a caller that sets TFNAS_CELL_DILATION on
    every descriptor: same kernels, same bits -- out, dx, every weight gradient, dwmix"""
    from tfnas_amd import _lib, functions as F

    class WithBit(F.HipModes):
        def apply(self, d, *kind):
            super().apply(d, *kind)
            d.flags |= _lib.CELL_DILATION
    o, m, x, r, e = _inputs(cfg, kds=[(k, 1) for k in orc.OP_KERNEL])
    assert all(b.dilation == 1 for b in m.m_ops)
    base, dbg0 = _run(m, x, r, e, idxs, F.HipModes())
    assert not dbg0['d'].flags & _lib.CELL_DILATION
    got, dbg1 = _run(m, x, r, e, idxs, WithBit())
    assert dbg1['d'].flags & _lib.CELL_DILATION
    for i, (a, b) in enumerate(zip(got, base)):
        assert torch.equal(a, b), i


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s2_relu_even'], _BY_NAME['s2_relu_ragged_tiles_cc16']],
                         ids=lambda c: c[0])
def test_stride2_odd_pixels_of_dEh_are_exactly_zero(cfg):
    """stride 2 with dilation 2: every tap lands on an even input row and column, so the odd pixels of a dilated group's dEh are
    exactly 0.0 -- and stored (the buffer is torch.empty: whatever it held is gone); an undilated group's are not zero"""
    from tfnas_amd import functions as F
    o, m, x, r, e = _inputs(cfg)
    _, dbg = _run(m, x, r, e, tuple(range(8)), F.HipModes())
    d = dbg['d']
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    dEh = dbg['dEh'][:N * H * W * d.M].view(N, H, W, d.M)
    assert bool(torch.isfinite(dEh[..., :d.g[7].off + d.g[7].mc]).all())
    for g, (k, dil) in enumerate(_dil.SOFT):
        mine = dEh[..., d.g[g].off:d.g[g].off + d.g[g].mc]
        odd = torch.cat([mine[:, 1::2].reshape(-1), mine[:, :, 1::2].reshape(-1)])
        if dil == 2:
            assert odd.numel() > 0 and bool((odd == 0.0).all()), g
            assert float(mine[:, 0::2, 0::2].abs().max()) > 0
        else:
            assert float(odd.abs().max()) > 0, g


# ------------------------------------------------------------------------------------------------ expand-free and mixed kinds
NOEXP_CASES = OrderedDict([
    # name: (N, ic, oc, H, W, k, stride, act, se)
    ('res_k5d2_swish_se', (2, 16, 16, 10, 22, 5, 1, 'swish', 8)),           # residual folded into the dx store; two column tiles
    ('res_k3d2_relu_1x1', (5, 16, 16, 1, 1, 3, 1, 'relu', 0)),
    ('s2_k5d2_relu_se_odd', (2, 20, 24, 9, 13, 5, 2, 'relu', 8)),           # one ragged channel chunk
    ('s2_k3d2_swish_even', (3, 16, 24, 12, 10, 3, 2, 'swish', 0)),
    ('s2_k5d2_swish_ragged_cc16', (1, 72, 40, 37, 41, 5, 2, 'swish', 0)),   # 72 = 4 x 16 + 8 channels in the 16-channel regime
])


def _noexp_case(name):
    N, ic, oc, H, W, k, s, act, se = NOEXP_CASES[name]
    o, x, r, w, seed = _dil.case_data([('N', k, se)], (2,), N, ic, oc, H, W, s, act, base=500)
    return o, x, r


@pytest.mark.parametrize('name', list(NOEXP_CASES))
def test_sampled_expand_free_dilated_cell(name):
    o, x, r = _noexp_case(name)
    blk = o.m_ops[0]
    assert blk.inverted_bottleneck is None and _dil.dilation_of(blk) == 2
    assert _kinds.kink_distance(o, x) >= _kinds.KINK_TAU
    xo = x.clone().requires_grad_(True)
    yo = blk(xo)
    (yo * r).sum().backward()
    m = _dil.hip_blocks_like(o)[0]
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ym = m(xm)
    (ym * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    d = m._plan.desc(x.shape[0], x.shape[2], x.shape[3])[0]
    from tfnas_amd import _lib
    assert d.flags & _lib.CELL_NOEXPAND and d.flags & _lib.CELL_DILATION and d.g[0].dil == 2
    res = OrderedDict(out=hc.err(ym, yo), dx=hc.err(xm.grad, xo.grad))
    for (kk, po), (_, pm) in zip(blk.named_parameters(), m.named_parameters()):
        res['g.' + kk] = hc.err(pm.grad, po.grad)
    assert not hc.worst(res), hc.worst(res)


class _NanRawCell(_rawcell.RawCell):
    """_rawcell.RawCell of an expand-free dilated block whose D and dx buffers are filled with NaN before every launch"""

    def __init__(self, o, x):
        lb = _rawcell._lib()
        super().__init__(o, x, lb.NOEXPAND, _rawcell.param_names(lb.NOEXPAND, o.se_channels))
        self.d.g[0].dil = _dil.dilation_of(o)
        self.d.flags |= lb.CELL_DILATION
        lb.check(self.lib.tfnas_cell_plan(C.byref(self.d)), 'tfnas_cell_plan')

    def _buf(self, n, guard=0, dtype=torch.float32):
        t = super()._buf(n, guard, dtype)
        if guard:
            t[:int(n)] = float('nan')
        return t


@pytest.mark.parametrize('name', ['s2_k5d2_relu_se_odd', 's2_k3d2_swish_even', 's2_k5d2_swish_ragged_cc16'])
def test_stride2_odd_pixels_of_expand_free_dx_are_stored_as_zero(name):
    """the dx of an expand-free dilated group at stride 2, in a buffer filled with NaN before the launch: the odd rows and
    columns are exactly 0.0, nothing is left NaN, the guard band behind dx is untouched -- and the numbers are the restatement's"""
    o, x, r = _noexp_case(name)
    blk = o.m_ops[0]
    xo = x.clone().requires_grad_(True)
    (blk(xo) * r).sum().backward()
    cell = _NanRawCell(blk, x)
    cell.forward()
    rc, dx, grads = cell.backward(r)
    d = cell.d
    assert rc == 0 and cell.guard_ok(cell.dx_raw, d.N * d.H * d.W * d.ic)
    assert bool(torch.isfinite(dx).all())
    assert bool((dx[:, :, 1::2] == 0.0).all()) and bool((dx[:, :, :, 1::2] == 0.0).all())
    assert float(dx[:, :, 0::2, 0::2].abs().max()) > 0
    res = OrderedDict(dx=hc.err(dx, xo.grad))
    for kk, po in blk.named_parameters():
        res['g.' + kk] = hc.err(grads[kk], po.grad)
    assert not hc.worst(res), hc.worst(res)


@pytest.mark.parametrize('name', ['res_k5d2_swish_se', 's2_k5d2_relu_se_odd'])
def test_accumulated_weight_grads_two_backwards_equal_twice_one(name):
    """TFNAS_CELL_ACCUM_WGRAD: the second backward adds its gradients to the first one's -- g + g, bit for bit; dx unchanged"""
    o, x, r = _noexp_case(name)
    cell = _NanRawCell(o.m_ops[0], x)
    cell.forward()
    rc, dx0, g0 = cell.backward(r)
    assert rc == 0
    rc, dx1, g1 = cell.backward(r, accum_into=list(g0.values()))
    assert rc == 0 and torch.equal(dx1, dx0)
    for kk in g0:
        assert torch.equal(g1[kk], g0[kk] + g0[kk]), kk
        assert float(g0[kk].abs().max()) > 0


KINDS_CANDS = [('N', 3, 0), ('M', 22, 5, 8), ('F', 22, 8), ('M', 30, 3, 0), ('S',)]
KINDS_DILS = (2, 2, 1, 1, 1)


@pytest.mark.parametrize('act', ['swish', 'relu'])
@pytest.mark.parametrize('need_wgrad', [False, True], ids=['frozen', 'wgrad'])
def test_kinds_cell_with_a_dilated_ds_a_dilated_mbi_an_fmb_and_a_skip(act, need_wgrad):
    from tfnas_amd import _lib
    o, x, r, w, seed = _dil.case_data(KINDS_CANDS, KINDS_DILS, 2, 8, 8, 7, 9, 1, act, base=600)
    plan = _dil.hip_plan(o)
    d = plan.desc(2, 7, 9)[0]
    assert d.flags & _lib.CELL_KINDS and d.flags & _lib.CELL_SKIP and d.flags & _lib.CELL_DILATION
    assert [d.g[g].dil for g in range(5)] == [2, 2, 0, 0, 0]
    ref = _kinds.ref_run(o, x, r, w)
    got = _kinds.hip_run(plan, x, r, w, need_wgrad)
    res = _kinds.compare(ref if need_wgrad else ref[:3] + (None,), got)
    assert not hc.worst(res), hc.worst(res)


# ------------------------------------------------------------------------------------------------ derived form
AFFINE = OrderedDict([
    # name: (ic, mc, se, oc, k, dil, stride, act, N, H, W, mode)
    ('res_k5d2_drop', (24, 72, 24, 24, 5, 2, 1, 'swish', 5, 9, 11, 'drop')),
    ('s2_k3d2_train', (40, 131, 0, 80, 3, 2, 2, 'swish', 2, 13, 9, 'train')),
    ('res_k3d2_eval', (32, 96, 32, 32, 3, 2, 1, 'swish', 3, 7, 7, 'eval')),
    ('noexp_s2_k5d2_relu_train', (16, 16, 8, 24, 5, 2, 2, 'relu', 2, 9, 13, 'train')),
    ('noexp_res_k3d2_drop', (16, 16, 16, 16, 3, 2, 1, 'swish', 5, 7, 9, 'drop')),
])


def _affine_case(name):
    ic, mc, se, oc, k, dil, s, act, N, H, W, mode = AFFINE[name]
    for seed in range(64):
        gen = torch.Generator().manual_seed(900 + seed)
        o = orc.DerivedBlock(ic, mc, se, oc, k, s, act)
        ar.randomise(o, gen)
        _dil.dilate(o, dil)
        x, r = ar.inputs(gen, N, ic, H, W, (N, oc, (H - 1) // s + 1, (W - 1) // s + 1))
        u = ar.drop_u(mode, N)
        if not ar.conditioned(o):
            continue
        ref = ar.run_block(copy.deepcopy(o).double(), x.double(), r.double(), mode, None if u is None else u.double())
        if ar.kink_clear(ref['_taps'], act, 2 if mc > ic else 1):
            return o, x, r, u, mode, ref
    raise AssertionError('no qualifying seed for %s' % name)


@pytest.mark.parametrize('name', list(AFFINE))
def test_affine_dilated_block_matches_float64_restatement(name):
    """tfnas_mbconv_fwd/bwd through layers.MBInvertedResBlock(affine=True, dilation=2): y, dx, every conv / SE / BatchNorm
    gradient within 2e-5 + 1e-4 max|ref|, every running buffer within 1e-6 + 1e-5 |ref|, of the float64 restatement; training
    mode with drop-connect (images kept and dropped) and eval mode (running buffers untouched)"""
    from tfnas_amd.layers import MBInvertedResBlock
    ic, mc, se, oc, k, dil, s, act = AFFINE[name][:8]
    o, x, r, u, mode, ref = _affine_case(name)
    m = MBInvertedResBlock(ic, mc, se, oc, k, s, affine=True, act_func=act, dilation=dil)
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
    print('DIL_AFFINE %-26s %s' % (name, '  '.join('%s %.4f' % kv for kv in ar.classes(ratios).items())))
    bad = {kk: v for kk, v in ratios.items() if not v <= 1.0}
    assert not bad, bad
    if mode == 'eval':
        for kk, b in o.named_buffers():
            if 'running' in kk:
                assert torch.equal(got['b.' + kk].cpu(), b), kk


def test_networkcfg_with_dilated_stage5_blocks_matches_the_derived_restatement():
    """model_eval.NetworkCfg from a config whose two stage-5 blocks are dilated (a dilated 5 x 5 at stride 2, a dilated 3 x 3
    residual) against oracle.DerivedNetwork with the same blocks dilated, at 2 x 3 x 64 x 64: eval-mode logits and train-mode
    logits within the tolerance of tests/test_gpu_derived.py (1e-3 + 1e-3 |ref|); the undilated network of the same weights is
    far outside it"""
    from tfnas_amd import model_eval as me
    cfg = _dil.dil_network_config(20)
    arch = {st: {'block%d' % (i + 1): (j * 3 + i) % 8 for i in range(2)} for j, st in enumerate(orc.STAGE_CFG)}
    arch['stage6'] = {'block1': 7}
    torch.manual_seed(5)
    o = _dil.dilate_network(orc.DerivedNetwork(20, arch, orc.initial_mc_num_dddict()))
    gen = torch.Generator().manual_seed(6)
    ar.randomise(o, gen)
    with torch.no_grad():
        o.classifier.linear.weight.copy_(torch.randn(o.classifier.linear.weight.shape, generator=gen) * 0.05)
    m = me.NetworkCfg(20, cfg)
    m.load_state_dict(o.state_dict())
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = ar.MOMENTUM
    m = m.cuda()
    x = torch.randn(2, 3, 64, 64, generator=gen)
    plain = copy.deepcopy(o)
    for b in plain.stage5:
        _dil.dilate(b, 1)
    for mode in ('eval', 'train'):
        o.train(mode == 'train'); m.train(mode == 'train'); plain.train(mode == 'train')
        with torch.no_grad():
            yo, yp = o(x), plain(x)
            ym = m(x.cuda()).cpu()
        # (the gate tests/test_gpu_derived.py holds whole-network logits to)
        assert torch.allclose(ym, yo, atol=1e-3, rtol=1e-3), (mode, float((ym - yo).abs().max()))
        if mode == 'train':                       # (batch statistics over 2 x 2 x 2 stage-5 pixels: the dilation shows in the logits)
            assert float((yp - yo).abs().max()) > 20 * (1e-3 + 1e-3 * float(yo.abs().max()))


def test_latency_measurement_of_a_dilated_block():
    import math
    from tfnas_amd import lut_builder
    t = lut_builder.Measurer(torch.device('cuda:0'))
    for mode in ('inference', 'search'):
        ms = t.measure(24, 72, 0, 24, 5, 1, 'relu', 28, batch=4, iters=2, reps=1, mode=mode, dilation=2)
        assert math.isfinite(ms) and ms > 0
