"""MBConv blocks WITHOUT an expand convolution (mid_channels <= in_channels: TFNAS_CELL_NOEXPAND, the raw-input form of the LDS
tile depthwise kernels) on the HIP path, search form: ``layers.MBInvertedResBlock(affine=False)`` against ``oracle.MBConv``
(pinned to the reference in tests/test_noexp_oracle_pin.py), stage by stage through the oracle's ``detail`` dict (D, pooled,
gate, P, out), dx and every weight gradient, at the tolerance of _hipcheck.check_cell (abs err <= 2e-5 + 1e-4 max|ref| per tensor).

Shapes are the smallest at which each thing can break (the table below says which).  Kinks: no element is exempted -- every
case's seed was picked so that, in a float64 run of the oracle, no BN2 output and no SE hidden pre-activation lies within 1e-4
of a kink of the activation (0; 6; -3, 3), which the test asserts before it compares: two fp32 implementations then take the same
side everywhere.  The raw-ABI tests add what the modules do not expose: the route word cannot move the cell, accumulation is
g + v bit for bit, dx == NULL with frozen weights returns 0 with nothing to produce, and the floats behind D and dx stay
untouched."""
import ctypes as C

import pytest
import torch

import _acts
import _hipcheck as hc
import _noexp

pytestmark = pytest.mark.gpu

# id: (N, ic, oc, H, W, k, stride, act, se, seed)
CASES = {
    'px1_res_swish':        (5, 16, 16, 1, 1, 3, 1, 'swish', 0, 0),       # 1 x 1 image; residual folded into the dx store
    'img3x5_k5_relu_se':    (2, 16, 24, 3, 5, 5, 1, 'relu', 8, 0),   # image smaller than the kernel; ic != oc at stride 1
    'img3x5_k7_hswish_res': (2, 16, 16, 3, 5, 7, 1, 'h-swish', 0, 0),
    's2_odd_ic20_relu6_se': (2, 20, 24, 9, 13, 3, 2, 'relu6', 8, 0),  # stride 2, odd extent; one ragged channel chunk
    's2_even_k5_swish':     (3, 16, 24, 12, 10, 5, 2, 'swish', 0, 0),     # stride 2, even extent
    'two_col_tiles_res_se': (2, 16, 16, 10, 22, 3, 1, 'relu', 8, 15),  # two column tiles, several workgroups, residual + SE
    'ic72_k5_res_swish':    (2, 72, 72, 7, 9, 5, 1, 'swish', 0, 0),       # 72 = 32 + 32 + 8 channels
    'ic72_s2_k7_relu_se':   (2, 72, 40, 9, 13, 7, 2, 'relu', 8, 5),
    'second_stem':          (2, 32, 16, 12, 12, 3, 1, 'relu', 8, 5),  # the reference's second_stem (32, 32, 8, 16, k3, s1, relu)
}


def _case(name):
    N, ic, oc, H, W, k, s, act, se, seed = CASES[name]
    o = _noexp.oracle_block(ic, se, oc, k, s, act, 100 + seed)
    gen = torch.Generator().manual_seed(7000 + seed)
    x = torch.randn(N, ic, H, W, generator=gen)
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=gen)
    return o, x, r


def _oracle_run(o, x, r):
    xo = x.clone().requires_grad_(True)
    det = {}
    out = o(xo, det)
    (out * r).sum().backward()
    return out, det, xo.grad


@pytest.mark.parametrize('name', list(CASES))
def test_block_without_expand_matches_oracle(name):
    from tfnas_amd.functions import MixedOpFn
    N, ic, oc, H, W, k, s, act, se, _ = CASES[name]
    with _acts.wrapped_oracle():
        o, x, r = _case(name)
        assert o.inverted_bottleneck is None
        assert _noexp.kink_distance(o, x) > _noexp.KINK_TAU          # the seed keeps every pre-activation clear of the kinks
        out_o, det, dx_o = _oracle_run(o, x, r)
    m = _noexp.hip_block_like(o)
    assert m.inverted_bottleneck is None and len(m.hip_params()) == (6 if se else 2)
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    MixedOpFn.debug_sink, MixedOpFn.fwd_sink = [], []
    try:
        out_m = m(xm)                                                # (a RuntimeError before this feature)
        saved = out_m.grad_fn.saved_tensors                          # xh, wmix, E, D, Pr, fsmall, stats, *params
        (out_m * r.cuda()).sum().backward()
        torch.cuda.synchronize()
        frec = MixedOpFn.fwd_sink[0]
    finally:
        MixedOpFn.debug_sink = MixedOpFn.fwd_sink = None
    d, ws = frec['d'], frec['ws']
    assert saved[2] is None and ws.E == 0 and frec['E'] is None     # E is neither allocated nor saved
    M, Ho, Wo = d.M, d.Ho, d.Wo
    res = {}
    D = saved[3][:N * Ho * Wo * M].view(N, Ho, Wo, M)
    res['D'] = hc.err(D[..., :ic], hc.nhwc(det['D']))
    if se:
        fs = saved[5]
        res['pooled'] = hc.err(fs[ws.off_pooled:ws.off_pooled + N * M].view(N, M)[:, :ic], det['pooled'].flatten(1))
        res['gate'] = hc.err(fs[ws.off_gate:ws.off_gate + N * M].view(N, M)[:, :ic], det['gate'].flatten(1))
    res['P'] = hc.err(saved[4].view(N, Ho, Wo, oc), hc.nhwc(det['P']))
    res['out'] = hc.err(out_m, out_o)
    res['dx'] = hc.err(xm.grad, dx_o)
    names = ['dw', 'proj'] + (['se_rw', 'se_rb', 'se_ew', 'se_eb'] if se else [])
    op = o.params()
    for nme, p in zip(names, m.hip_params()):
        res['grad_' + nme] = hc.err(p.grad, op[nme].grad)
    bad = hc.worst(res)
    assert not bad, bad


def _raw(name):
    with _acts.wrapped_oracle():
        o, x, r = _case(name)
        out_o, det, dx_o = _oracle_run(o, x, r)
    return o, x, r, out_o, dx_o, _noexp.raw_cell(o, x)


@pytest.mark.parametrize('name', ['two_col_tiles_res_se', 's2_odd_ic20_relu6_se'])
def test_raw_abi_route_word_accumulation_and_guard_bands(name):
    from tfnas_amd import _lib
    o, x, r, out_o, dx_o, cell = _raw(name)
    d, ws = cell.d, cell.ws
    P = d.N * d.H * d.W
    Po = d.N * d.Ho * d.Wo

    def written_D():           # (the pad columns [ic, M) of a row are never read or written)
        return cell.D[:Po * d.M].view(Po, d.M)[:, :d.ic].clone()
    out0 = cell.forward().clone()
    D0 = written_D()
    assert cell.guard_ok(cell.D, ws.D)
    rc, dx0, g0 = cell.backward(r)
    assert rc == 0 and cell.guard_ok(cell.dx_raw, P * d.ic)
    res = {'out': hc.err(out0, out_o), 'dx': hc.err(dx0, dx_o)}
    op = dict(o.named_parameters())
    for nme, g in g0.items():
        res['grad_' + nme] = hc.err(g, op[nme].grad)
    assert not hc.worst(res), hc.worst(res)
    # the route word cannot move the cell: register-window, ring and tile requests (and the expand-side bits) are one launch plan
    for route in (1 << 6, 2 << 6, 3 << 6, (1 << 6) | _lib.ROUTE_XG_ALL | _lib.ROUTE_GRAM2 | _lib.ROUTE_DWWG_OFF | _lib.ROUTE_DWWG2_OFF):
        assert torch.equal(cell.forward(route), out0) and torch.equal(written_D(), D0) and cell.guard_ok(cell.D, ws.D)
        rc, dx1, g1 = cell.backward(r, route)
        assert rc == 0 and torch.equal(dx1, dx0) and all(torch.equal(a, b) for a, b in zip(g1.values(), g0.values()))
    cell.forward()
    # TFNAS_CELL_ACCUM_WGRAD: g + v bit for bit; dx unchanged
    gen = torch.Generator().manual_seed(5)
    have = [torch.randn(g.shape, generator=gen).cuda() for g in g0.values()]
    rc, dx2, g2 = cell.backward(r, accum_into=have)
    assert rc == 0 and torch.equal(dx2, dx0)
    for h, v, got in zip(have, g0.values(), g2.values()):
        assert torch.equal(got, h + v)
    # weight gradients on the caller's stream: the same numbers
    rc, dx3, g3 = cell.backward(r, _lib.ROUTE_WGRAD_INLINE)
    assert rc == 0 and torch.equal(dx3, dx0) and all(torch.equal(a, b) for a, b in zip(g3.values(), g0.values()))
    # frozen weights: dx alone, and nothing at all when dx is not wanted either
    rc, dx4, _ = cell.backward(r, need_wgrad=False)
    assert rc == 0 and torch.equal(dx4, dx0)
    rc, dx5, _ = cell.backward(r, need_wgrad=False, want_dx=False)
    assert rc == 0 and dx5 is None
    # weight gradients without dx: the depthwise backward-data pass is skipped, the gradients are the same
    rc, dx6, g6 = cell.backward(r, want_dx=False)
    assert rc == 0 and dx6 is None and all(torch.equal(a, b) for a, b in zip(g6.values(), g0.values()))


def test_entry_points_refuse_a_changed_descriptor_before_launching():
    """the bit is checked again by every entry point: a descriptor that stopped describing an expand-free block after its plan
    (an expand pointer, another width) is TFNAS_EINVAL before anything is launched"""
    o, x, r, _, _, cell = _raw('img3x5_k5_relu_se')
    cell.forward()
    cell.d.g[0].w_expand = cell.w[0].data_ptr()
    with pytest.raises(RuntimeError, match='code -1'):
        cell.forward()
    cell.d.g[0].w_expand = None
    cell.d.g[0].mc = 24
    with pytest.raises(RuntimeError, match='code -1'):
        cell.forward()
    cell.d.g[0].mc = 16
    cell.forward()
    rc, dx, _ = cell.backward(r)
    assert rc == 0
