"""The two small kernels on every cell's data-gradient chain, against the CPU oracle at the project's own tolerances
(_hipcheck.check_cell: rtol 1e-4, atol 2e-5):
  k_mix_bwd_stats   BN3-backward sums: unrolled row steps with masked tails, one LDS pass for all accumulators
  k_bn2_gather[_few] per-image BN2-backward / SE-gate tables from the records of the project-dgrad epilogue
Swish throughout: no element is exempt (no ReLU kink mask), the comparison covers every element.  The shapes are the smallest
at which the thread mappings can still go wrong; each runs in soft mode (all 8 candidates, frozen weights) and sampled with
weight gradients for candidate 0 (no SE) and 5 (SE)."""
import copy

import pytest
import torch

import _hipcheck as hc
import tfnas_oracle as orc

MIDS = [32, 52, 28, 56, 36, 60, 40, 64]
RAGGED = [53, 107, 44, 88, 61, 96, 48, 79]           # the last channel quads of a group are partial
SHAPES = [
    # name, ic, oc, stride, H, W, N, mids
    # BN3 sums: 15 rows -- fewer than one workgroup's share and than one unrolled step; oc = 24 leaves 4 threads idle
    ('mix_few_rows_oc24', 24, 24, 1, 5, 3, 1, MIDS),
    # BN3 sums: 297 rows, no multiple of the unroll or of the row lanes; residual cell.  Gather: 99-pixel images, ragged widths
    ('mix_odd_rows_res', 40, 40, 1, 9, 11, 3, RAGGED),
    # BN3 sums: 3 row lanes, 16 idle threads (oc = 320), no residual
    ('mix_oc320', 192, 320, 1, 7, 7, 2, [576, 1152] * 4),
    # BN3 sums: 64 row lanes (oc = 16), stride 2, odd output extent
    ('mix_oc16_s2', 16, 16, 2, 9, 13, 2, [24, 40, 20, 36, 28, 44, 24, 48]),
    # gather: 128-row tiles touching 3-4 images, just above the 43-pixel limit of the record format
    ('gather_45px', 32, 48, 1, 5, 9, 7, [40, 72, 36, 64, 44, 80, 52, 68]),
    ('gather_49px', 32, 48, 1, 7, 7, 6, [40, 72, 36, 64, 44, 80, 52, 68]),
    # gather: 2-3 tiles per image, image boundaries inside tiles
    ('gather_196px', 80, 80, 1, 14, 14, 3, [96, 168, 104, 152, 120, 184, 88, 136]),
    # gather: 34 tiles per image, more than one unrolled round of 32 (one-candidate launches only gather at this size)
    ('gather_34_tiles', 16, 24, 1, 65, 65, 1, [24, 40, 28, 36, 32, 44, 24, 48]),
]
IDS = [s[0] for s in SHAPES]


def _inputs(cfg, cuda=True):
    name, ic, oc, s, H, W, N, mids = cfg
    torch.manual_seed(len(name))
    if cuda:
        o, m = hc.make_cell_pair(ic, oc, s, 'swish', mids, seed=len(name))
    else:                                             # the oracle half of make_cell_pair, same parameters
        from collections import OrderedDict
        mc = OrderedDict((i, int(v)) for i, v in enumerate(mids))

        class AnyLut(dict):
            def __missing__(self, key):
                v = self[key] = {int(v_): 1.0 for v_ in mids}
                return v
        o = orc.MixedOP(ic, oc, s, 'swish', mc, AnyLut())
        with torch.no_grad():
            for p in o.parameters():
                if p.dim() == 1 and p.numel() != 8:
                    p.copy_(torch.randn(p.shape) * 0.1)
            o.log_alphas.copy_(torch.log_softmax(torch.randn(8) * 0.5, -1))
        o.set_temperature(2.5)
        m = None
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, ic, H, W, generator=g)
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=g)
    e = torch.empty(8).exponential_(generator=g)
    return o, m, x, r, e


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', SHAPES, ids=IDS)
def test_soft_mode(cfg):
    o, m, x, r, e = _inputs(cfg)
    res = hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=False)
    assert 'kink_fraction' not in res                  # Swish: nothing was masked


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', SHAPES, ids=IDS)
@pytest.mark.parametrize('idx', [0, 5])
def test_sampled_mode_with_weight_grads(cfg, idx):
    o, m, x, r, e = _inputs(cfg)
    assert bool(o.m_ops[idx].se_channels) == (idx == 5)
    res = hc.check_cell(o, m, x, r, e, [idx], need_wgrad=True)
    assert 'kink_fraction' not in res


SUBSETS = [(0, 5), (1, 4, 6), (0, 2, 3, 5, 7), (0, 1, 2, 3, 4, 5, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize('idxs', SUBSETS, ids=['G%d' % len(s) for s in SUBSETS])
def test_group_counts_between_one_and_eight(idxs):
    """The search only launches 1 or 8 groups; the ABI takes any count, and k_mix_bwd_stats unrolls 3 / 2 / 2 / 1 row steps at
    G = 2 / 3-4 / 5-6 / 7-8.  Mixed launch of a subset (weights = the subset's softmax weights) against the oracle, frozen
    weights: out, dx and d wmix."""
    from tfnas_amd.functions import MixedOpFn
    o, m, x, r, e = _inputs(SHAPES[IDS.index('mix_odd_rows_res')])
    w_o = orc.gumbel_softmax(o.log_alphas, o.T, e)[list(idxs)].detach().requires_grad_(True)
    xo = x.clone().requires_grad_(True)
    out_o = sum(w_o[k] * o.m_ops[i](xo) for k, i in enumerate(idxs))
    (out_o * r).sum().backward()
    plan = m._plan(tuple(idxs))
    ps = plan.params()
    for p in ps:
        p.requires_grad_(False)
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w_m = w_o.detach().cuda().requires_grad_(True)
    out_m = MixedOpFn.apply(plan, xm, w_m, *ps)
    (out_m * r.cuda()).sum().backward()
    res = {'out': hc.err(out_m, out_o), 'dx': hc.err(xm.grad, xo.grad), 'dwmix': hc.err(w_m.grad, w_o.grad)}
    assert not hc.worst(res), hc.worst(res)


def _backward_bits(cfg, idxs):
    from tfnas_amd.functions import MixedOpFn
    o, m, x, r, e = _inputs(cfg)
    plan = m._plan(tuple(idxs))
    ps = plan.params()
    for p in ps:
        p.requires_grad_(False)
    w0 = orc.gumbel_softmax(o.log_alphas, o.T, e).detach().cuda() if len(idxs) > 1 else None
    outs = []
    for _ in range(2):
        xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = w0.clone().requires_grad_(True) if w0 is not None else None
        MixedOpFn.debug_sink, MixedOpFn.fwd_sink = [], []
        try:
            y = MixedOpFn.apply(plan, xm, w, *ps)
            (y * r.cuda()).sum().backward()
            torch.cuda.synchronize()
            dbg = MixedOpFn.debug_sink[0]
            d = dbg['d']                               # (the pad columns between the groups are nobody's: never written)
            dZ = dbg['dZ'].view(-1, d.M)
            dZ = torch.cat([dZ[:, d.g[g].off:d.g[g].off + d.g[g].mc] for g in range(len(idxs))], 1)
        finally:
            MixedOpFn.debug_sink = MixedOpFn.fwd_sink = None
        outs.append((dZ, xm.grad.clone(), w.grad.clone() if w is not None else None))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize('idxs', [tuple(range(8)), (5,)], ids=['soft', 'sampled'])
def test_backward_twice_gives_identical_bits(idxs):
    """the order of every partial sum is fixed by the code: the same launch twice gives the same bits in dZ, dx and d wmix"""
    a, b = _backward_bits(SHAPES[IDS.index('gather_196px')], idxs)
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v)


def _oracle_grads(o, x, r, e, idxs, dtype):
    o = copy.deepcopy(o).to(dtype)
    x = x.to(dtype).clone().requires_grad_(True)
    soft = len(idxs) > 1
    w = None
    if soft:
        w = orc.gumbel_softmax(o.log_alphas, o.T, e.to(dtype))
        w.retain_grad()
    dets, ys = [], []
    for i in idxs:
        det = {}
        ys.append(o.m_ops[i](x, det))
        det['Z'].retain_grad()
        det['Eh'].retain_grad()
        dets.append(det)
    out = sum(w[i] * y for i, y in zip(idxs, ys)) if soft else ys[0]
    (out * r.to(dtype)).sum().backward()
    res = {'out': out.detach(), 'dx': x.grad}
    if soft:
        res['dwmix'] = w.grad
    for i, det in zip(idxs, dets):
        res['g%d.dZ' % i] = det['Z'].grad
        res['g%d.dEh' % i] = det['Eh'].grad
        res['g%d.P' % i] = det['P'].detach()
        if not soft:
            for k, p in o.m_ops[i].params().items():
                res['g%d.grad_%s' % (i, k)] = p.grad
    return res


@pytest.mark.parametrize('cfg', SHAPES, ids=IDS)
def test_fp32_oracle_is_inside_the_tolerances_on_these_inputs(cfg):
    """No GPU: the fp32 oracle against its own fp64 run, at the tolerances of the GPU comparisons above -- so a failure there can
    only come from the kernels, not from inputs on which fp32 itself is that far off."""
    o, _, x, r, e = _inputs(cfg, cuda=False)
    subsets = [list(s) for s in SUBSETS] if cfg[0] == 'mix_odd_rows_res' else []
    for idxs in [list(range(8)), [0], [5]] + subsets:
        a = _oracle_grads(o, x, r, e, idxs, torch.float32)
        b = _oracle_grads(o, x, r, e, idxs, torch.float64)
        res = {k: hc.err(a[k], b[k]) for k in a}
        assert not hc.worst(res), hc.worst(res)
