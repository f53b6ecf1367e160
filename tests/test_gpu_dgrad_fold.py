"""The BN2-table epilogue of k_project_dgrad<NT, MM, FOLD> (gemm_kernels.hip: fold_slab and the record combine) against the CPU
oracle at the project's own tolerances (_hipcheck.check_cell: rtol 1e-4, atol 2e-5).

The epilogue keeps a wave's rows, its image boundary and the end of the tensor in scalar registers and adds the rows four at a
time; the shapes are the smallest at which that row-range logic can go wrong:
  * 7 x 7 and 5 x 9 images (49 / 45 pixels, just above the record format's 43-pixel limit) with N = 5 / 7: every wave's 32 rows hold
    an image boundary, a 128-row tile touches 3-4 images, and Po = 245 / 315 is a multiple of neither 128 nor 16 nor 4 (the last
    tile of N = 5, 7 x 7 has 117 rows: one wave's second slab has 5 valid rows);
  * 14 x 14, N = 3: boundaries at rows 196 and 392 = row 4 of a slab, i.e. exactly between two groups of four rows;
  * 65 x 65, N = 1 (Po = 4225): no boundary at all and ONE valid row in the last tile (one-candidate launches only: above 28 x 28
    the all-candidate launch takes the tables in their own pass);
  * mid widths for which the launch plan picks each column-tile width: 64 (all mids >= 200), 80 (72 | 144) and 112 (112) -- at 80
    and 112 a lane owns two columns and the second pass is partly empty -- and one ragged list (mc % 4 != 0: the fp32 loop with the
    guarded column limits, n0 + col < mc against < mcp).
Each shape runs in soft mode (all 8 candidates, frozen weights) and sampled with weight gradients for candidate 0 (no SE) and
5 (SE), with the fp32-MFMA and the split-bf16 GEMM loop (forced on every launch), and on both routes: tables in the epilogue and
tables in their own pass (k_bn2_pool) -- the same mathematics.

Swish: no element is exempt.  ReLU (fold_slab<RELU> is its own instantiation; one shape per tile width): these launches
materialise E, so check_cell replays the HIP launch's own ReLU decisions in the oracle and compares every element strictly -- the
kink cap (max_kink_fraction = 1e-4) only binds where a mask is used at all, and none is here."""
import pytest
import torch

import _hipcheck as hc
import tfnas_oracle as orc

W64 = [200, 264, 208, 232, 216, 248, 224, 256]       # every group >= 200: 64-wide column tiles
W80 = [72, 144] * 4                                  # 80-wide tiles (a lane's second column: 16 of 64 lanes)
W112 = [112] * 8                                     # 112-wide tiles (second column: 48 of 64 lanes)
RAGGED = [53, 107, 44, 88, 61, 96, 48, 79]           # mc % 4 != 0: fp32 loop, guarded column limits
BIG1 = [52, 40, 28, 36, 32, 72, 24, 48]              # one-candidate launches: candidate 0 -> 64-wide tiles, 5 -> 80-wide
BIG2 = [112, 40, 28, 36, 32, 200, 24, 48]            # candidate 0 -> 112-wide, 5 -> 64-wide
SHAPES = [
    # name, ic, oc, stride, H, W, N, mids, activation, soft mode too
    ('px49_n5_w64', 32, 48, 1, 7, 7, 5, W64, 'swish', True),
    ('px49_n5_w80', 32, 48, 1, 7, 7, 5, W80, 'swish', True),
    ('px49_n5_w112', 32, 48, 1, 7, 7, 5, W112, 'swish', True),
    ('px45_n7_ragged', 32, 48, 1, 5, 9, 7, RAGGED, 'swish', True),
    ('px45_n7_w112', 32, 48, 1, 5, 9, 7, W112, 'swish', True),
    ('px196_n3_w80', 40, 40, 1, 14, 14, 3, W80, 'swish', True),
    ('px196_n3_ragged', 40, 40, 1, 14, 14, 3, RAGGED, 'swish', True),
    ('px4225_n1_a', 16, 24, 1, 65, 65, 1, BIG1, 'swish', False),
    ('px4225_n1_b', 16, 24, 1, 65, 65, 1, BIG2, 'swish', False),
    ('relu_px49_n5_w64', 32, 48, 1, 7, 7, 5, W64, 'relu', True),
    ('relu_px49_n5_w80', 32, 48, 1, 7, 7, 5, W80, 'relu', True),
    ('relu_px45_n7_w112', 32, 48, 1, 5, 9, 7, W112, 'relu', True),
]
IDS = [s[0] for s in SHAPES]
# (GEMM arithmetic, tables in the epilogue); ragged widths always run the fp32 loop: one arithmetic is enough there
CASES = [(cfg, gemm, fold) for cfg in SHAPES for gemm in ('f32', 'x3') for fold in (True, False)
         if not (gemm == 'x3' and any(m % 4 for m in cfg[7]))]
CASE_IDS = ['%s-%s-%s' % (c[0][0], c[1], 'fold' if c[2] else 'pool') for c in CASES]


def _inputs(cfg, gemm='f32', fold=True):
    from tfnas_amd import functions as F
    name, ic, oc, s, H, W, N, mids, act, _ = cfg
    o, m = hc.make_cell_pair(ic, oc, s, act, mids, seed=len(name))
    F.adopt_modes(m, F.HipModes(gemm=gemm, everywhere=True, route=F.route_bits(fold=fold)))
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, ic, H, W, generator=g)
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=g)
    e = torch.empty(8).exponential_(generator=g)
    return o, m, x, r, e


@pytest.mark.gpu
@pytest.mark.parametrize('cfg,gemm,fold', CASES, ids=CASE_IDS)
def test_tables_against_oracle(cfg, gemm, fold):
    """soft mode (frozen weights) and sampled mode with weight gradients, candidate 0 (no SE) and 5 (SE)"""
    launches = ([list(range(8))] if cfg[9] else []) + [[0], [5]]
    for idxs in launches:
        o, m, x, r, e = _inputs(cfg, gemm, fold)
        if len(idxs) == 1:
            assert bool(o.m_ops[idxs[0]].se_channels) == (idxs[0] == 5)
        res = hc.check_cell(o, m, x, r, e, idxs, need_wgrad=len(idxs) == 1, max_kink_fraction=1e-4)
        assert 'kink_fraction' not in res                  # nothing was masked: Swish, or ReLU under replayed decisions


def _backward_bits(cfg, idxs):
    from tfnas_amd.functions import MixedOpFn
    o, m, x, r, e = _inputs(cfg)
    soft = len(idxs) > 1
    plan = m._plan(tuple(idxs))
    ps = plan.params()
    for p in ps:
        p.requires_grad_(not soft)
    w0 = orc.gumbel_softmax(o.log_alphas, o.T, e).detach().cuda() if soft else None
    outs = []
    for _ in range(2):
        for p in ps:
            p.grad = None
        xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = w0.clone().requires_grad_(True) if soft else None
        MixedOpFn.debug_sink, MixedOpFn.fwd_sink = [], []
        try:
            y = MixedOpFn.apply(plan, xm, w, *ps)
            (y * r.cuda()).sum().backward()
            torch.cuda.synchronize()
            dbg = MixedOpFn.debug_sink[0]
            d = dbg['d']                               # (the pad columns between the groups are nobody's: never written)
            dZ = dbg['dZ'].view(-1, d.M)
            dZ = torch.cat([dZ[:, d.g[g].off:d.g[g].off + d.g[g].mc] for g in range(len(idxs))], 1).clone()
        finally:
            MixedOpFn.debug_sink = MixedOpFn.fwd_sink = None
        outs.append([dZ, xm.grad.clone()] + ([w.grad.clone()] if soft else [p.grad.clone() for p in ps]))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize('idxs', [tuple(range(8)), (0,), (5,)], ids=['soft', 'sampled0', 'sampled5'])
@pytest.mark.parametrize('name', ['px49_n5_w80', 'px196_n3_ragged'])
def test_backward_twice_gives_identical_bits(name, idxs):
    """the order of every partial sum is fixed by the code: the same launch twice gives the same bytes in dZ, dx, d wmix (soft mode)
    and every weight gradient (sampled mode)"""
    a, b = _backward_bits(SHAPES[IDS.index(name)], idxs)
    assert len(a) == len(b) and len(a) >= 3
    for u, v in zip(a, b):
        assert torch.equal(u, v)
