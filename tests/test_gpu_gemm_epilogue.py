"""The tile epilogue of the row-tiled GEMMs (gemm_core.h: emit_tile_rows -- k_expand_fwd, k_project_fwd, k_project_dgrad with and
without the BN2-table epilogue, k_expand_dgrad) where the small-shape suites cannot reach it, forward + backward through the C ABI
against a float64 run of the oracle at the project's tolerances (_hipcheck.worst: rtol 1e-4, atol 2e-5 on the tensor's maximum).

A wave stages its 16-row slabs through its own piece of LDS and orders the slab's stores, its reads and the next slab's stores at
wave level only; the workgroup meets once per tile, behind the last slab.  Two things follow that nothing else tests:

  * several row tiles per workgroup -- the staging area aliases the K loop's operand buffers, so the NEXT tile's first operand
    stores race with a slow wave's last slab unless the barrier behind the slabs holds.  A workgroup walks more than one tile only
    above 1024 row tiles (gemm_kernels.hip: row_blocks): N = 1, 363 x 363, stride 1, 16 input channels and one candidate of 48 mid
    channels is 131 769 pixels = 1030 row tiles, the last with 57 valid rows; on the expand side (k_expand_fwd) always, with 24
    output channels on the project side (k_project_fwd, k_project_dgrad with the BN2-table epilogue: one candidate, 363 * 363 >= 43
    pixels per image) too.  test_row_tile_arithmetic re-derives the grids from the planner's rule.  (k_expand_dgrad's rule allows
    4096 row blocks: it walks one tile per workgroup here, and a shape above 4096 tiles costs a float64 reference of gigabytes.)
  * skew -- waves of one workgroup no longer wait for each other between slabs, and in all-candidate launches whose group widths
    differ by a factor of two neighbouring workgroups leave their K loops at different times: 14 x 14 images (N = 3, N = 5) and
    ragged 45- / 49- / 77- / 171-pixel ones, the three column-tile widths 64 / 80 / 112 (at 80 and 112 a lane of the table epilogue
    owns two columns), and a last tile that holds ONE valid row (5 x 77 and 3 x 171 pixels are 1 modulo 128).

Swish and ReLU, fp32-MFMA and split-bf16 loop (forced on every launch), with and without squeeze-excite.  ReLU launches
materialise E, so the reference replays the HIP launch's own ReLU decisions (_hipcheck.hip_relu_masks / ReluInjector: a replayed
decision may differ from the float64 one only within 2e-5 of the kink) and no element is exempt.

Every case runs twice from the same inputs and all outputs (dZ and the forward's D included) must be bit-identical: a
missing ordering shows as a flipped bit long before it shows in a tolerance."""
import copy
from collections import OrderedDict

import pytest
import torch

import _hipcheck as hc
import tfnas_oracle as orc

FLIP_TAU = 2e-5                 # _hipcheck.compare_cell's bound on |pre-activation| at a replayed ReLU decision that differs

# ------------------------------------------------------------------------------------------------ shapes
# several tiles per workgroup: name, ic, oc, H, W, N, mids, activation
MT = [
    ('mt_oc16_swish', 16, 16, 363, 363, 1, [48] * 8, 'swish'),
    ('mt_oc16_relu', 16, 16, 363, 363, 1, [48] * 8, 'relu'),
    ('mt_oc24_swish', 16, 24, 363, 363, 1, [48] * 8, 'swish'),
    ('mt_oc24_relu', 16, 24, 363, 363, 1, [48] * 8, 'relu'),
]
MT_CASES = [(cfg, gemm, cand) for cfg in MT for gemm in ('f32', 'x3') for cand in (0, 4)]       # candidate 0: no SE, 4: SE
MT_IDS = ['%s-%s-%s' % (c[0][0], c[1], 'se' if c[2] == 4 else 'nose') for c in MT_CASES]

W64x2 = [200, 400, 208, 416, 216, 432, 224, 448]       # every group >= 200: 64-wide tiles; neighbours differ by a factor of two
W80x2 = [72, 144] * 4                                  # 80-wide tiles
W112x2 = [112, 224] * 4                                # 112-wide tiles
SKEW = [
    ('px196_n3_w64', 40, 40, 14, 14, 3, W64x2, 'swish'),
    ('px196_n5_w80', 40, 40, 14, 14, 5, W80x2, 'relu'),
    ('px196_n3_w112', 40, 40, 14, 14, 3, W112x2, 'swish'),
    ('px49_n5_w64', 32, 48, 7, 7, 5, W64x2, 'relu'),
    ('px45_n3_w112', 32, 48, 5, 9, 3, W112x2, 'relu'),
    ('px77_n5_w80_onerow', 32, 48, 7, 11, 5, W80x2, 'swish'),       # 385 rows = 3 * 128 + 1
    ('px171_n3_w112_onerow', 32, 48, 9, 19, 3, W112x2, 'swish'),    # 513 rows = 4 * 128 + 1
    ('px77_n5_w64_onerow', 32, 48, 11, 7, 5, W64x2, 'swish'),
]
SKEW_CASES = [(cfg, gemm) for cfg in SKEW for gemm in ('f32', 'x3')]
SKEW_IDS = ['%s-%s' % (c[0][0], c[1]) for c in SKEW_CASES]


# ------------------------------------------------------------------------------------------------ the planner's rule, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def row_blocks(rows, other, cap, slots, max_gx=1024):
    """gemm_kernels.hip: row_blocks (the gx that minimises rounds * tiles per workgroup, the larger on ties)."""
    nrt = _cdiv(rows, 128)
    lim = max(1, min(nrt, cap, max_gx))
    best, best_cost = 1, None
    for gx in range(1, lim + 1):
        cost = _cdiv(gx * max(other, 1), slots) * _cdiv(nrt, gx)
        if best_cost is None or cost <= best_cost:
            best, best_cost = gx, cost
    return best


def test_row_tile_arithmetic():
    """363 x 363 pixels: 1030 row tiles, more than any grid of the capped launches has row blocks (1024: four resident workgroups
    per CU, the fp32 loop of the narrow tiles; 768: three, the split-bf16 loop), the last tile 57 rows; the one-row shapes"""
    P = 363 * 363
    assert _cdiv(P, 128) == 1030 and P - 1029 * 128 == 57
    for slots, gx, two in ((1024, 1024, 6), (768, 768, 262)):
        assert row_blocks(P, 1, 1024, slots) == gx          # one column tile (48 mid channels / 16 or 24 output channels)
        assert sum(1 for b in range(gx) if len(range(b, 1030, gx)) == 2) == two
    assert row_blocks(P, 1, 1 << 30, 1024, 4096) == 1030    # k_expand_dgrad: one tile per workgroup
    for cfg in SKEW:
        if cfg[0].endswith('onerow'):
            assert (cfg[3] * cfg[4] * cfg[5]) % 128 == 1
        assert cfg[3] * cfg[4] >= 43                         # the record format of the BN2-table epilogue


# ------------------------------------------------------------------------------------------------ HIP side
def _inputs(cfg, gemm):
    from tfnas_amd import functions as F
    name, ic, oc, H, W, N, mids, act = cfg
    o, m = hc.make_cell_pair(ic, oc, 1, act, mids, seed=len(name))
    # fx = False: the all-candidate launches of the 14 x 14 shapes run the expand GEMMs too (not the fused per-image kernels)
    F.adopt_modes(m, F.HipModes(gemm=gemm, everywhere=True, route=F.route_bits(fx=False, fold=True)))
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, ic, H, W, generator=g)
    r = torch.randn(N, oc, H, W, generator=g)
    e = torch.empty(8).exponential_(generator=g)
    return o, m, x, r, e


def hip_run(cfg, gemm, idxs, runs=2):
    """The launch ``idxs`` of the cell (eight candidates: soft mode, frozen weights; one: sampled, with weight gradients) `runs`
    times from the same inputs.  Returns (per run an OrderedDict name -> tensor, context for the reference)."""
    from tfnas_amd.functions import MixedOpFn
    o, m, x, r, e = _inputs(cfg, gemm)
    soft = len(idxs) > 1
    plan = m._plan(tuple(idxs))
    ps = plan.params()
    for p in ps:
        p.requires_grad_(not soft)
    w0 = orc.gumbel_softmax(o.log_alphas, o.T, e).detach() if soft else None
    outs, frec = [], None
    for _ in range(runs):
        for p in ps:
            p.grad = None
        xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = w0.cuda().requires_grad_(True) if soft else None
        MixedOpFn.debug_sink, MixedOpFn.fwd_sink = [], []
        try:
            y = MixedOpFn.apply(plan, xm, w, *ps)
            (y * r.cuda()).sum().backward()
            torch.cuda.synchronize()
            dbg, frec = MixedOpFn.debug_sink[0], MixedOpFn.fwd_sink[0]
        finally:
            MixedOpFn.debug_sink = MixedOpFn.fwd_sink = None
        d = dbg['d']

        def cols(t):                                   # (the pad columns between the groups are nobody's: never written)
            t = t.view(-1, d.M)
            return torch.cat([t[:, d.g[g].off:d.g[g].off + d.g[g].mc] for g in range(len(idxs))], 1).clone()
        t = OrderedDict(out=y.detach().clone(), dx=xm.grad.clone())
        if soft:
            t['dwmix'] = w.grad.clone()
        else:
            for k, p in enumerate(ps):
                t['grad%d' % k] = p.grad.clone()
        npx = x.shape[0] * x.shape[2] * x.shape[3]
        t['D'] = cols(frec['D'][:npx * d.M])
        t['dZ'] = cols(dbg['dZ'][:npx * d.M])
        outs.append(t)
    for p in ps:
        p.grad = None
    return outs, dict(o=o, x=x, r=r, w0=w0, frec=frec, idxs=idxs, E=frec['E'])


# ------------------------------------------------------------------------------------------------ float64 reference
_REF = {}


def ref64(cfg, ctx):
    """out, dx, d wmix / the weight gradients of the launch from a float64 copy of the oracle cell (same fp32 parameter, input and
    mix-weight values).  Swish: computed once per (shape, launch) and shared by the GEMM arithmetics; ReLU: under the replayed
    decisions of this HIP launch."""
    o, x, r, w0, idxs = ctx['o'], ctx['x'], ctx['r'], ctx['w0'], ctx['idxs']
    relu = cfg[7] == 'relu'
    key = (cfg[0], tuple(idxs))
    if not relu and key in _REF:
        return _REF[key]
    soft = len(idxs) > 1
    o64 = copy.deepcopy(o).double()
    o64.zero_grad()
    x64 = x.double().clone().requires_grad_(True)
    w64 = w0.double().clone().requires_grad_(True) if soft else None
    inj = None
    if relu:
        assert ctx['E'] is not None, 'this launch did not materialise E: its first ReLU decisions cannot be replayed'
        ctx['frec']['fx'] = False
        masks = []
        for gi, (m1, m2) in zip(idxs, hc.hip_relu_masks(ctx['frec'])):
            masks += [m1, m2] + ([None] if o.m_ops[gi].se_channels else [])      # (SE hidden ReLU: the oracle's own)
        inj = hc.ReluInjector(masks)
    orc.RELU_HOOK = inj
    try:
        ys = [o64.m_ops[i](x64) for i in idxs]
    finally:
        orc.RELU_HOOK = None
    if inj is not None:
        inj.done()
        assert inj.max_abs_at_flip <= FLIP_TAU, ('a replayed ReLU decision differs far from the kink', inj.flips, inj.max_abs_at_flip)
    out = sum(w64[i] * y for i, y in zip(idxs, ys)) if soft else ys[0]
    (out * r.double()).sum().backward()
    ref = OrderedDict(out=out.detach(), dx=x64.grad)
    if soft:
        ref['dwmix'] = w64.grad
    else:
        op = o64.m_ops[idxs[0]].params()
        names = ['expand', 'dw', 'proj'] + (['se_rw', 'se_rb', 'se_ew', 'se_eb'] if o.m_ops[idxs[0]].se_channels else [])
        for k, n in enumerate(names):
            ref['grad%d' % k] = op[n].grad
    if not relu:
        _REF[key] = ref
    return ref


def check(cfg, gemm, idxs):
    (a, b), ctx = hip_run(cfg, gemm, idxs)
    ref = ref64(cfg, ctx)
    res = OrderedDict()
    for k, v in ref.items():
        assert tuple(a[k].shape) == tuple(v.shape), (k, tuple(a[k].shape), tuple(v.shape))
        res[k] = ((a[k].detach().double().cpu() - v).abs().max().item(), v.abs().max().item())
    print(cfg[0], gemm, idxs, ' '.join('%s %.3g/%.3g' % (k, v[0], v[1]) for k, v in res.items()))
    bad = hc.worst(res)
    assert not bad, bad
    assert list(a) == list(b) and len(a) >= len(ref) + 2
    for k in a:
        assert torch.equal(a[k], b[k]), 'the second run differs in ' + k


@pytest.mark.gpu
@pytest.mark.parametrize('cfg,gemm,cand', MT_CASES, ids=MT_IDS)
def test_several_tiles_per_workgroup(cfg, gemm, cand):
    """one candidate, weight gradients wanted: 1030 row tiles on 1024 (fp32 loop) or 768 (split-bf16) row blocks"""
    assert orc.OP_KERNEL[cand] == 3 and bool(orc.OP_SE_MULT[cand]) == (cand == 4)
    check(cfg, gemm, [cand])


@pytest.mark.gpu
@pytest.mark.parametrize('cfg,gemm', SKEW_CASES, ids=SKEW_IDS)
def test_wave_private_staging_under_skew(cfg, gemm):
    """all eight candidates (frozen weights), group widths alternating by a factor of two"""
    mids = cfg[6]
    assert all(b == 2 * a for a, b in zip(mids[::2], mids[1::2]))
    check(cfg, gemm, list(range(8)))
