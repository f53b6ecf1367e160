"""The path level on an extended-candidate supernet (model_search.Network(..., extended_paths=True); tests/_pathsext.py: every
kind, a dilated, a MixConv and a 7 x 7 candidate in every cell, a skip in every residual one) against the per-cell route the same
network takes without the keyword: same kernels, so search iterations, the drop-in forward's gradients and the sampled skips must
come out bit-identical; the fused optimizer tails against torch.optim; the plan rules at the C ABI.

32 x 32 images at batch 4 (the existing search tests' shape) and 64 x 64 at batch 2 (more than one pixel in stages 3-5)."""
import pytest
import torch
import torch.nn.functional as F

import _kinds
import _pathsext as px
import _skip

pytestmark = pytest.mark.gpu

EINVAL = -1
# cells: stage1 0-1, stage2 2-4, stage3 5-8, stage4 9-12, stage5 13-16, stage6 17.  rand_pos 6 = the last of the seven candidates
# the gumbel pass left: the skip of a residual cell (unless the gumbel pass took it -- then it was sampled anyway)
LAST = {1, 4, 8, 12, 16}                                   # residual cells that close their stage
SKIP_AT = [
    {3, 8, 5},                # a depth-choice cell in mid-stage, the last cell of a stage; candidate 7 of a non-residual cell
    {6, 7, 15, 16, 1},        # a run of two before a computing cell, a run of two up to the stage's end, stage 1's last cell
    {10, 11, 12, 4, 17},      # a run of three: every residual cell of stage 4
    {14, 3, 4},               # one skip between computing cells, every residual cell of stage 2
]


def _rand_pos(step):
    return [6 if ci in SKIP_AT[step] else (3 * ci + step) % 6 for ci in range(18)]


def _iterate(ext, B, size, pairs=2):
    from tfnas_amd import search
    old_f, old_t = search.FUSED_OPT, search.FUSED_TAIL
    search.FUSED_OPT = False               # (same torch.optim tail on both sides: this test is about the path level)
    search.FUSED_TAIL = False              # (... and the same stock classifier + cross-entropy)
    try:
        m = px.model(True if ext else None)
        st = search.SearchState(m)
        probe = torch.zeros(1, device='cuda')
        if ext:
            assert st.runner is not None and m._use_paths(probe)
        else:
            assert st.runner is None and not m._use_paths(probe)
        ow, oa = search.make_optimizers(m)
        noise = search.NoiseSource(11)
        gen = torch.Generator(device='cuda').manual_seed(5)
        lats = []

        def batch():
            return (torch.randn(B, 3, size, size, device='cuda', generator=gen),
                    torch.randint(0, 100, (B,), device='cuda', generator=gen))
        with px.Recorder(m) as rec:
            for p in range(pairs):
                b0, b1, ba = batch(), batch(), batch()
                search.w_step(st, b0[0], b0[1], ow, 5.0, noise.exp('cuda'), _rand_pos(2 * p))
                _, _, lat, g = search.a_step(st, ba[0], ba[1], oa, 15.0, 0.1, 5.0, noise.exp('cuda'), return_grads=True)
                lats.append((float(lat), [t.clone() for t in g]))
                search.w_step(st, b1[0], b1[1], ow, 5.0, noise.exp('cuda'), _rand_pos(2 * p + 1))
        torch.cuda.synchronize()
        return {k: p.detach().clone() for k, p in m.named_parameters()}, lats, rec.seen
    finally:
        search.FUSED_OPT, search.FUSED_TAIL = old_f, old_t


@pytest.mark.parametrize('B,size', px.SHAPES, ids=lambda v: str(v))
def test_path_level_iterations_are_bit_identical_to_the_per_cell_route(B, size):
    pa, la, seen_a = _iterate(True, B, size)
    pb, lb, seen_b = _iterate(False, B, size)
    assert sorted(seen_a) == sorted(seen_b)                 # both sides sampled the same sub-networks (the per-cell sweep
                                                            # samples a cell's two paths together, the path level path by path)
    res = set(px.residual_index())
    assert {i for ci, i in seen_a} == set(range(8))         # every kind was sampled ...
    assert any(i == px.SKIP_IDX for ci, i in seen_a if ci not in res)       # ... the eighth candidate of a non-residual cell too
    skips = {ci for ci, i in seen_a if ci in res and i == px.SKIP_IDX}
    assert skips & LAST and skips - LAST                    # a skip in a last-of-stage cell and in a depth-choice cell in mid-stage
    assert {6, 7} <= skips and {10, 11, 12} <= skips        # runs of skips
    for k in pa:
        assert torch.equal(pa[k], pb[k]), (k, float((pa[k] - pb[k]).abs().max()))
    for (l1, g1), (l2, g2) in zip(la, lb):
        assert abs(l1 - l2) < 1e-5                         # (the six stage latencies are summed in a different order)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)


def _run_opt(fused, B=4, size=32):
    from tfnas_amd import search
    old = search.FUSED_OPT
    search.FUSED_OPT = fused
    try:
        m = px.model(True)
        st = search.SearchState(m)
        assert st.runner is not None
        ow, oa = search.make_optimizers(m)
        noise = search.NoiseSource(4)
        gen = torch.Generator(device='cuda').manual_seed(8)

        def batch():
            return (torch.randn(B, 3, size, size, device='cuda', generator=gen),
                    torch.randint(0, 100, (B,), device='cuda', generator=gen))
        # (alpha-step first: it does not touch the weights, and the w-step depends on the alphas only through the sampled indices,
        # so both steps start from bit-identical inputs in the two runs: tests/test_gpu_paths.py)
        b0, ba = batch(), batch()
        search.a_step(st, ba[0], ba[1], oa, 15.0, 0.1, 5.0, noise.exp('cuda'))
        with px.Recorder(m) as rec:
            search.w_step(st, b0[0], b0[1], ow, 5.0, noise.exp('cuda'), _rand_pos(1))
        torch.cuda.synchronize()
        mom = {k: ow.state[p]['momentum_buffer'].clone() for k, p in m.named_parameters() if p in ow.state}
        if fused:
            st.export_optimizer_state(oa)
        adam = {k: (oa.state[p]['exp_avg'].clone(), oa.state[p]['exp_avg_sq'].clone(), float(oa.state[p]['step']))
                for k, p in m.named_parameters() if p in oa.state}
        return {k: p.detach().clone() for k, p in m.named_parameters()}, mom, adam, rec.seen
    finally:
        search.FUSED_OPT = old


def test_fused_tails_on_an_extended_network_match_torch_optim():
    """clip + SGD over the arena ranges of the sampled candidates (a skip owns the empty range) and clip + Adam + projection, one
    step of each kind from the same start, against clip_grad_norm_ + torch.optim: the tolerances of
    tests/test_gpu_paths.py::test_fused_clip_sgd_and_adam_projection_match_torch_optim"""
    pa, ma, aa, seen = _run_opt(True)
    pb, mb, ab, seen_b = _run_opt(False)
    assert seen == seen_b and any(i == px.SKIP_IDX and ci in set(px.residual_index()) for ci, i in seen)
    for k in pa:
        tol = 2e-6 if (k.endswith('log_alphas') or k.endswith('betas')) else 1e-7 + 1e-6 * float(pb[k].abs().max())
        assert torch.allclose(pa[k], pb[k], atol=tol, rtol=0), (k, float((pa[k] - pb[k]).abs().max()))
    for k in mb:
        assert torch.allclose(ma[k], mb[k], atol=1e-7 + 1e-5 * float(mb[k].abs().max()), rtol=0), k
    assert set(aa) == set(ab)
    for k in ab:
        assert aa[k][2] == ab[k][2] == 1.0
        assert torch.allclose(aa[k][0], ab[k][0], atol=1e-7, rtol=1e-4), k
        assert torch.allclose(aa[k][1], ab[k][1], atol=1e-9, rtol=1e-4), k


def _forced_noise(picks):
    """Exp(1) draws under which the gumbel pass takes candidate picks[ci] of cell ci (a tiny draw is a huge Gumbel one)"""
    e = torch.empty(18, 8).exponential_(generator=torch.Generator().manual_seed(3)).clamp_min_(1e-3)
    for ci, k in enumerate(picks):
        e[ci, k] = 1e-9
    return e.cuda()


def _dropin(ext, configs, B, size):
    """For every (gumbel picks, rand_pos, repeats): model(x, True, 'gumbel') + model(x, True, 'random'), one backward of the summed
    loss, ``repeats`` times without zero_grad; the logits and every parameter's .grad after each backward."""
    from tfnas_amd import search
    m = px.model(True if ext else None)
    st = search.SearchState(m)
    st.require(True, False)                # (d betas of a sampled forward would take the per-cell route)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, 3, size, size, generator=gen).cuda()
    y = torch.randint(0, 100, (B,), generator=gen).cuda()
    out = []
    for picks, rp, repeats in configs:
        m.zero_grad()
        with px.Recorder(m) as rec:
            for _ in range(repeats):
                lg, _ = m(x, True, 'gumbel', exp_noise=_forced_noise(picks))
                lr, _ = m(x, True, 'random', rand_pos=rp)
                (F.cross_entropy(lg, y) + F.cross_entropy(lr, y)).backward()
                torch.cuda.synchronize()
                grads = {k: None if p.grad is None else p.grad.detach().clone() for k, p in m.named_parameters()}
                out.append((lg.detach().clone(), lr.detach().clone(), grads, list(rec.seen)))
    if ext:
        assert st.runner is not None and {'A', 'B'} <= set(st.runner._slots)      # both forwards ran on the path level
    else:
        assert st.runner is None
    return out


def test_drop_in_forward_gradients_accumulation_and_stages_of_skips():
    res = set(px.residual_index())
    # every kind on both paths, skips in mid-stage and last cells (cells 7, 15 on the gumbel path; 1, 3, 12 on the random one)
    g1 = [ci % 8 for ci in range(18)]
    r1 = [6 if ci in (1, 3, 12) else (3 * ci + 1) % 6 for ci in range(18)]
    # every residual cell of stages 2, 3 and 4 a skip on the gumbel path (each of those stages returns its sink over the output of
    # its first cell); the residual cells of stage 5 on the random one
    g2 = [7 if ci in (3, 4, 6, 7, 8, 10, 11, 12) else (ci + 3) % 7 for ci in range(18)]
    r2 = [6 if ci in (14, 15, 16) else (5 * ci + 2) % 6 for ci in range(18)]
    configs = [(g1, r1, 2), (g2, r2, 1)]
    B, size = px.SHAPES[0]
    a, b = _dropin(True, configs, B, size), _dropin(False, configs, B, size)
    for (lga, lra, ga, sa), (lgb, lrb, gb, sb) in zip(a, b):
        assert sa == sb
        assert torch.equal(lga, lgb) and torch.equal(lra, lrb)
        for k in gb:
            assert (ga[k] is None) == (gb[k] is None), k
            if gb[k] is not None:
                assert torch.equal(ga[k], gb[k]), (k, float((ga[k] - gb[k]).abs().max()))
    seen = a[1][3]
    assert {i for ci, i in seen} == set(range(8)) and {ci for ci, i in seen if ci in res and i == px.SKIP_IDX} >= {7, 15, 1, 3, 12}
    # a second backward without zero_grad doubles every gradient: written where .grad was None, added where it was not (the
    # kernels add to the arena range: the sum of the same partials once more, a few roundings of 2 g apart)
    n = 0
    for k, g in a[0][2].items():
        if g is None:
            continue
        g2x = a[1][2][k]
        tol = 8 * 2.0 ** -24 * float(g2x.abs().max())
        assert float((g2x - 2 * g).abs().max()) <= tol, (k, float((g2x - 2 * g).abs().max()), tol)
        n += int(float(g.abs().max()) > 0)
    assert n > 60
    # the stages of skips: sampled as asked, and (above) the logits and gradients of the per-cell route, which hands the SAME tensor
    # to every slot of the stage's sink
    seen3 = a[2][3]
    assert all((ci, 7) in seen3 for ci in (3, 4, 6, 7, 8, 10, 11, 12))


def test_a_stage_of_skips_returns_its_sink_over_its_input():
    """runner.sampled on a path whose residual cells of stage 3 are all skips: the stage's output is the sink of four copies of
    its first cell's output, sum(softmax(betas)) * out1 = out1 up to the rounding of the sink kernel"""
    from tfnas_amd import search
    from tfnas_amd.functions import SinkFn
    m = px.model(True)
    st = search.SearchState(m)
    st.require(True, False)                # (weights that want gradients: the route of the weight step on both sides -- a frozen
                                           #  sampled launch of the per-cell route may run E-free, the path level's does not)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    idxs = [0] * 18
    for ci in (6, 7, 8):
        idxs[ci] = px.SKIP_IDX
    feat = m._stem(x).detach()
    got = st.runner.sampled(feat, idxs).detach()
    # the per-cell walk of the same path
    h = feat
    for stg in m.stages():
        outs = [h]
        for blk in stg.blocks():
            blk._pre = idxs[m.cells().index(blk)]
            outs.append(blk(outs[-1], True, 'random')[0])
        if stg is m.stage3:
            assert outs[2] is outs[1] and outs[3] is outs[1] and outs[4] is outs[1]
        h, _ = SinkFn.apply(stg.betas, None, *outs[stg.start_res:])
    h = h.detach()
    torch.cuda.synchronize()
    assert torch.equal(got, h)


def test_plan_rules_at_the_c_abi():
    from tfnas_amd import _lib, functions
    rp = px.RawPlan()
    try:
        N, H, W = 2, 9, 7
        relu = _lib.ACT['relu']

        def fused(ic, oc, s):
            return _lib.describe_block(_lib.FUSED, N, H, W, ic, 40, 8, oc, 3, s, relu)

        def noexp(c, h, w):
            return _lib.describe_block(_lib.NOEXPAND, N, h, w, c, c, 8, c, 5, 1, relu, dilation=2)

        def packed(c, h, w):
            return _lib.describe_block(_lib.MBCONV, N, h, w, c, 53, 0, c, 7, 1, relu, mix_kernels=(3, 5, 7))

        def plain(c, h, w):
            return _lib.describe_block(_lib.MBCONV, N, h, w, c, 44, 8, c, 3, 1, relu)

        def skip(c, h, w):
            return functions.fill_pass_desc(_lib.TfnasCellDesc(), c, N, h, w)
        # one-kind, packed, dilated and pass-through cells of a sampled path (stride 2 first: start_res 1)
        rc, ws = rp.plan([fused(16, 24, 2), noexp(24, 5, 4), packed(24, 5, 4), skip(24, 5, 4)], False, 1)
        assert rc == 0 and ws.total > 0 and (ws.out_h, ws.out_w, ws.out_c) == (5, 4, 24)
        rc, ws1 = rp.plan([fused(16, 24, 2), noexp(24, 5, 4), packed(24, 5, 4), plain(24, 5, 4)], False, 1)
        assert rc == 0 and ws1.saved > ws.saved                          # a pass-through cell owns no workspace
        # a pass-through cell as the first cell of a stage whose input is a depth choice, and a run of them
        assert rp.plan([skip(24, 5, 4), skip(24, 5, 4), plain(24, 5, 4)], False, 0)[0] == 0
        assert rp.plan([plain(24, 5, 4), skip(24, 5, 4), skip(24, 5, 4)], False, 0)[0] == 0
        # mixed cells, with and without skip groups, in a soft path
        mixed = _kinds.mixed_desc(_kinds.EIGHT, N, H, W, 8, 8)
        mixed_s = _skip.skip_desc(_skip.EIGHT_S, N, H, W, 8, 8)
        assert rp.plan([mixed, mixed_s], True, 0)[0] == 0
        # ... refused: a pass-through cell in a soft path
        assert rp.plan([mixed, skip(8, H, W)], True, 0)[0] == EINVAL
        # a pass-through cell in a non-residual position (it changes the width / it strides)
        bad = skip(24, 5, 4)
        bad.oc = 32
        assert rp.plan([fused(16, 24, 2), bad], False, 1)[0] == EINVAL
        bad = skip(16, H, W)
        bad.stride = 2
        assert rp.plan([bad, plain(16, 5, 4)], False, 1)[0] == EINVAL
        # a pass-through descriptor that is not empty
        bad = skip(24, 5, 4)
        bad.g[0].mc = 24
        assert rp.plan([fused(16, 24, 2), bad], False, 1)[0] == EINVAL
        # G != 1 on a sampled path
        assert rp.plan([mixed, mixed_s], False, 0)[0] == EINVAL
        # an efree_mask_lo bit on a non-plain cell; legal on the plain cell next to it
        plain16 = _lib.describe_block(_lib.MBCONV, N, H, W, 16, 44, 0, 16, 3, 1, relu)
        assert rp.plan([plain16, noexp(16, H, W)], True, 0, efree_mask=1)[0] == 0
        assert rp.plan([plain16, noexp(16, H, W)], True, 0, efree_mask=2)[0] == EINVAL
        assert rp.plan([mixed, mixed_s], True, 0, efree_mask=1)[0] == EINVAL
        assert rp.plan([fused(16, 16, 1), plain16], True, 0, efree_mask=1)[0] == EINVAL
        # without TFNAS_PATH_EXTENDED every one of them is refused as it always was; an unknown flag bit is refused
        assert rp.plan([plain16, plain16], True, 0, path_flags=0)[0] == 0
        for cells, soft, sr in (([fused(16, 24, 2)], False, 1), ([noexp(16, H, W)], False, 0), ([packed(16, H, W)], False, 0),
                                ([plain16, skip(16, H, W)], False, 0), ([mixed], True, 0), ([mixed_s], True, 0)):
            assert rp.plan(cells, soft, sr)[0] == 0 and rp.plan(cells, soft, sr, path_flags=0)[0] == EINVAL
        assert rp.plan([plain16, plain16], True, 0, path_flags=2)[0] == EINVAL
    finally:
        rp.close()
