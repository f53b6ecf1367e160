"""The search steps of an extended-candidate supernet ON THE PATH LEVEL (model_search.Network(..., extended_paths=True): path
runner, weight arena, fused optimizer tails) against the oracle: one bi-sampling weight step and one architecture step of
tfnas_amd.search, each from identical state, against the oracle's w_step / a_step on an oracle Network built as
tests/test_gpu_skip_search.py / tests/test_gpu_mix_search.py build theirs -- stage 1 on the default primitives, the restatement
blocks of tests/_fused.py, _dil.py, _mix.py and the identity module of tests/_skip.py in stages 2-6 (tests/_pathsext.py).

32 x 32 images, batch 4; gates: those files' (logits 1e-3, expected latency 1e-3, post-step arch parameters 1e-3, loss 2e-3;
weights: atol 2e-5 + rtol 1e-3 * max|ref|).  The noise and rand_pos of the weight step are made on the CPU so that the ORACLE samples
the skip on each path -- in a run of cells and in a stage's last cell -- (asserted on the oracle's own indices)."""
import pytest
import torch

import _pathsext as px
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu


def _batch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 100, (4,), generator=g)
    ng = torch.empty(18, 8).exponential_(generator=g)
    rp = [int(v) for v in torch.randint(0, 7, (18,), generator=g)]
    na = torch.empty(18, 8).exponential_(generator=g)
    return x, y, ng, rp, na


def test_w_step_on_the_path_level_against_the_oracle():
    from tfnas_amd import search
    o, m = px.oracle_pair()
    assert not m.plain_candidates() and m.path_capable() and m._use_paths(torch.zeros(1).cuda())
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert st.runner is not None and st.arena is not None          # path level, weight arena, fused tails
    x, y, ng, rp, _ = _batch()
    # the gumbel path takes the skip in cells 6, 7 (a run in mid-stage) and 12 (a stage's last cell), the random path in 3, 4 (all
    # residual cells of stage 2) and 15
    for ci in (6, 7, 12):
        ng[ci, 7] = 1e-6
    for ci in (3, 4, 15):
        ng[ci, 7] = 50.0
        rp[ci] = 6
    before = {k: v.detach().clone() for k, v in o.named_parameters()}
    lo, logits_o, gi, ri = orc.w_step(o, x, y, oo[0], 5.0, noise_g=ng, rand_pos=rp)
    assert all(gi[ci] == 7 for ci in (6, 7, 12)) and all(ri[ci] == 7 for ci in (3, 4, 15))     # the ORACLE sampled the skips
    kinds = {type(c.m_ops[i]).__name__ for c, i in zip(o.cells(), gi)} | {type(c.m_ops[i]).__name__ for c, i in zip(o.cells(), ri)}
    assert {'IdentityRef', 'FusedRef'} <= kinds and len(kinds) >= 3
    lm, logits_m = search.w_step(st, x.cuda(), y.cuda(), mo[0], 5.0, noise_g=ng.cuda(), rand_pos=rp)
    torch.cuda.synchronize()
    print('w_step loss', float(lo), float(lm), 'logits', float((logits_m.cpu() - logits_o).abs().max()))
    assert abs(float(lo) - float(lm)) < 2e-3
    assert torch.allclose(logits_m.cpu(), logits_o, atol=1e-3, rtol=1e-3)
    touched = 0
    for (k, a), (k2, b) in zip(o.named_parameters(), m.named_parameters()):
        assert k == k2
        err, ref = float((b.detach().cpu() - a.detach()).abs().max()), float(a.detach().abs().max())
        assert err <= 2e-5 + 1e-3 * ref, (k, err, ref)
        touched += int(not torch.equal(a.detach(), before[k]))
    assert touched > 40


def test_a_step_on_the_path_level_against_the_oracle():
    from tfnas_amd import search
    o, m = px.oracle_pair()
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert st.runner is not None
    x, y, _, _, na = _batch()
    la_o, ll_o, lat_o, g_o = orc.a_step(o, x, y, oo[1], 15.0, 0.1, 5.0, noise=na)
    la_m, ll_m, lat_m, g_m = search.a_step(st, x.cuda(), y.cuda(), mo[1], 15.0, 0.1, 5.0, noise=na.cuda(), return_grads=True)
    torch.cuda.synchronize()
    print('a_step loss', float(la_o), float(la_m), 'lat', float(lat_o), float(lat_m))
    assert abs(float(lat_o) - float(lat_m)) < 1e-3 and abs(float(la_o) - float(la_m)) < 2e-3
    assert abs(float(ll_o) - float(ll_m)) < 1e-3
    for a, b in zip(o.arch_parameters(), m.arch_parameters()):
        assert torch.allclose(b.detach().cpu(), a.detach(), atol=1e-3), float((b.detach().cpu() - a.detach()).abs().max())
    # the skip slots of the residual cells of stages 2-5: a gradient arrived on both sides (stage 1 keeps the default primitives)
    names = [k for k, _ in o.named_parameters() if k.endswith('log_alphas') or k.endswith('betas')]
    cells = px.cell_names()
    n = 0
    for ci in px.residual_index():
        stg, b = cells[ci]
        if stg == 'stage1':
            continue
        k = names.index('%s.%s.log_alphas' % (stg, b))
        assert float(g_m[k][px.SKIP_IDX].abs()) > 0 and float(g_o[k][px.SKIP_IDX].abs()) > 0
        n += 1
    assert n == 11
