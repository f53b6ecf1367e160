"""GPU parity of the activations 'relu6' and 'h-swish' in search cells: sampled launches with weight gradients (one candidate
with squeeze-excite, one without), soft launches over all eight candidates with and without weight gradients, a cell that mixes
kernel sizes 3 / 5 / 7 with a new activation, the route word, and a MixedStage through the module API and the path level --
against the CPU oracle under tests/_acts.wrapped_oracle() (pinned to the reference in tests/test_act_oracle_pin.py).

Every tensor of every stage is compared at the project's standing gate, abs err <= 2e-5 + 1e-4 * max|ref| (_hipcheck.worst).
ReLU6's lower kink is replayed (the HIP launch's own decisions, rebuilt from the E and D it saved -- E is always materialised on
this route -- and injected into the oracle), never exempted: a replayed decision may differ from the oracle's own only within
2e-5 of 0.

The inputs reach every branch: x = randn * (1 + 11 s), s ~ Bernoulli(0.02) per pixel (with plain randn a batch-normalised
pre-activation essentially never exceeds 6, and ReLU6 would be tested as ReLU).  Each comparison asserts in the oracle that every
branch of the activation (below, between, above the two kinks) holds at least 0.1 % of the BN1 pre-activations and that none lies
within 2e-5 of an upper kink (6; -3 and 3), where a flipped decision would be a genuine O(1) gradient difference; the seeds were
picked so that the oracle alone satisfies this.  After BN2 the same is asserted for all three branches of hard-swish; ReLU6's
upper clamp is NOT reachable there in a search cell (the depthwise input is bounded by 6: measured 0.00 % on most of these
geometries), so only the branches below it are required here and that clamp is covered by the derived-block tests
(tests/test_gpu_acts_derived.py: gamma ~ 3, beta ~ 2)."""
import pytest
import torch

import _acts
import _k7
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [
    # name, N, ic, oc, H, W, stride, mids, seed of the input
    ('s1_res_two_column_tiles', 2, 24, 24, 10, 22, 1, [32, 52, 28, 56, 37, 60, 40, 62], 8),
    ('s2_odd', 2, 24, 40, 9, 13, 2, [36, 72, 40, 60, 33, 66, 44, 71], 7),
    ('s2_even', 2, 16, 24, 12, 10, 2, [24, 40, 20, 36, 29, 44, 24, 50], 7),
    ('s1_ragged_mids', 3, 40, 40, 8, 6, 1, [53, 107, 44, 88, 61, 96, 48, 79], 7),
    ('s1_14x14_where_swish_is_fused', 2, 80, 80, 14, 14, 1, [240, 477, 250, 480, 243, 470, 260, 466], 8),
    ('s2_37x41_where_relu_is_efree', 1, 16, 24, 37, 41, 2, [48, 96] * 4, 7),
]
_BY_NAME = {c[0]: c for c in SHAPES}
_IDS = [c[0] for c in SHAPES]
SE_IDX, PLAIN_IDX = 5, 1        # a sampled candidate with squeeze-excite (width ic) and one without


def oracle_inputs(cfg, act, ks=None):
    name, N, ic, oc, H, W, s, mids, seed = cfg
    o = _acts.make_oracle_cell(ic, oc, s, act, mids, ks=ks, seed=len(name))
    g = torch.Generator().manual_seed(seed)
    x = _acts.spiked_input((N, ic, H, W), g)
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=g)
    e = torch.empty(8).exponential_(generator=g)
    return o, x, r, e


def _inputs(cfg, act, ks=None):
    o, x, r, e = oracle_inputs(cfg, act, ks)
    return o, _k7.hip_cell_like(o), x, r, e


@pytest.mark.parametrize('idx', [SE_IDX, PLAIN_IDX], ids=['se', 'plain'])
@pytest.mark.parametrize('cfg', SHAPES, ids=_IDS)
@pytest.mark.parametrize('act', _acts.NEW_ACTS)
def test_sampled_candidate_with_weight_grads(act, cfg, idx):
    o, m, x, r, e = _inputs(cfg, act)
    assert bool(o.m_ops[idx].se_channels) == (idx == SE_IDX) and m.m_ops[idx].act_func == act
    res = _acts.check_cell(o, m, x, r, e, [idx], need_wgrad=True)
    assert 'g%d.grad_dw' % idx in res and 'g%d.dEh' % idx in res and 'g%d.E' % idx in res
    assert ('relu_flips' in res) == (act == 'relu6')
    if idx == SE_IDX:
        assert 'g%d.grad_se_rw' % idx in res and 'g%d.gate' % idx in res


@pytest.mark.parametrize('need_wgrad', [False, True], ids=['frozen', 'wgrad'])
@pytest.mark.parametrize('cfg', SHAPES, ids=_IDS)
@pytest.mark.parametrize('act', _acts.NEW_ACTS)
def test_soft_launch_over_all_candidates(act, cfg, need_wgrad):
    """all eight candidates in one launch; frozen weights is where a ReLU / Swish cell of the last two shapes would leave the
    materialised route (compare_cell asserts that this one does not: E is saved, tfnas_fx / efree_supported are 0)"""
    o, m, x, r, e = _inputs(cfg, act)
    res = _acts.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=need_wgrad)
    assert all('g%d.dEh' % i in res for i in range(8)) and 'dwmix' in res
    assert all(('g%d.grad_dw' % i in res) == need_wgrad for i in range(8))


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_odd'], _BY_NAME['s1_res_two_column_tiles']], ids=lambda c: c[0])
@pytest.mark.parametrize('act', _acts.NEW_ACTS)
def test_cell_mixing_kernel_sizes_3_5_7_with_a_new_activation(act, cfg):
    """both additive flag bits in one descriptor: TFNAS_CELL_K7 and TFNAS_CELL_ACTS"""
    from tfnas_amd import _lib
    o, m, x, r, e = _inputs(cfg, act, ks=_k7.SOFT_KS)
    assert [op.kernel_size for op in m.m_ops] == list(_k7.SOFT_KS)
    d, _ = m._plan(tuple(range(8))).desc(x.shape[0], x.shape[2], x.shape[3])
    assert d.flags & _lib.CELL_K7 and d.flags & _lib.CELL_ACTS
    res = _acts.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=True)
    assert all('g%d.grad_dw' % i in res for i in range(8))
    _acts.check_cell(o, m, x, r, e, [7], need_wgrad=True)            # a sampled 7 x 7 candidate with SE


def _run(m, x, r, e, idxs, route):
    from tfnas_amd import functions as F
    from tfnas_amd.functions import MixedOpFn
    F.adopt_modes(m, F.HipModes(route=route))
    plan = m._plan(tuple(idxs))
    ps = plan.params()
    for p in ps:
        p.requires_grad_(True)
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = torch.softmax(-e.log(), 0).cuda().requires_grad_(True) if len(idxs) > 1 else None
    out = MixedOpFn.apply(plan, xm, w, *ps)
    (out * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = [out.detach().clone(), xm.grad.clone()] + [p.grad.clone() for p in ps] + ([w.grad.clone()] if w is not None else [])
    for p in ps:
        p.grad = None
    return got


@pytest.mark.parametrize('idxs', [(SE_IDX,), tuple(range(8))], ids=['sampled', 'soft'])
@pytest.mark.parametrize('cfg', [_BY_NAME['s2_odd'], _BY_NAME['s1_res_two_column_tiles']], ids=lambda c: c[0])
@pytest.mark.parametrize('act', _acts.NEW_ACTS)
def test_route_word_cannot_move_a_new_activation_cell(act, cfg, idxs):
    """TFNAS_ROUTE_DW_*: a cell with a new activation runs the tile kernels whatever the route asks -- every value gives the bits
    of the default route (on these shapes a ReLU / Swish cell takes the register-window kernels at stride 2 and the ring kernels
    at 22 columns); nor is the weight gradient ever fused into the backward-data pass"""
    from tfnas_amd import functions as F
    o, m, x, r, e = _inputs(cfg, act)
    base = _run(m, x, r, e, idxs, F.route_bits())
    for kw in (dict(dw='direct'), dict(dw='lds'), dict(dw='tiled'), dict(dwwg=False), dict(dwwg2=False), dict(fx=False)):
        got = _run(m, x, r, e, idxs, F.route_bits(**kw))
        assert len(got) == len(base)
        for i, (a, b) in enumerate(zip(got, base)):
            assert torch.equal(a, b), (kw, i)


# ------------------------------------------------------------------------------------------------ a stage
def _stage_pair(act='h-swish'):
    """a three-cell stage (24 -> 40 at stride 2, then two residual cells) at 2 x 24 x 9 x 13 on both sides"""
    from collections import OrderedDict
    from tfnas_amd.model_search import MixedStage
    ics, ocs, ss = [24, 40, 40], [40, 40, 40], [2, 1, 1]
    mids = [[36, 72, 40, 60, 33, 66, 44, 71], [53, 107, 44, 88, 61, 96, 48, 79], [50, 100, 47, 90, 64, 99, 52, 81]]
    mcd = OrderedDict(('block%d' % (b + 1), OrderedDict((i, m) for i, m in enumerate(ms))) for b, ms in enumerate(mids))
    lut = _acts._AnyLut(mids[0])
    for b, ms in enumerate(mids):              # one table for all three cells: {key: {mid: latency}} of every candidate
        for i, mid in enumerate(ms):
            size = 13 if b == 0 else 7
            key = 'MBInvertedResBlock_{}_{}_{}_{}_k{}_s{}_{}'.format(size, ics[b], ics[b] * orc.OP_SE_MULT[i], ocs[b],
                                                                    orc.OP_KERNEL[i], ss[b], act)
            dict.setdefault(lut, key, {})[mid] = 0.2 + 0.07 * i + 0.31 * b
    torch.manual_seed(11)
    o = orc.MixedStage(ics, ocs, ss, act, mcd, lut)
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() == 1 and p.numel() > 8:
                p.copy_(torch.randn(p.shape) * 0.1)
        for blk in o.blocks():
            blk.log_alphas.copy_(torch.log_softmax(torch.randn(8) * 0.5, -1))
        o.betas.copy_(torch.randn(o.betas.shape) * 0.4)
    m = MixedStage(ics, ocs, ss, [False] * 3, [act] * 3, mcd, lut, 2)
    m.load_state_dict(o.state_dict())
    for bo, bm in zip(o.blocks(), m.blocks()):
        bo.set_temperature(2.5)
        bm.set_temperature(2.5)
    g = torch.Generator().manual_seed(5)
    x = _acts.spiked_input((2, 24, 9, 13), g)
    r = torch.randn(2, 40, 5, 7, generator=g)
    e = torch.empty(3, 8).exponential_(generator=g)
    return o, m.cuda(), x, r, e


def _close(a, b, what):
    err, ref = float((a.detach().cpu() - b.detach()).abs().max()), float(b.detach().abs().max())
    assert err <= 2e-5 + 1e-4 * ref, (what, err, ref)


def test_mixed_stage_soft_matches_oracle_stage():
    """MixedStage('h-swish').forward(x, False, None): output, stage latency, dx, d betas, d log_alphas against the oracle's stage"""
    o, m, x, r, e = _stage_pair()
    xo = x.clone().requires_grad_(True)
    with _acts.wrapped_oracle():
        out_o, lat_o = o(xo, False, None, exp_noise=e)
        ((out_o * r).sum() + 3.0 * lat_o).backward()
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out_m, lat_m = m(xm, False, None, exp_noise=e.cuda())
    ((out_m * r.cuda()).sum() + 3.0 * lat_m).backward()
    _close(out_m, out_o, 'out')
    assert abs(float(lat_m.detach()) - float(lat_o.detach())) < 1e-5
    _close(xm.grad, xo.grad, 'dx')
    _close(m.betas.grad, o.betas.grad, 'dbetas')
    for b, (bo, bm) in enumerate(zip(o.blocks(), m.blocks())):
        _close(bm.log_alphas.grad, bo.log_alphas.grad, 'dalpha%d' % b)
        for (k, po), (_, pm) in zip(bo.named_parameters(), bm.named_parameters()):
            if k != 'log_alphas':
                _close(pm.grad, po.grad, 'block%d.%s' % (b, k))


def test_mixed_stage_gumbel_sampling_matches_oracle_stage():
    """MixedStage('h-swish').forward(x, True, 'gumbel'): the same candidates are drawn, output and every gradient agree"""
    o, m, x, r, e = _stage_pair()
    xo = x.clone().requires_grad_(True)
    with _acts.wrapped_oracle():
        out_o, _ = o(xo, True, 'gumbel', exp_noise=e)
        (out_o * r).sum().backward()
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out_m, _ = m(xm, True, 'gumbel', exp_noise=e.cuda())
    (out_m * r.cuda()).sum().backward()
    assert [b.last_idx for b in m.blocks()] == [b.last_idx for b in o.blocks()]
    _close(out_m, out_o, 'out')
    _close(xm.grad, xo.grad, 'dx')
    _close(m.betas.grad, o.betas.grad, 'dbetas')
    for b, (bo, bm) in enumerate(zip(o.blocks(), m.blocks())):
        i = bo.last_idx
        for (k, po), (_, pm) in zip(bo.m_ops[i].named_parameters(), bm.m_ops[i].named_parameters()):
            _close(pm.grad, po.grad, 'block%d.op%d.%s' % (b, i, k))


class _OneStage(torch.nn.Module):
    """what path.PathRunner needs of a model: cells(), stages(), parameters()"""

    def __init__(self, stage):
        super().__init__()
        self.stage = stage

    def cells(self):
        return self.stage.blocks()

    def stages(self):
        return [self.stage]


def test_path_level_runs_the_planned_hswish_cells():
    """the path level (tfnas_path_plan / tfnas_paths_fwd / _bwd over planned cells: path.PathRunner) with frozen weights, soft and
    sampled, against the oracle's stage"""
    from tfnas_amd.path import PathRunner
    o, m, x, r, e = _stage_pair()
    for p in m.parameters():
        p.requires_grad_(False)
    m.betas.requires_grad_(True)
    runner = PathRunner(_OneStage(m))
    try:
        with _acts.wrapped_oracle():
            xo = x.clone().requires_grad_(True)
            out_o, lat_o = o(xo, False, None, exp_noise=e)
            ((out_o * r).sum() + 3.0 * lat_o).backward()
            dbetas_o = o.betas.grad.clone()
            xs = x.clone().requires_grad_(True)
            idxs = [5, 1, 6]
            outs = [xs]
            for blk, i in zip(o.blocks(), idxs):
                outs.append(blk.m_ops[i](outs[-1]))
            wb = torch.softmax(o.betas.detach(), -1)
            samp_o = sum(w * t for w, t in zip(wb, outs[o.start_res:]))
            (samp_o * r).sum().backward()
        W = torch.stack([orc.gumbel_softmax(b.log_alphas.detach(), b.T, e[i]) for i, b in enumerate(o.blocks())]).cuda()
        CL = torch.stack([(W[i].cpu() * torch.tensor(b.get_lookup_latency(13 if i == 0 else 7))).sum()
                          for i, b in enumerate(o.blocks())]).float().cuda()
        xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        out_m, lat_m = runner.soft(xm, W, CL)
        ((out_m * r.cuda()).sum() + 3.0 * lat_m.sum()).backward()
        _close(out_m, out_o, 'soft out')
        assert abs(float(lat_m.detach().sum()) - float(lat_o.detach())) < 1e-5
        _close(xm.grad, xo.grad, 'soft dx')
        _close(m.betas.grad, dbetas_o, 'soft dbetas')
        xm2 = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        samp_m = runner.sampled(xm2, idxs)
        (samp_m * r.cuda()).sum().backward()
        _close(samp_m, samp_o, 'sampled out')
        _close(xm2.grad, xs.grad, 'sampled dx')
        torch.cuda.synchronize()
    finally:
        runner.close()
