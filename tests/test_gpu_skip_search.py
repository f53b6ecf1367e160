"""The search steps on a supernet whose residual cells of stages 2-5 end in a skip (identity) candidate
(model_search.Network(primitives=...) with NAMES[:7] + ['skip'] there and the default set elsewhere): one bi-sampling weight step and
one architecture step of tfnas_amd.search, each from identical state, against the oracle's w_step / a_step on an oracle Network
whose m_ops entries of those cells were replaced by the restatement blocks of tests/_kinds.py / tests/_fused.py and, in slot 7,
the identity module of tests/_skip.py; then the sampled MixedOP, and parse_searched_model -> NetworkCfg on an architecture whose
argmax picks a skip.

32 x 32 images, batch 4, as tests/test_gpu_kinds_search.py; gates: that file's (logits 1e-3, expected latency 1e-3, post-step arch
parameters 1e-3, loss 2e-3; weights: atol 2e-5 + rtol 1e-3 * max|ref|).  The noise and rand_pos of the weight step are made on the
CPU so that the ORACLE samples the skip on each path in at least one cell (asserted on the oracle's own indices)."""
import copy
import math

import pytest
import torch

import _fused
import _skip
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

NAMES = ['MBI_k3_e3', 'FMB_k3_e6', 'DS_k5', 'MBI_k7_e6', 'FMB_k3_e3_se', 'DS_k3_se', 'MBI_k5_e3_se', 'skip']
SKIP_STAGES = ('stage2', 'stage3', 'stage4', 'stage5')


def _skip_cells():
    from tfnas_amd import geometry
    return [(st, b) for st, b in geometry.residual_cells() if st in SKIP_STAGES]


def _primitives():
    prim = {}
    for st, b in _skip_cells():
        prim.setdefault(st, {})[b] = list(NAMES)
    return prim


def _lut():
    lut = _skip.SkipLut()
    lut['base'] = 1.5
    return lut


def _pair(seed=2, T=5.0):
    """(oracle Network with restatement blocks and an identity module in the skip cells, product Network(primitives=...)) with
    identical weights"""
    from tfnas_amd import Network, geometry
    mc = geometry.initial_mc_num_dddict()
    torch.manual_seed(seed)
    o = orc.Network(100, orc.initial_mc_num_dddict(), _lut())
    gen = torch.Generator().manual_seed(seed + 1)
    cells = set(_skip_cells())
    for st, b, ic, oc, s, act, size in geometry.iter_cells():
        if (st, b) not in cells:
            continue
        cell = getattr(getattr(o, st), b)
        for i, name in enumerate(NAMES):
            layer, mid, se, k = geometry.primitive_block(name, ic, mc[st][b][i])
            if layer == 'IdentityLayer':
                cell.m_ops[i] = _skip.IdentityRef(ic, oc)
                continue
            if layer == 'FusedMBConvBlock':
                blk = _fused.FusedRef(ic, mid, se, oc, s, act)
                blk.name = layer
            else:
                blk = orc.MBConv(ic, mid, se, oc, k, s, act)
            with torch.no_grad():
                for p in blk.parameters():
                    if p.dim() == 1:
                        p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            cell.m_ops[i] = blk
    m = Network(100, mc, _lut(), primitives=_primitives())
    assert list(o.state_dict()) == list(m.state_dict())
    m.load_state_dict(o.state_dict())
    o.set_temperature(T)
    m.set_temperature(T)
    return o, m.cuda()


def _cell_index():
    from tfnas_amd import geometry
    return {(st, b): i for i, (st, b, *_) in enumerate(geometry.iter_cells())}


def test_w_step_against_the_oracle_with_a_skip_on_each_path():
    from tfnas_amd import search
    o, m = _pair()
    assert not m.plain_candidates() and not m._use_paths(torch.zeros(1).cuda())
    idx = _cell_index()
    skip_ci = [idx[c] for c in _skip_cells()]
    assert len(skip_ci) == 11 and all(m.cells()[ci].m_ops[7].name == 'IdentityLayer' for ci in skip_ci)
    assert sum(c.m_ops[7].name == 'IdentityLayer' for c in m.cells()) == 11
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert st.runner is None                                       # the per-cell route in every step
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 100, (4,), generator=g)
    ng = torch.empty(18, 8).exponential_(generator=g)
    rp = [int(v) for v in torch.randint(0, 7, (18,), generator=g)]
    # the gumbel path takes the skip in two cells (a tiny Exp(1) draw is a huge Gumbel one), the random path in two others (the
    # last of the seven candidates the gumbel path left)
    for ci in (skip_ci[0], skip_ci[5]):
        ng[ci, 7] = 1e-6
    for ci in (skip_ci[2], skip_ci[7]):
        ng[ci, 7] = 50.0
        rp[ci] = 6
    before = {k: v.detach().clone() for k, v in o.named_parameters()}
    lo, logits_o, gi, ri = orc.w_step(o, x, y, oo[0], 5.0, noise_g=ng, rand_pos=rp)
    assert [ci for ci in range(18) if gi[ci] == 7] and [ci for ci in range(18) if ri[ci] == 7]      # the ORACLE sampled a skip on each path
    assert gi[skip_ci[0]] == 7 and gi[skip_ci[5]] == 7 and ri[skip_ci[2]] == 7 and ri[skip_ci[7]] == 7
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


def test_a_step_loss_latency_and_the_alphas_of_the_skip_slots():
    from tfnas_amd import search
    o, m = _pair()
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 100, (4,), generator=g)
    na = torch.empty(18, 8).exponential_(generator=g)
    before = [c.log_alphas.detach().cpu().clone() for c in m.cells()]
    la_o, ll_o, lat_o, g_o = orc.a_step(o, x, y, oo[1], 15.0, 0.1, 5.0, noise=na)
    la_m, ll_m, lat_m, g_m = search.a_step(st, x.cuda(), y.cuda(), mo[1], 15.0, 0.1, 5.0, noise=na.cuda(), return_grads=True)
    torch.cuda.synchronize()
    print('a_step loss', float(la_o), float(la_m), 'lat', float(lat_o), float(lat_m))
    assert abs(float(lat_o) - float(lat_m)) < 1e-3 and abs(float(la_o) - float(la_m)) < 2e-3
    assert abs(float(ll_o) - float(ll_m)) < 1e-3
    for a, b in zip(o.arch_parameters(), m.arch_parameters()):
        assert torch.allclose(b.detach().cpu(), a.detach(), atol=1e-3), float((b.detach().cpu() - a.detach()).abs().max())
    # the skip slots: a gradient arrived, the step moved them, and they moved as the oracle's did
    idx = _cell_index()
    names = [k for k, _ in o.named_parameters() if k.endswith('log_alphas') or k.endswith('betas')]
    for stg, b in _skip_cells():
        ci = idx[(stg, b)]
        k = names.index('%s.%s.log_alphas' % (stg, b))
        assert float(g_m[k][7].abs()) > 0 and float(g_o[k][7].abs()) > 0
        a_o = getattr(getattr(o, stg), b).log_alphas.detach()[7]
        a_m = m.cells()[ci].log_alphas.detach().cpu()[7]
        assert float(a_m) != float(before[ci][7]) and abs(float(a_m) - float(a_o)) < 1e-3


def test_sampled_skip_returns_its_input_tensor_itself():
    _, m = _pair()
    cell = m.stage3.block2
    x = torch.randn(4, 80, 2, 2, device='cuda')
    cell._pre = 7
    y, lat = cell(x, True, 'random')
    assert y is x and lat == 0 and cell.last_idx == 7
    with torch.no_grad():
        cell.log_alphas[7] += 9.0
    y, lat = cell(x, True, 'max_alphas')
    assert y is x and lat == 0


def test_interleaved_bisample_sweep_equals_the_two_sequential_forwards():
    """Network.forward_bisample with a skip sampled on each path: the same kernels on the same inputs as forward(gumbel, pos=)
    followed by forward(random, rand_pos=) -- bit-identical logits"""
    _, m = _pair()
    idx = _cell_index()
    skip_ci = [idx[c] for c in _skip_cells()]
    pos_g = [ci % 7 for ci in range(18)]
    rp = [(3 * ci) % 7 for ci in range(18)]
    pos_g[skip_ci[1]] = 7
    rp[skip_ci[4]] = 6                                             # (pos_g there is < 7: the last of the seven left is the skip)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(9)).cuda()
    side = torch.cuda.Stream()
    with torch.no_grad():
        la, lb = m.forward_bisample(x, pos_g, rp, side)
        torch.cuda.synchronize()
        assert m.cells()[skip_ci[4]].last_idx == 7
        m.reset_switches()
        ya, _ = m(x, True, 'gumbel', pos=pos_g)
        assert m.cells()[skip_ci[1]].last_idx == 7
        yb, _ = m(x, True, 'random', rand_pos=rp)
        torch.cuda.synchronize()
    assert torch.equal(la, ya) and torch.equal(lb, yb)


def test_parsed_architecture_with_a_skip_exports_and_trains_like_the_net_without_the_block():
    from tfnas_amd import model_eval as me, parsing
    _, m = _pair()
    picked = [('stage2', 'block2'), ('stage3', 'block3'), ('stage5', 'block2')]
    with torch.no_grad():
        for stg, b in picked:
            getattr(getattr(m, stg), b).log_alphas[7] += 3.0
        for stg in m.stages():                                     # every depth: the deepest output of each stage
            stg.betas[-1] += 3.0
    res = parsing.parse_searched_model(m, lat_lookup=_lut(), num_classes=20)
    parsed, cfg = res['parsed_arch'], res['config']
    assert all(parsed[stg][b] == 7 for stg, b in picked)
    ids = [(stg, i) for stg in SKIP_STAGES for i, c in enumerate(cfg[stg]) if c['name'] == 'IdentityLayer']
    assert len(ids) == 3
    bare = copy.deepcopy(cfg)
    for stg in SKIP_STAGES:
        bare[stg] = [c for c in bare[stg] if c['name'] != 'IdentityLayer']
    assert res['macs_M'] == parsing.count_macs_in_M(bare) and res['params_MB'] == parsing.count_params_in_MB(bare)
    torch.manual_seed(3)
    net = me.NetworkCfg(20, cfg, _lut(), 0.0, 0.0).cuda()
    twin = me.NetworkCfg(20, bare, _lut(), 0.0, 0.0).cuda()
    assert net.config == cfg and net.block_count == twin.block_count + 3
    # the same weights: the state_dict keys of the blocks behind a skip are shifted by one stage index
    src = [p for p in net.parameters()] + [b for b in net.buffers()]
    dst = [p for p in twin.parameters()] + [b for b in twin.buffers()]
    assert len(src) == len(dst)
    with torch.no_grad():
        for a, b in zip(src, dst):
            assert a.shape == b.shape
            b.copy_(a)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 32, 32, generator=gen).cuda()
    y = torch.randint(0, 20, (4,), generator=gen).cuda()
    assert float(net.get_lookup_latency(x)) == float(twin.get_lookup_latency(x))
    net.eval()
    twin.eval()
    with torch.no_grad():
        assert torch.equal(net(x), twin(x))                        # eval-mode logits: bit-identical
    net.train()
    twin.train()
    outs = []
    for n in (net, twin):
        opt = torch.optim.SGD(n.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
        loss, logits = me.train_step(n, x, y, me.CrossEntropyLabelSmooth(20, 0.1), opt, 5.0)
        torch.cuda.synchronize()
        assert math.isfinite(float(loss))
        outs.append((loss, logits))
    assert torch.equal(outs[0][1], outs[1][1])
    for a, b in zip(net.parameters(), twin.parameters()):
        assert torch.equal(a, b)                                   # one train_step (drop_connect_rate = 0): identical weights
