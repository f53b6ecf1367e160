"""The search steps on supernets with MixConv candidates (model_search.Network(primitives=...) with names of MIX_OPS): one
bi-sampling weight step (injected noise and rand_pos) and one architecture step of tfnas_amd.search, each from identical state,
against the oracle's w_step / a_step driving an oracle Network whose m_ops entries were replaced by the restatement blocks of
tests/_mix.py with the same weights; then parse_searched_model -> derived_config -> NetworkCfg.

4 x 3 x 32 x 32 batches, as tests/test_gpu_dil_search.py.  A network with a MixConv candidate is not plain_candidates(): it takes
the per-cell route (st.runner is None).  Gates: those tests/test_gpu_dil_search.py applies to the same quantities (logits 1e-3,
expected latency 1e-3, post-step arch parameters 1e-3, loss 2e-3; weights: atol 2e-5 + rtol 1e-3 * max|ref|)."""
import math

import pytest
import torch

import _kinds
import _mix
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

# MBI_k35_* and MBI_k357_* beside their plain twins, in every cell (SE on the last four, widths from the default tables)
MBI = ['MBI_k35_e3', 'MBI_k3_e6', 'MBI_k357_e3', 'MBI_k5_e6', 'MBI_k3_e3_se', 'MBI_k35_e6_se', 'MBI_k5_e3_se', 'MBI_k357_e6_se']
# ... and a cell list with expand-free MixConv candidates, for the cells of stage 3
DS = ['MBI_k3_e3', 'MBI_k35_e6', 'DS_k35', 'MBI_k5_e6', 'MBI_k3_e3_se', 'MBI_k3_e6_se', 'DS_k357_se', 'MBI_k357_e6_se']


def _primitives():
    from tfnas_amd import geometry
    prims = {}
    for st, b, *_ in geometry.iter_cells():
        prims.setdefault(st, {})[b] = list(DS if st == 'stage3' else MBI)
    return prims


def _lut():
    lut = _kinds.AnyLut()
    lut['base'] = 1.5
    return lut


def _pair(seed=2, T=5.0):
    """(oracle Network with the restatement's MixConv blocks, product Network(primitives=...)) with identical weights"""
    from tfnas_amd import Network, geometry
    mc = geometry.initial_mc_num_dddict()
    prims = _primitives()
    torch.manual_seed(seed)
    o = orc.Network(100, orc.initial_mc_num_dddict(), _lut())
    gen = torch.Generator().manual_seed(seed + 1)
    for st, b, ic, oc, s, act, size in geometry.iter_cells():
        names = geometry.cell_primitives(prims, st, b)
        cell = getattr(getattr(o, st), b)
        for i, name in enumerate(names):
            if name == geometry.PRIMITIVES[i]:
                continue
            layer, mid, se, k = geometry.primitive_block(name, ic, mc[st][b][i])
            ks = geometry.primitive_mix_kernels(name)
            blk = orc.MBConv(ic, mid, se, oc, k, s, act)
            if ks is not None:
                _mix.mixify(blk, ks)
                blk.kernel_size = _mix.KTag(ks)            # (the oracle's latency key of this block says 'k35' / 'k357')
            with torch.no_grad():
                for n, p in blk.named_parameters():
                    if p.dim() == 1 and 'depth_conv' not in n:
                        p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            cell.m_ops[i] = blk
    m = Network(100, mc, _lut(), primitives=prims)
    assert list(o.state_dict()) == list(m.state_dict())
    m.load_state_dict(o.state_dict())
    o.set_temperature(T)
    m.set_temperature(T)
    return o, m.cuda()


def _batch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 100, (4,), generator=g)
    ng = torch.empty(18, 8).exponential_(generator=g)
    rp = [int(v) for v in torch.randint(0, 7, (18,), generator=g)]
    na = torch.empty(18, 8).exponential_(generator=g)
    return x, y, ng, rp, na


def test_w_step_with_mixconv_candidates_on_the_per_cell_route():
    from tfnas_amd import search
    o, m = _pair()
    assert not m.plain_candidates()
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert st.runner is None
    x, y, ng, rp, _ = _batch()
    before = {k: v.detach().clone() for k, v in o.named_parameters()}
    lo, logits_o, gi, ri = orc.w_step(o, x, y, oo[0], 5.0, noise_g=ng, rand_pos=rp)
    lm, logits_m = search.w_step(st, x.cuda(), y.cuda(), mo[0], 5.0, noise_g=ng.cuda(), rand_pos=rp)
    torch.cuda.synchronize()
    mixes = [[b.mix_kernels for b in c.m_ops] for c in m.cells()]
    sampled = {mixes[c][i] for c, i in enumerate(gi)} | {mixes[c][i] for c, i in enumerate(ri)}
    assert (3, 5) in sampled and (3, 5, 7) in sampled and None in sampled                  # MixConv candidates were sampled
    print('w_step loss', float(lo), float(lm), 'logits', float((logits_m.cpu() - logits_o).abs().max()))
    assert abs(float(lo) - float(lm)) < 2e-3
    assert torch.allclose(logits_m.cpu(), logits_o, atol=1e-3, rtol=1e-3)
    touched = packed = 0
    for (k, a), (k2, b) in zip(o.named_parameters(), m.named_parameters()):
        assert k == k2
        err, ref = float((b.detach().cpu() - a.detach()).abs().max()), float(a.detach().abs().max())
        assert err <= 2e-5 + 1e-3 * ref, (k, err, ref)
        moved = not torch.equal(a.detach(), before[k])
        touched += int(moved)
        packed += int(moved and a.dim() == 1 and k.endswith('depth_conv.conv.weight'))
    assert touched > 60 and packed > 0                     # (packed depthwise weights took the step too)


def test_a_step_with_mixconv_candidates_on_the_per_cell_route():
    from tfnas_amd import search
    o, m = _pair()
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert st.runner is None
    x, y, _, _, na = _batch()
    la_o, ll_o, lat_o, g_o = orc.a_step(o, x, y, oo[1], 15.0, 0.1, 5.0, noise=na)
    la_m, ll_m, lat_m, g_m = search.a_step(st, x.cuda(), y.cuda(), mo[1], 15.0, 0.1, 5.0, noise=na.cuda(), return_grads=True)
    torch.cuda.synchronize()
    print('a_step loss', float(la_o), float(la_m), 'lat', float(lat_o), float(lat_m))
    assert abs(float(lat_o) - float(lat_m)) < 1e-3 and abs(float(la_o) - float(la_m)) < 2e-3
    assert abs(float(ll_o) - float(ll_m)) < 1e-3
    for a, b in zip(o.arch_parameters(), m.arch_parameters()):
        assert torch.allclose(b.detach().cpu(), a.detach(), atol=1e-3), float((b.detach().cpu() - a.detach()).abs().max())


def test_exported_config_round_trip():
    """parse_searched_model of the model itself (no primitives argument: it exports what its cells hold) -> a config whose MixConv
    choices carry 'mix_kernels' and nothing else does -> NetworkCfg builds the twin of model_eval.Network and trains one step"""
    from tfnas_amd import geometry, model_eval as me, parsing
    _, m = _pair()
    with torch.no_grad():                                          # make MixConv candidates win somewhere, plain ones elsewhere
        for ci, c in enumerate(m.cells()):
            c.log_alphas[(0, 1, 2, 7, 5, 2, 6, 1)[ci % 8]] += 3.0  # (stage 3, cells 5-8: DS_k35 and DS_k357_se win in its first two)
    out = parsing.parse_searched_model(m, num_classes=20)
    cfg, parsed = out['config'], out['parsed_arch']
    prims = _primitives()
    assert cfg == parsing.derived_config(parsed, m.mc_num_dddict, 20, primitives=prims)
    want = [geometry.primitive_mix_kernels(geometry.cell_primitives(prims, st, b)[op]) for st in parsed for b, op in parsed[st].items()]
    got = [c.get('mix_kernels') for st in parsed for c in cfg[st]]
    assert got == [None if w is None else list(w) for w in want] and [3, 5] in got and [3, 5, 7] in got and None in got
    assert any(c.get('mix_kernels') and c['mid_channels'] == c['in_channels'] for c in cfg['stage3'])       # an expand-free one
    net = me.NetworkCfg(20, cfg, None, 0.0, 0.0).cuda()
    twin = me.Network(20, parsed, m.mc_num_dddict, primitives=prims)
    assert list(twin.state_dict()) == list(net.state_dict()) and net.config == cfg == twin.config
    before = {k: v.detach().cpu().clone() for k, v in net.named_parameters()}
    opt = torch.optim.SGD(net.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 32, 32, generator=gen).cuda()
    y = torch.randint(0, 20, (4,), generator=gen).cuda()
    loss, logits = me.train_step(net, x, y, me.CrossEntropyLabelSmooth(20, 0.1), opt, 5.0)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and torch.isfinite(logits).all()
    for k, p in net.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach().cpu(), before[k]), k
