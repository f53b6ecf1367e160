"""The search steps on supernets with dilated candidates (model_search.Network(primitives=...) with names of DILATED_OPS): one
bi-sampling weight step (injected noise and rand_pos) and one architecture step of tfnas_amd.search, each from identical state,
against the oracle's w_step / a_step driving an oracle Network whose m_ops entries were replaced by the restatement blocks of
tests/_dil.py with the same weights; then parse_searched_model -> derived_config -> NetworkCfg.

4 x 3 x 32 x 32 batches, as tests/test_gpu_kinds_search.py.  A network whose dilated candidates are all MBI_* is
plain_candidates(): it takes the path level, the weight arena and the fused optimizer tails (st.runner is not None), and the same
two steps with search.USE_PATHS off are bit-identical.  A network with a DS_k3d2 candidate takes the per-cell route.  Gates: those
tests/test_gpu_kinds_search.py applies to the same quantities (logits 1e-3, expected latency 1e-3, post-step arch parameters
1e-3, loss 2e-3; weights: atol 2e-5 + rtol 1e-3 * max|ref|)."""
import math

import pytest
import torch

import _dil
import _kinds
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

# the four MBI_k?d2 names beside their undilated twins, in every cell (SE on the last four, widths from the default tables)
MBI = ['MBI_k3d2_e3', 'MBI_k3_e6', 'MBI_k5d2_e3', 'MBI_k5_e6', 'MBI_k3_e3_se', 'MBI_k3d2_e6_se', 'MBI_k5_e3_se', 'MBI_k5d2_e6_se']
# ... and a cell list with an expand-free dilated candidate, for the cells of stage 3
DS = ['MBI_k3_e3', 'MBI_k3d2_e6', 'DS_k3d2', 'MBI_k5_e6', 'MBI_k3_e3_se', 'MBI_k3_e6_se', 'DS_k5d2_se', 'MBI_k5d2_e6_se']


def _primitives(which):
    from tfnas_amd import geometry
    if which == 'mbi':
        return list(MBI)
    return {'stage3': {b: list(DS) for st, b, *_ in geometry.iter_cells() if st == 'stage3'}}


def _lut():
    lut = _kinds.AnyLut()
    lut['base'] = 1.5
    return lut


def _pair(which, seed=2, T=5.0):
    """(oracle Network with the restatement's dilated blocks, product Network(primitives=...)) with identical weights"""
    from tfnas_amd import Network, geometry
    mc = geometry.initial_mc_num_dddict()
    prims = _primitives(which)
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
            d = geometry.primitive_dilation(name)
            blk = orc.MBConv(ic, mid, se, oc, k, s, act)
            with torch.no_grad():
                for p in blk.parameters():
                    if p.dim() == 1:
                        p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            if d != 1:
                _dil.dilate(blk, d)
                blk.kernel_size = _dil.KTag(k, d)          # (the oracle's latency key of this block says 'k3d2' / 'k5d2')
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


def _w_step_against_oracle(which, paths):
    from tfnas_amd import search
    o, m = _pair(which)
    assert m.plain_candidates() == paths
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert (st.runner is not None) == paths
    x, y, ng, rp, _ = _batch()
    before = {k: v.detach().clone() for k, v in o.named_parameters()}
    lo, logits_o, gi, ri = orc.w_step(o, x, y, oo[0], 5.0, noise_g=ng, rand_pos=rp)
    lm, logits_m = search.w_step(st, x.cuda(), y.cuda(), mo[0], 5.0, noise_g=ng.cuda(), rand_pos=rp)
    torch.cuda.synchronize()
    dils = [[b.dilation for b in c.m_ops] for c in m.cells()]
    assert 2 in {dils[c][i] for c, i in enumerate(gi)} | {dils[c][i] for c, i in enumerate(ri)}      # dilated candidates were sampled
    print('w_step loss', float(lo), float(lm), 'logits', float((logits_m.cpu() - logits_o).abs().max()))
    assert abs(float(lo) - float(lm)) < 2e-3
    assert torch.allclose(logits_m.cpu(), logits_o, atol=1e-3, rtol=1e-3)
    touched = 0
    for (k, a), (k2, b) in zip(o.named_parameters(), m.named_parameters()):
        assert k == k2
        err, ref = float((b.detach().cpu() - a.detach()).abs().max()), float(a.detach().abs().max())
        assert err <= 2e-5 + 1e-3 * ref, (k, err, ref)
        touched += int(not torch.equal(a.detach(), before[k]))
    assert touched > 60


def _a_step_against_oracle(which, paths):
    from tfnas_amd import search
    o, m = _pair(which)
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert (st.runner is not None) == paths
    x, y, _, _, na = _batch()
    la_o, ll_o, lat_o, g_o = orc.a_step(o, x, y, oo[1], 15.0, 0.1, 5.0, noise=na)
    la_m, ll_m, lat_m, g_m = search.a_step(st, x.cuda(), y.cuda(), mo[1], 15.0, 0.1, 5.0, noise=na.cuda(), return_grads=True)
    torch.cuda.synchronize()
    print('a_step loss', float(la_o), float(la_m), 'lat', float(lat_o), float(lat_m))
    assert abs(float(lat_o) - float(lat_m)) < 1e-3 and abs(float(la_o) - float(la_m)) < 2e-3
    assert abs(float(ll_o) - float(ll_m)) < 1e-3
    for a, b in zip(o.arch_parameters(), m.arch_parameters()):
        assert torch.allclose(b.detach().cpu(), a.detach(), atol=1e-3), float((b.detach().cpu() - a.detach()).abs().max())


def test_w_step_of_dilated_mbi_candidates_on_the_path_level():
    _w_step_against_oracle('mbi', True)


def test_a_step_of_dilated_mbi_candidates_on_the_path_level():
    _a_step_against_oracle('mbi', True)


def test_w_step_with_a_dilated_ds_candidate_on_the_per_cell_route():
    _w_step_against_oracle('ds', False)


def test_a_step_with_a_dilated_ds_candidate_on_the_per_cell_route():
    _a_step_against_oracle('ds', False)


def _two_steps(use_paths):
    from tfnas_amd import search
    old = search.USE_PATHS, search.FUSED_OPT, search.FUSED_TAIL
    search.USE_PATHS = use_paths
    search.FUSED_OPT = search.FUSED_TAIL = False       # (the same torch.optim / classifier tail on both sides: tests/test_gpu_paths.py)
    try:
        _, m = _pair('mbi')
        st = search.SearchState(m)
        assert (st.runner is not None) == use_paths
        ow, oa = search.make_optimizers(m)
        x, y, ng, rp, na = _batch()
        lw, _ = search.w_step(st, x.cuda(), y.cuda(), ow, 5.0, noise_g=ng.cuda(), rand_pos=rp)
        la, ll, lat, g = search.a_step(st, x.cuda(), y.cuda(), oa, 15.0, 0.1, 5.0, noise=na.cuda(), return_grads=True)
        torch.cuda.synchronize()
        return float(lw), float(la), float(lat), [t.clone() for t in g], {k: p.detach().clone() for k, p in m.named_parameters()}
    finally:
        search.USE_PATHS, search.FUSED_OPT, search.FUSED_TAIL = old


def test_path_level_steps_are_bit_identical_to_the_per_cell_route():
    lw_a, la_a, lat_a, g_a, p_a = _two_steps(True)
    lw_b, la_b, lat_b, g_b, p_b = _two_steps(False)
    assert lw_a == lw_b and la_a == la_b
    assert abs(lat_a - lat_b) < 1e-5                       # (the six stage latencies are summed in a different order)
    for a, b in zip(g_a, g_b):
        assert torch.equal(a, b)
    for k in p_a:
        assert torch.equal(p_a[k], p_b[k]), k


@pytest.mark.parametrize('which', ['mbi', 'ds'])
def test_exported_config_round_trip(which):
    """parse_searched_model of the model itself (no primitives argument: it exports what its cells hold) -> a config whose dilated
    choices carry 'dilation': 2 and nothing else does -> NetworkCfg builds the twin of model_eval.Network and trains one step"""
    from tfnas_amd import geometry, model_eval as me, parsing
    _, m = _pair(which)
    names = MBI if which == 'mbi' else DS
    with torch.no_grad():                                          # make dilated candidates win somewhere, undilated ones elsewhere
        for ci, c in enumerate(m.cells()):
            c.log_alphas[2 if which == 'ds' else (0, 1, 2, 7, 6)[ci % 5]] += 3.0          # ('ds': DS_k3d2 wins in stage 3)
    out = parsing.parse_searched_model(m, num_classes=20)
    cfg, parsed = out['config'], out['parsed_arch']
    assert cfg == parsing.derived_config(parsed, m.mc_num_dddict, 20, primitives=_primitives(which))
    want = [geometry.primitive_dilation(geometry.cell_primitives(_primitives(which), st, b)[op])
            for st in parsed for b, op in parsed[st].items()]
    got = [c.get('dilation', 1) for st in parsed for c in cfg[st]]
    assert got == want and 2 in got and 1 in got
    assert all(('dilation' in c) == (c.get('dilation') == 2) for st in parsed for c in cfg[st])
    if which == 'ds':
        assert any(c.get('dilation') == 2 and c['mid_channels'] == c['in_channels'] for c in cfg['stage3']), names
    net = me.NetworkCfg(20, cfg, None, 0.0, 0.0).cuda()
    twin = me.Network(20, parsed, m.mc_num_dddict, primitives=_primitives(which))
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
