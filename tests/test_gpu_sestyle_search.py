"""The search steps and the epoch driver on a supernet with a squeeze-excite style: model_search.Network(se_style=...) with
('relu', 'h-sigmoid') on stages 2-6 and the default primitives.  32 x 32 images, batch 4.  Stage 1 keeps the default style (its
ReLU cells are handled exactly as tests/test_gpu_network.py / test_gpu_kinds_search.py handle them).

One bi-sampling weight step (injected noise and rand_pos) and one architecture step of tfnas_amd.search, each from identical state,
against the oracle's w_step / a_step over an oracle Network whose blocks of stages 2-6 were restyled by tests/_sestyle.py.  Gates:
those of tests/test_gpu_kinds_search.py (logits 1e-3, loss 2e-3, latency 1e-3, post-step arch parameters 1e-3, weights atol 2e-5 +
rtol 1e-3 * max|ref|).  The model takes the path level (asserted); the same two steps with search.USE_PATHS off -- the per-cell
route -- must be bit-identical, as in tests/test_gpu_paths.py.  Then a two-epoch run_search(..., se_style=...): one warm-up and one
architecture epoch at the sizes of tests/test_gpu_epoch.py; the networks it builds carry the style."""
import os

import pytest
import torch

import _kinds
import _sestyle as S
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

STYLED = ('stage2', 'stage3', 'stage4', 'stage5', 'stage6')
STYLE = {st: S.MNV3 for st in STYLED}


def _lut():
    lut = _kinds.AnyLut()
    lut['base'] = 1.5
    return lut


def _pair(seed=2, T=5.0):
    """(oracle Network with the blocks of stages 2-6 restyled, product Network(se_style=...)) with identical weights"""
    from tfnas_amd import Network, geometry
    torch.manual_seed(seed)
    o = orc.Network(100, orc.initial_mc_num_dddict(), _lut())
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in o.named_parameters():
            if 'squeeze_excite' in k and p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    S.restyle_all(o, *S.MNV3, skip=[o.second_stem, o.stage1])
    m = Network(100, geometry.initial_mc_num_dddict(), _lut(), se_style=STYLE)
    assert list(o.state_dict()) == list(m.state_dict())
    m.load_state_dict(o.state_dict())
    o.set_temperature(T)
    m.set_temperature(T)
    return o, m.cuda()


def _data():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 100, (4,), generator=g)
    ng = torch.empty(18, 8).exponential_(generator=g)
    rp = [int(v) for v in torch.randint(0, 7, (18,), generator=g)]
    na = torch.empty(18, 8).exponential_(generator=g)
    return x, y, ng, rp, na


def test_the_pair_is_styled_where_it_should_be():
    o, m = _pair()
    for net in (o, m):
        assert (getattr(net.second_stem, 'se_gate', 'sigmoid'), getattr(net.second_stem, 'se_act', None)) == ('sigmoid', None)
        assert all(getattr(b, 'se_gate', 'sigmoid') == 'sigmoid' for c in net.stage1.blocks() for b in c.m_ops)
        assert all((b.se_act, b.se_gate) == S.MNV3 for st in STYLED for c in getattr(net, st).blocks() for b in c.m_ops)
    assert m.plain_candidates()


def test_w_step_against_the_oracle():
    from tfnas_amd import search
    o, m = _pair()
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert st.runner is not None                                   # the path level is in use
    x, y, ng, rp, _ = _data()
    before = {k: v.detach().clone() for k, v in o.named_parameters()}
    lo, logits_o, gi, ri = orc.w_step(o, x, y, oo[0], 5.0, noise_g=ng, rand_pos=rp)
    lm, logits_m = search.w_step(st, x.cuda(), y.cuda(), mo[0], 5.0, noise_g=ng.cuda(), rand_pos=rp)
    torch.cuda.synchronize()
    assert sum(i >= 4 for i in gi[2:]) + sum(i >= 4 for i in ri[2:]) >= 4            # styled SE candidates were sampled
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
    # the style is what was computed: the unstyled oracle's step from the same state is elsewhere
    u, _ = _pair()
    S.restyle_all(u)
    lu = orc.w_step(u, x, y, orc.make_optimizers(u)[0], 5.0, noise_g=ng, rand_pos=rp)[0]
    assert abs(float(lu) - float(lm)) > 2e-3


def test_a_step_against_the_oracle():
    from tfnas_amd import search
    o, m = _pair()
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert st.runner is not None
    x, y, _, _, na = _data()
    la_o, ll_o, lat_o, _ = orc.a_step(o, x, y, oo[1], 15.0, 0.1, 5.0, noise=na)
    la_m, ll_m, lat_m, _ = search.a_step(st, x.cuda(), y.cuda(), mo[1], 15.0, 0.1, 5.0, noise=na.cuda(), return_grads=True)
    torch.cuda.synchronize()
    print('a_step loss', float(la_o), float(la_m), 'lat', float(lat_o), float(lat_m))
    assert abs(float(lat_o) - float(lat_m)) < 1e-3 and abs(float(la_o) - float(la_m)) < 2e-3
    assert abs(float(ll_o) - float(ll_m)) < 1e-3
    for a, b in zip(o.arch_parameters(), m.arch_parameters()):
        assert torch.allclose(b.detach().cpu(), a.detach(), atol=1e-3), float((b.detach().cpu() - a.detach()).abs().max())


def _two_steps(use_paths):
    from tfnas_amd import search
    old, old_f, old_t = search.USE_PATHS, search.FUSED_OPT, search.FUSED_TAIL
    search.USE_PATHS = use_paths
    search.FUSED_OPT = False               # (the same torch.optim tail and the same stock classifier + cross-entropy on both
    search.FUSED_TAIL = False              #  sides, as in tests/test_gpu_paths.py: this is about the path level)
    try:
        _, m = _pair()
        st = search.SearchState(m)
        assert (st.runner is not None) == use_paths
        ow, oa = search.make_optimizers(m)
        x, y, ng, rp, na = _data()
        search.w_step(st, x.cuda(), y.cuda(), ow, 5.0, noise_g=ng.cuda(), rand_pos=rp)
        _, _, lat, g = search.a_step(st, x.cuda(), y.cuda(), oa, 15.0, 0.1, 5.0, noise=na.cuda(), return_grads=True)
        torch.cuda.synchronize()
        if use_paths:                      # the templates the path level planned carry the style
            styles = {(k[0], t.se_style) for k, t in st.runner._tmpl.items() if any(t.g[g].se for g in range(t.G))}
            assert styles and all(s == (0x11 if ci >= 2 else 0) for ci, s in styles), styles
        return {k: p.detach().clone() for k, p in m.named_parameters()}, float(lat), [t.clone() for t in g]
    finally:
        search.USE_PATHS, search.FUSED_OPT, search.FUSED_TAIL = old, old_f, old_t


def test_path_level_is_bit_identical_to_the_per_cell_route():
    pa, la, ga = _two_steps(True)
    pb, lb, gb = _two_steps(False)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), (k, float((pa[k] - pb[k]).abs().max()))
    assert abs(la - lb) < 1e-5                             # (the six stage latencies are summed in a different order)
    assert len(ga) == len(gb) and all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_epoch_driver_builds_styled_networks(tmp_path, monkeypatch):
    from tfnas_amd import epoch as ep, model_search as ms
    from tfnas_amd.latency import load_lat_lookup
    built = []

    class Recording(ms.Network):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self)
    monkeypatch.setattr(ms, 'Network', Recording)
    lut = load_lat_lookup('gpu')
    gen = torch.Generator().manual_seed(0)

    def queue(n):
        return lambda e: [(torch.randn(4, 3, 224, 224, generator=gen), torch.randint(0, 100, (4,), generator=gen))
                          for _ in range(n)]
    hist = ep.run_search(str(tmp_path), lut, queue(2), queue(1), epochs=2, warmup_epochs=1, target_lat=12.0,
                         log=None, se_style=STYLE)
    assert [h['steps'] for h in hist] == [2, 2] and 'parsed_arch' not in hist[0] and 'parsed_arch' in hist[1]
    assert all(os.path.exists(os.path.join(tmp_path, 'searched_model_%02d.pth.tar' % e)) for e in range(3))
    assert len(built) == 3                                 # the max-width store's network and one per epoch
    for net in built:
        assert all((b.se_act, b.se_gate) == S.MNV3 for st in STYLED for c in getattr(net, st).blocks() for b in c.m_ops)
        assert all(b.se_gate == 'sigmoid' for c in net.stage1.blocks() for b in c.m_ops)
    sd, _ = ep.load_search_checkpoint(str(tmp_path), 2)
    assert all(torch.isfinite(v).all() for v in sd.values())
