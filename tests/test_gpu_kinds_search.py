"""The search steps on a supernet whose cells mix all three block kinds (model_search.Network(primitives=...)): one bi-sampling
weight step (injected noise and rand_pos) and one architecture step of tfnas_amd.search, each from identical state, against the
oracle's w_step / a_step, which drive an oracle Network whose m_ops entries were replaced by the restatement blocks of
tests/_kinds.py / tests/_fused.py with the same weights; then parse_architecture -> derived_config -> NetworkCfg trains one step.

32 x 32 images, batch 4.  Stage 1 keeps the default primitives (its ReLU cells are handled exactly as tests/test_gpu_network.py
handles them); stages 2-6 (swish) hold plain, 7 x 7, expand-free and Fused-MBConv candidates.  The model does not take the path
level: every cell launch goes through the per-cell entry points, the mixed alpha-step cells through TFNAS_CELL_KINDS.
Gates: those tests/test_gpu_network.py applies to the same quantities (logits 1e-3, expected latency 1e-3,
post-step arch parameters 1e-3, loss 2e-3; weights: atol 2e-5 + rtol 1e-3 * max|ref|).  The architecture gradients themselves,
which the steps' comparison does not list, are held to a float64 run of the oracle within the float32 oracle's own distance from
it (test_a_step_single_step_arch_gradients says why the 1e-4 of the 224 x 224 test cannot be the bound at this shape)."""
import math

import pytest
import torch

import _fused
import _kinds
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

NAMES = ['MBI_k3_e3', 'FMB_k3_e6', 'DS_k5', 'MBI_k7_e6', 'FMB_k3_e3_se', 'DS_k3_se', 'MBI_k5_e3_se', 'MBI_k5_e6_se']
MIXED_STAGES = ('stage2', 'stage3', 'stage4', 'stage5', 'stage6')


def _primitives():
    from tfnas_amd import geometry
    return {st: {b: list(NAMES) for s2, b, *_ in geometry.iter_cells() if s2 == st} for st in MIXED_STAGES}


def _lut():
    lut = _kinds.AnyLut()
    lut['base'] = 1.5
    return lut


def _pair(seed=2, T=5.0):
    """(oracle Network with restatement blocks in stages 2-6, product Network(primitives=...)) with identical weights"""
    from tfnas_amd import Network, geometry
    mc = geometry.initial_mc_num_dddict()
    torch.manual_seed(seed)
    o = orc.Network(100, orc.initial_mc_num_dddict(), _lut())
    gen = torch.Generator().manual_seed(seed + 1)
    for st, b, ic, oc, s, act, size in geometry.iter_cells():
        if st not in MIXED_STAGES:
            continue
        cell = getattr(getattr(o, st), b)
        for i, name in enumerate(NAMES):
            layer, mid, se, k = geometry.primitive_block(name, ic, mc[st][b][i])
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


def test_w_step_against_the_oracle():
    from tfnas_amd import search
    o, m = _pair()
    assert not m.plain_candidates() and not m._use_paths(torch.zeros(1).cuda())
    kinds = [[op.kind.name for op in c.m_ops] for c in m.cells()]
    assert all(set(k) == {'MBCONV'} for k in kinds[:2]) and all(set(k) == {'MBCONV', 'NOEXPAND', 'FUSED'} for k in kinds[2:])
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    assert st.runner is None                                       # the per-cell route in every step
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 100, (4,), generator=g)
    ng = torch.empty(18, 8).exponential_(generator=g)
    rp = [int(v) for v in torch.randint(0, 7, (18,), generator=g)]
    before = {k: v.detach().clone() for k, v in o.named_parameters()}
    lo, logits_o, gi, ri = orc.w_step(o, x, y, oo[0], 5.0, noise_g=ng, rand_pos=rp)
    lm, logits_m = search.w_step(st, x.cuda(), y.cuda(), mo[0], 5.0, noise_g=ng.cuda(), rand_pos=rp)
    torch.cuda.synchronize()
    assert len({kinds[c][i] for c, i in enumerate(gi)} | {kinds[c][i] for c, i in enumerate(ri)}) == 3   # every kind was sampled
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


def _a_step_pair(with_f64=False):
    """one architecture step of both sides from IDENTICAL state (the single-step gates of tests/test_gpu_network.py are "from
    identical state": it teacher-forces before its first architecture step); all 18 cells soft, those of stages 2-6 as mixed
    launches.  with_f64: also the same step of a float64 copy of the oracle network."""
    import copy
    from tfnas_amd import search
    o, m = _pair()
    oo, mo = orc.make_optimizers(o), search.make_optimizers(m)
    st = search.SearchState(m)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 32, 32, generator=g)
    y = torch.randint(0, 100, (4,), generator=g)
    na = torch.empty(18, 8).exponential_(generator=g)
    r64 = None
    if with_f64:
        o64 = copy.deepcopy(o).double()
        r64 = orc.a_step(o64, x.double(), y, orc.make_optimizers(o64)[1], 15.0, 0.1, 5.0, noise=na.double())
    ro = orc.a_step(o, x, y, oo[1], 15.0, 0.1, 5.0, noise=na)
    rm = search.a_step(st, x.cuda(), y.cuda(), mo[1], 15.0, 0.1, 5.0, noise=na.cuda(), return_grads=True)
    torch.cuda.synchronize()
    return (o, m, ro, rm, r64) if with_f64 else (o, m, ro, rm)


def test_a_step_loss_latency_and_post_step_parameters():
    o, m, (la_o, ll_o, lat_o, g_o), (la_m, ll_m, lat_m, g_m) = _a_step_pair()
    print('a_step loss', float(la_o), float(la_m), 'lat', float(lat_o), float(lat_m))
    assert abs(float(lat_o) - float(lat_m)) < 1e-3 and abs(float(la_o) - float(la_m)) < 2e-3
    assert abs(float(ll_o) - float(ll_m)) < 1e-3
    for a, b in zip(o.arch_parameters(), m.arch_parameters()):
        assert torch.allclose(b.detach().cpu(), a.detach(), atol=1e-3), float((b.detach().cpu() - a.detach()).abs().max())


def test_a_step_single_step_arch_gradients():
    """d loss / d log_alphas and d betas of the step above (beyond the quantities the steps are compared on: a gradient is what an
    Adam step hides best).  Reference: the same step of a float64 copy of the oracle network.  Bound, per arch parameter: the
    float32 oracle's OWN distance from that float64 run on the same tensor -- the product must be at least as close to float64 as
    the float32 reference is (+ 1e-7 for a tensor both get exactly, stage6.betas = 0).  Nothing in the bound comes from the HIP
    side.

    Why not the atol 1e-4 against the float32 oracle that tests/test_gpu_network.py uses at 224 x 224: at 32 x 32 / batch 4 the
    cells of stages 3-6 see 2 x 2 and 1 x 1 pixels, every BatchNorm there normalises over 16 or 4 values, gradients reach
    |g| = 4.5, and the float32 oracle itself is up to 1.25e-2 (stage2.betas; relative 1e-3 ... 6.5e-3 over the 24 tensors) from
    its float64 run -- a float32 target that noisy cannot be hit to 1e-4 by any float32 implementation (an all-default supernet
    through the per-cell launches is 2.8e-3 from it at this shape).  Measured on an MI355X: HIP is within 3.1e-3 of float64
    (relative 2.5e-4 ... 1.6e-3), 2.3 ... 4.6 times closer than the float32 oracle on every tensor."""
    o, m, (_, _, _, g_o), (_, _, _, g_m), (_, _, _, g_64) = _a_step_pair(with_f64=True)
    names = [k for k, _ in o.named_parameters() if k.endswith('log_alphas') or k.endswith('betas')]
    rows = []
    for k, a, b, c in zip(names, g_o, g_m, g_64):
        own, err = float((a.double() - c).abs().max()), float((b.cpu().double() - c).abs().max())
        rows.append((k, own, err))
        print('d %-26s |g64| %.3e  float32 oracle - float64 %.3e  HIP - float64 %.3e' % (k, float(c.abs().max()), own, err))
    assert len(rows) == 24 and max(own for _, own, _ in rows) > 1e-4         # (the shape IS ill-conditioned: see above)
    for k, own, err in rows:
        assert err <= own + 1e-7, (k, err, own)


def test_parsed_architecture_exports_and_trains():
    from tfnas_amd import geometry, model_eval as me, parsing
    _, m = _pair()
    with torch.no_grad():                                          # make the three kinds win somewhere
        for ci, c in enumerate(m.cells()[2:]):
            c.log_alphas[(1, 2, 0, 4, 5)[ci % 5]] += 3.0
    parsed = parsing.parse_architecture(*parsing.get_op_and_depth_weights(m))
    cfg = parsing.derived_config(parsed, m.mc_num_dddict, 20, primitives=_primitives())
    names = [b['name'] for st in MIXED_STAGES for b in cfg[st]]
    assert 'FusedMBConvBlock' in names and 'MBInvertedResBlock' in names
    assert any(b['name'] == 'MBInvertedResBlock' and b['mid_channels'] == b['in_channels'] for st in MIXED_STAGES for b in cfg[st])
    net = me.NetworkCfg(20, cfg, None, 0.0, 0.0).cuda()
    twin = me.Network(20, parsed, m.mc_num_dddict, primitives=_primitives())
    assert list(twin.state_dict()) == list(net.state_dict()) and net.config == cfg
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
