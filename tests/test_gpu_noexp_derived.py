"""MBConv blocks WITHOUT an expand convolution in the derived-network ("retrain") path: ``layers.MBInvertedResBlock(affine=True)``
-- two BatchNorm sites, tfnas_mbconv_fwd/bwd with TFNAS_CELL_NOEXPAND -- against ``oracle.DerivedBlock`` (pinned to the reference
in tests/test_noexp_oracle_pin.py) in train and eval mode, with injected drop-connect draws (some images dropped), a negative
gamma and the running statistics, at the tolerances of tests/test_gpu_derived.py; a chain that carries dx through the new
backward-data epilogue twice; a NetworkCfg whose stage1 opens with such a block; and the latency measurer."""
import math

import pytest
import torch

import _noexp

pytestmark = pytest.mark.gpu


def _negative_gamma(o):
    with torch.no_grad():
        o.depth_conv.bn.weight[0] = -0.7            # (the affine fold must not rely on gamma > 0)
        o.point_linear.bn.weight[1] = -0.4


def _compare(o, m, xo, xm, yo, ym, r):
    assert torch.allclose(ym.cpu(), yo, atol=2e-5, rtol=1e-4), float((ym.cpu() - yo).abs().max())
    for p in list(o.parameters()) + list(m.parameters()):
        p.grad = None
    (yo * r).sum().backward()
    (ym * r.cuda()).sum().backward()
    assert torch.allclose(xm.grad.cpu(), xo.grad, atol=2e-5 + 1e-3 * float(xo.grad.abs().max()), rtol=1e-3)
    po, pm = dict(o.named_parameters()), dict(m.named_parameters())
    assert list(po) == list(pm)
    for kk in po:
        assert pm[kk].grad is not None, kk
        err, ref = float((pm[kk].grad.cpu() - po[kk].grad).abs().max()), float(po[kk].grad.abs().max())
        assert err <= 2e-5 + 2e-3 * ref, (kk, err, ref)
    bo, bm = dict(o.named_buffers()), dict(m.named_buffers())
    assert list(bo) == list(bm)
    for kk in bo:
        assert torch.allclose(bm[kk].cpu().float(), bo[kk].float(), atol=1e-5, rtol=1e-4), kk   # running stats / batch counter


# (ic, se, oc, k, stride, act, H, W)
@pytest.mark.parametrize('geom', [(16, 8, 16, 3, 1, 'relu', 9, 13), (20, 0, 24, 5, 2, 'swish', 9, 13),
                                  (32, 8, 16, 3, 1, 'relu', 12, 12), (16, 16, 16, 7, 1, 'h-swish', 6, 7)],
                         ids=lambda g: 'ic%d_se%d_oc%d_k%d_s%d_%s' % g[:6])
@pytest.mark.parametrize('mode', ['train', 'train_drop', 'eval'])
def test_affine_block_without_expand_matches_oracle(geom, mode):
    import _acts
    ic, se, oc, k, s, act, H, W = geom
    N = 5
    with _acts.wrapped_oracle():
        o = _noexp.oracle_block(ic, se, oc, k, s, act, 31, derived=True)
        _negative_gamma(o)
        m = _noexp.hip_block_like(o, affine=True)
        assert m.inverted_bottleneck is None and len(m.bn_modules()) == 2
        gen = torch.Generator().manual_seed(5)
        x = torch.randn(N, ic, H, W, generator=gen)
        r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=gen)
        if mode == 'eval':
            o.eval(); m.eval()
        if mode == 'train_drop':
            o.drop_connect_rate = m.drop_connect_rate = 0.4
            u = torch.tensor([0.05, 0.9, 0.3, 0.7, 0.55])         # floor(0.6 + u): images 0 and 2 are dropped
            o.drop_u, m.drop_u = u, u
        xo = x.clone().requires_grad_(True)
        xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        yo, ym = o(xo), m(xm)                                     # (a RuntimeError before this feature)
        assert not any('inverted_bottleneck' in k for k, _ in m.named_parameters())
        _compare(o, m, xo, xm, yo, ym, r)


def test_chain_carries_dx_through_the_new_epilogue_twice():
    """an expand block, an expand-free residual block, an expand-free stride-2 block: train mode, drop-connect on the middle one"""
    specs = [(16, 48, 0, 16, 3, 1, 'relu'), (16, 16, 8, 16, 5, 1, 'relu'), (16, 8, 0, 24, 3, 2, 'relu')]
    os_, ms = [], []
    for i, (ic, mc, se, oc, k, s, act) in enumerate(specs):
        o = _noexp.oracle_block(ic, se, oc, k, s, act, 60 + i, derived=True, mc=mc)
        os_.append(o)
        ms.append(_noexp.hip_block_like(o, affine=True))
    assert [b.inverted_bottleneck is None for b in ms] == [False, True, True]
    u = torch.tensor([0.9, 0.1, 0.8, 0.6])
    os_[1].drop_connect_rate = ms[1].drop_connect_rate = 0.3
    os_[1].drop_u, ms[1].drop_u = u, u
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(4, 16, 10, 14, generator=gen)
    r = torch.randn(4, 24, 5, 7, generator=gen)
    xo = x.clone().requires_grad_(True)
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yo, ym = xo, xm
    for o, m in zip(os_, ms):
        yo, ym = o(yo), m(ym)
    oc_, mc_ = torch.nn.Sequential(*os_), torch.nn.Sequential(*ms)
    _compare(oc_, mc_, xo, xm, yo, ym, r)


def _train_once(monkeypatch, direct, lazy, steps=1):
    from tfnas_amd import model_eval as me
    monkeypatch.setattr(me, 'DIRECT_GRADS', direct)
    monkeypatch.setattr(me, 'LAZY_JOIN', lazy)
    torch.manual_seed(5)
    m = me.NetworkCfg(20, _noexp.noexp_network_config(20), None, 0.0, 0.2).cuda()
    before = {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    opt = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
    crit = me.CrossEntropyLabelSmooth(20, 0.1)
    gen = torch.Generator().manual_seed(11)
    blocks = [m.second_stem] + [b for st in m._stages() for b in st]
    losses = []
    for _ in range(steps):
        x = torch.randn(4, 3, 64, 64, generator=gen).cuda()
        y = torch.randint(0, 20, (4,), generator=gen).cuda()
        for b in blocks:
            b.drop_u = torch.rand(4, generator=gen)
        loss, _ = me.train_step(m, x, y, crit, opt, 5.0)
        losses.append(float(loss))
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    out.update({'mom%d' % i: opt.state[p]['momentum_buffer'].detach().cpu().clone() for i, p in enumerate(m.parameters())})
    return m, before, out, losses


def test_network_cfg_whose_stage1_opens_with_an_expand_free_block(monkeypatch):
    from tfnas_amd import model_eval as me, parsing
    cfg = _noexp.noexp_network_config(20)
    assert cfg['stage1'][0]['mid_channels'] == cfg['stage1'][0]['in_channels'] == 16
    for size in (64, 224):
        assert abs(parsing.count_macs_in_M(cfg, size) - _noexp.hand_macs_in_M(cfg, size)) < 1e-9
    m, before, base, losses = _train_once(monkeypatch, True, True)
    first = m.stage1[0]
    assert first.inverted_bottleneck is None and first.mid_channels == 16 and len(first.bn_modules()) == 2
    assert all(math.isfinite(v) for v in losses)
    for k, p in m.named_parameters():
        assert torch.isfinite(p).all(), k
        assert not torch.equal(p.detach().cpu(), before[k]), k            # every parameter moved
    assert m.config == cfg                                               # mid_channels == in_channels round-trips
    lut = {'base': 1.0}
    size = 32
    for st in m._stages():
        for b in st:
            key = '{}_{}_{}_{}_{}_k{}_s{}_{}'.format(b.name, size, b.in_channels, b.se_channels, b.out_channels, b.kernel_size,
                                                     b.stride, b.act_func)
            lut.setdefault(key, {})[b.mid_channels] = 0.5
            size = (size - 1) // b.stride + 1
    m.lat_lookup = lut
    nblk = sum(len(st) for st in m._stages())
    assert abs(m.get_lookup_latency(torch.zeros(1, 3, 64, 64)) - (1.0 + 0.5 * nblk)) < 1e-9
    # two fresh copies are bit-identical, and so are the plain gradient route and the eager join
    for direct, lazy in ((True, True), (False, False), (True, False), (False, True)):
        _, _, other, _ = _train_once(monkeypatch, direct, lazy)
        assert base.keys() == other.keys()
        for k in base:
            assert torch.equal(base[k], other[k]), (direct, lazy, k)
    # eval mode (running statistics) runs and is finite
    m.eval()
    with torch.no_grad():
        y = m(torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda())
    assert torch.isfinite(y).all()


@pytest.mark.parametrize('mode', ['inference', 'search'])
def test_measurer_times_an_expand_free_block(mode):
    from tfnas_amd.lut_builder import Measurer
    t = Measurer(torch.device('cuda')).measure(16, 16, 0, 16, 3, 1, 'relu', 28, batch=4, iters=2, reps=1, mode=mode)
    assert math.isfinite(t) and t > 0
    t = Measurer(torch.device('cuda')).measure(24, 12, 24, 40, 5, 2, 'swish', 28, batch=4, iters=2, reps=1, mode=mode)
    assert math.isfinite(t) and t > 0
