"""GPU parity of the activations 'relu6' and 'h-swish' in the derived network: MBInvertedResBlock(affine=True) in train and eval
mode (drop-connect draws injected), a NetworkCfg whose blocks name the two activations, the latency measurement and the head --
against the CPU oracle under tests/_acts.wrapped_oracle() (pinned to the reference in tests/test_act_oracle_pin.py) and, for the
head, against torch.

Blocks: BN1 and BN2 get gamma ~ 3 (some entries negative) and beta ~ 2, and each test asserts in the oracle that every branch of
the activation (below, between, above its two kinks) holds at least 1 % of the pre-activations at BOTH sites -- this is where
ReLU6's upper clamp after BN2 is exercised (a search cell cannot reach it: tests/test_gpu_acts.py) -- and that no pre-activation
lies within 2e-5 of a kink (ReLU6's lower one included: nothing is replayed here).  Tolerances: those of the affine entry points'
standing tests (tests/test_gpu_derived.py, tests/test_gpu_k7.py) -- the same launches and arithmetic with another activation
body; the head at the cells' gate, abs err <= 2e-5 + 1e-4 * max|ref|, against a float64 reference."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import _acts
import _k7
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

BLOCKS = [
    # name, ic, mc, se, oc, k, stride, hw, N
    ('s1_res_se', 24, 72, 24, 24, 3, 1, 10, 4),
    ('s1_res_plain', 24, 72, 0, 24, 5, 1, 10, 4),
    ('s2_se', 40, 131, 40, 80, 5, 2, 9, 4),
    ('s2_plain', 40, 131, 0, 80, 3, 2, 9, 4),
]
# seed of each case's weights and input: the smallest from 5 up for which the oracle alone satisfies block_preact_check
SEEDS = {
    ('relu6', 's1_res_se', 'train'): 6, ('relu6', 's1_res_se', 'eval'): 5, ('relu6', 's1_res_plain', 'train'): 5, ('relu6', 's1_res_plain', 'eval'): 6,
    ('relu6', 's2_se', 'train'): 5, ('relu6', 's2_se', 'eval'): 5, ('relu6', 's2_plain', 'train'): 5, ('relu6', 's2_plain', 'eval'): 5,
    ('h-swish', 's1_res_se', 'train'): 5, ('h-swish', 's1_res_se', 'eval'): 5, ('h-swish', 's1_res_plain', 'train'): 5, ('h-swish', 's1_res_plain', 'eval'): 5,
    ('h-swish', 's2_se', 'train'): 5, ('h-swish', 's2_se', 'eval'): 5, ('h-swish', 's2_plain', 'train'): 5, ('h-swish', 's2_plain', 'eval'): 5,
}
ALL_KINKS = {'relu6': (0.0, 6.0), 'h-swish': (-3.0, 3.0)}


def oracle_block(cfg, act, mode):
    """the oracle's DerivedBlock of one case with strong BN1 / BN2, running statistics near the batch's, input and cotangent"""
    name, ic, mc, se, oc, k, s, hw, N = cfg
    seed = SEEDS[(act, name, mode)]
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    o = orc.DerivedBlock(ic, mc, se, oc, k, s, act)
    _acts.strong_bn(o, gen)
    x = _acts.spiked_input((N, ic, hw, hw), gen, p=0.0)
    ho = (hw - 1) // s + 1
    r = torch.randn(N, oc, ho, ho, generator=gen)
    # running statistics of BN1 / BN2 near the batch's own (eval mode then reaches the same branches as train mode)
    c = copy.deepcopy(o).train()
    for m in (c.inverted_bottleneck.bn, c.depth_conv.bn):
        m.momentum = 1.0
    with torch.no_grad(), _acts.wrapped_oracle():
        c(x)
    with torch.no_grad():
        for dst, src in ((o.inverted_bottleneck.bn, c.inverted_bottleneck.bn), (o.depth_conv.bn, c.depth_conv.bn)):
            dst.running_mean.copy_(src.running_mean * 1.05)
            dst.running_var.copy_(src.running_var * 1.1)
    o.drop_connect_rate = 0.4
    o.drop_u = torch.tensor([0.9, 0.1, 0.7, 0.3])       # floor(0.6 + u): images 0 and 2 kept, 1 and 3 dropped
    if mode == 'eval':
        o.eval()
    else:
        o.train()
    return o, x, r


def block_preact_check(o, x, act):
    """every branch holds at least 1 % at both sites; nothing within 2e-5 of any kink"""
    z1, z2 = _acts.derived_preacts(o, x)
    out = []
    for z in (z1, z2):
        fr = _acts.branch_fractions(z, act)
        assert min(fr) >= 0.01, (act, fr)
        assert all(int(((z - kk).abs() < 2e-5).sum()) == 0 for kk in ALL_KINKS[act]), act
        out.append(fr)
    return out


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('cfg', BLOCKS, ids=lambda c: c[0])
@pytest.mark.parametrize('act', _acts.NEW_ACTS)
def test_derived_block_matches_wrapped_oracle(act, cfg, mode):
    from tfnas_amd.layers import MBInvertedResBlock
    name, ic, mc, se, oc, k, s, hw, N = cfg
    o, x, r = oracle_block(cfg, act, mode)
    block_preact_check(o, x, act)
    m = MBInvertedResBlock(ic, mc, se, oc, k, s, affine=True, act_func=act)
    m.load_state_dict(o.state_dict())
    m = m.cuda()
    m.drop_connect_rate, m.drop_u = o.drop_connect_rate, o.drop_u
    m.train(o.training)
    xo = x.clone().requires_grad_(True)
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with _acts.wrapped_oracle():
        yo = o(xo)
        (yo * r).sum().backward()
    ym = m(xm)
    assert torch.allclose(ym.cpu(), yo, atol=2e-5, rtol=1e-4), float((ym.cpu() - yo).abs().max())
    (ym * r.cuda()).sum().backward()
    assert torch.allclose(xm.grad.cpu(), xo.grad, atol=2e-5 + 1e-3 * float(xo.grad.abs().max()), rtol=1e-3)
    for (kk, po), (_, pm) in zip(o.named_parameters(), m.named_parameters()):      # gamma / beta gradients among them
        err, ref = float((pm.grad.cpu() - po.grad).abs().max()), float(po.grad.abs().max())
        assert err <= 2e-5 + 2e-3 * ref, (kk, err, ref)
    assert any(kk.endswith('bn.weight') for kk, _ in o.named_parameters())
    for (kk, bo), (_, bm) in zip(o.named_buffers(), m.named_buffers()):
        assert torch.allclose(bm.cpu().float(), bo.float(), atol=1e-5, rtol=1e-4), kk       # running stats / batch counter


def oracle_network(num_classes=50):
    """(config, the oracle's DerivedNetwork with the config's activations and non-trivial BatchNorms, input, targets, draws)"""
    cfg, arch, mc = _acts.act_network_config(num_classes)
    torch.manual_seed(3)
    o = orc.DerivedNetwork(num_classes, arch, mc, 0.0, 0.2)
    blocks = o.blocks()
    cfg_blocks = [c for i in range(1, 7) for c in cfg['stage%d' % i]]
    assert len(blocks) == len(cfg_blocks)
    for b, c in zip(blocks, cfg_blocks):
        assert (b.in_channels, b.mid_channels, b.kernel_size, b.stride) == (c['in_channels'], c['mid_channels'], c['kernel_size'],
                                                                            c['stride'])
        b.act_func = c['act_func']
    _k7.randomise_bn(o, torch.Generator().manual_seed(1))
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 64, 64, generator=gen)
    y = torch.randint(0, num_classes, (2,), generator=gen)
    us = [torch.rand(2, generator=gen) for _ in range(1 + len(blocks))]
    return cfg, o, x, y, us


def test_networkcfg_with_new_activations_matches_oracle_network():
    """NetworkCfg from a config whose blocks name 'relu6' and 'h-swish' in turn, at 2 x 3 x 64 x 64: config() returns the
    activations it was given; one training step (loss, every parameter and buffer afterwards) and the eval-mode logits against
    oracle.DerivedNetwork built from the same config"""
    from tfnas_amd import model_eval as me
    cfg, o, x, y, us = oracle_network()
    m = me.NetworkCfg(50, cfg, None, 0.0, 0.2)
    assert m.config == cfg
    got = [c['act_func'] for i in range(1, 7) for c in m.config['stage%d' % i]]
    assert got == [_acts.NEW_ACTS[i % 2] for i in range(len(got))] and len(got) == 11
    m.load_state_dict(o.state_dict())
    m = m.cuda()
    for bo, bm, u in zip([o.second_stem] + o.blocks(), [m.second_stem] + [b for st in m._stages() for b in st], us):
        bo.drop_u, bm.drop_u = u, u
    oo = torch.optim.SGD(o.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
    mo = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
    o.train()
    with _acts.wrapped_oracle():
        lo = orc.label_smooth_loss(o(x), y, 50, 0.1)
        oo.zero_grad()
        lo.backward()
    torch.nn.utils.clip_grad_norm_(o.parameters(), 5.0)
    oo.step()
    lm, _ = me.train_step(m, x.cuda(), y.cuda(), me.CrossEntropyLabelSmooth(50, 0.1), mo, 5.0)
    assert abs(float(lo.detach()) - float(lm.detach())) < 1e-4
    for (k, a), (_, b) in zip(o.state_dict().items(), m.state_dict().items()):
        err, ref = float((b.cpu().float() - a.float()).abs().max()), float(a.float().abs().max())
        assert err <= 1e-5 + 2e-3 * ref, (k, err, ref)
    o.eval(); m.eval()
    with torch.no_grad(), _acts.wrapped_oracle():
        eo = o(x)
    with torch.no_grad():
        em = m(x.cuda())
    assert torch.allclose(em.cpu(), eo, atol=1e-3, rtol=1e-3), float((em.cpu() - eo).abs().max())


@pytest.mark.parametrize('act', _acts.NEW_ACTS)
def test_latency_measurement_of_a_block(act):
    from tfnas_amd import lut_builder
    ms = lut_builder.Measurer(torch.device('cuda:0')).measure(24, 72, 24, 24, 5, 1, act, 28, batch=4, iters=2, reps=1)
    assert math.isfinite(ms) and ms > 0


# ------------------------------------------------------------------------------------------------ head
def _act64(z, act):
    return F.relu6(z) if act == 'relu6' else z * F.relu6(z + 3.0) / 6.0


def head_case(act, affine, seed):
    """2 x 320 x 7 x 7 -> 1280: the layer's weights, input, cotangent and the float64 reference (pooled, dx, dW, dgamma, dbeta)"""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(1280, 320, 1, 1, generator=gen) * 0.05
    gamma = 3.0 + 0.3 * torch.randn(1280, generator=gen)
    gamma[::5] *= -1
    beta = 2.0 + 0.2 * torch.randn(1280, generator=gen)
    x = _acts.spiked_input((2, 320, 7, 7), gen, p=0.0 if affine else 0.04)
    r = torch.randn(2, 1280, generator=gen)
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.batch_norm(F.conv2d(xd, wd), None, None, gd if affine else None, bd if affine else None, True, 0.0, 1e-5)
    pooled = F.adaptive_avg_pool2d(_act64(z, act), 1).flatten(1)
    (pooled * r.double()).sum().backward()
    ref = dict(pooled=pooled.detach(), dx=xd.grad, dw=wd.grad)
    if affine:
        ref.update(dgamma=gd.grad, dbeta=bd.grad)
    return w, gamma, beta, x, r, z.detach(), ref


HEAD_SEEDS = {('relu6', False): 2, ('relu6', True): 2, ('h-swish', False): 1, ('h-swish', True): 3}     # (the float64 reference alone satisfies the kink condition)


@pytest.mark.parametrize('affine', [False, True], ids=['search', 'affine'])
@pytest.mark.parametrize('act', _acts.NEW_ACTS)
def test_head_pool_and_its_backward_match_torch(act, affine):
    """TFNAS_MODE_HEAD (k_head_pool / k_head_bwd; tfnas_head_fwd/bwd and the affine pair): pooled output, dx, dW (and d gamma,
    d beta) against a float64 torch reference; every branch of the activation holds at least 1 % (affine) / 0.1 % (batch-stat
    form, spiked input) of the pre-activations and none lies within 2e-5 of a kink"""
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan, HeadAffineFn, HeadFn
    from tfnas_amd.layers import ConvLayer
    from tfnas_amd.model_eval import _HeadBlock
    w, gamma, beta, x, r, z, ref = head_case(act, affine, HEAD_SEEDS[(act, affine)])
    fr = _acts.branch_fractions(z, act)
    assert min(fr) >= (0.01 if affine else 1e-3), fr
    assert all(int(((z - kk).abs() < 2e-5).sum()) == 0 for kk in ALL_KINKS[act])
    layer = ConvLayer(320, 1280, kernel_size=1, stride=1, affine=affine, act_func=act)
    with torch.no_grad():
        layer.conv.weight.copy_(w)
        if affine:
            layer.bn.weight.copy_(gamma)
            layer.bn.bias.copy_(beta)
    layer = layer.cuda().train()
    plan = CellPlan(320, 4, 1, act, [_HeadBlock(layer)], mode=_lib.MODE_HEAD)
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    if affine:
        pooled = HeadAffineFn.apply(plan, xm, layer.bn, True, layer.conv.weight, layer.bn.weight, layer.bn.bias)
    else:
        pooled = HeadFn.apply(plan, xm, layer.conv.weight)
    (pooled * r.cuda()).sum().backward()
    got = dict(pooled=pooled.detach(), dx=xm.grad, dw=layer.conv.weight.grad)
    if affine:
        got.update(dgamma=layer.bn.weight.grad, dbeta=layer.bn.bias.grad)
    for k, want in ref.items():
        err, mx = float((got[k].cpu().double() - want).abs().max()), float(want.abs().max())
        assert err <= 2e-5 + 1e-4 * mx, (k, err, mx)
