"""Squeeze-excite styles in the derived network's affine form (tfnas_mbconv_fwd/bwd through layers.*Block(affine=True)): the style
('relu', 'h-sigmoid') on an 'h-swish' plain block and an 'h-swish' Fused-MBConv block, in training with injected drop-connect draws
and in eval mode with running statistics, held in float64 against the restatement of tests/_sestyle.py the way
tests/test_gpu_affine_f64.py holds the unstyled form: every tensor to ``2e-5 + 1e-4 max|ref|``, running statistics to
``1e-6 + 1e-5 |ref|`` elementwise (tests/_affineref.py), BatchNorm parameters with that file's edge channels.  Seeds: the first
whose float64 BatchNorm outputs, SE hidden pre-activations and gate pre-activations keep KINK_TAU from every kink (asserted on the
CPU before anything is launched); the gate biases are spread so that the gate saturates on both sides.
Then a styled ``model.config`` -> NetworkCfg trains one step."""
import copy
import math
from collections import OrderedDict

import pytest
import torch

import _affineref as ar
import _fused
import _sestyle as S
import tfnas_oracle as orc
from _rawcell import KINKS, KINK_TAU

pytestmark = pytest.mark.gpu

ACT, STYLE = 'h-swish', S.MNV3
# (ic, mc, se, oc, stride, N, H, W): residual blocks (drop-connect), 5 images (tests/_affineref.DROP_U), a ragged fused width
GEOM = {'plain': (16, 48, 16, 16, 1, 5, 5, 7), 'fused': (16, 22, 8, 16, 1, 5, 5, 7)}
_CACHE = {}


def _build(kind, mode, seed):
    ic, mc, se, oc, s, N, H, W = GEOM[kind]
    gen = torch.Generator().manual_seed(seed)
    o = orc.DerivedBlock(ic, mc, se, oc, 3, s, ACT) if kind == 'plain' else _fused.FusedRef(ic, mc, se, oc, s, ACT, derived=True)
    ar.randomise(o, gen)
    with torch.no_grad():
        o.squeeze_excite.conv_expand.bias.mul_(S.GATE_BIAS_GAIN)
    S.restyle(o, *STYLE)
    x, r = ar.inputs(gen, N, ic, H, W, (N, oc, H, W))
    return ar.Case(name='%s-%s' % (kind, mode), geom=GEOM[kind], mode=mode, seed=seed, o=o, x=x, r=r, u=ar.drop_u(mode, N))


def _kink_distance(case):
    """float64: BatchNorm outputs that feed the block's activation against its kinks, the SE hidden pre-activations against the
    hidden activation's, the gate pre-activations against +-3; also the gate's branch counts"""
    o = copy.deepcopy(case.o).double()
    o.train(case.mode != 'eval')
    bns = ar.batchnorms(o)[:-1]                       # (the last BatchNorm feeds no activation)
    zs = []
    hooks = [m.register_forward_hook(lambda _m, _i, out: zs.append(out.detach())) for m in bns]
    with torch.no_grad():
        o(case.x.double())
    for h in hooks:
        h.remove()
    st = o._last_state
    d = min(float((z - k).abs().min()) for z in zs for k in KINKS[ACT])
    d = min([d] + [float((st.hpre[0] - k).abs().min()) for k in KINKS[STYLE[0]]])
    d = min([d] + [float((st.gpre[0] - k).abs().min()) for k in S.GATE_KINKS[STYLE[1]]])
    v = st.gpre[0]
    return d, (int((v <= -3).sum()), int(((v > -3) & (v < 3)).sum()), int((v >= 3).sum()))


def _case(kind, mode):
    if (kind, mode) not in _CACHE:
        for seed in range(200):
            case = _build(kind, mode, seed)
            if not ar.conditioned(case.o):
                continue
            d, branches = _kink_distance(case)
            if d >= KINK_TAU and min(branches) > 0:
                case.ref = ar.reference(case)
                _CACHE[(kind, mode)] = case
                break
        else:
            raise AssertionError('no qualifying seed')
    case = _CACHE[(kind, mode)]
    d, branches = _kink_distance(case)
    assert d >= KINK_TAU and min(branches) > 0, (d, branches)
    return case


def _module(kind, case):
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock
    ic, mc, se, oc, s = case.geom[:5]
    cls = MBInvertedResBlock if kind == 'plain' else FusedMBConvBlock
    m = cls(ic, mc, se, oc, 3, s, affine=True, act_func=ACT, se_act=STYLE[0], se_gate=STYLE[1])
    m.load_state_dict(case.o.state_dict())
    for bn in m.bn_modules():
        bn.momentum = ar.MOMENTUM
    return m.cuda()


def _run_module(m, case):
    m.train(case.mode != 'eval')
    m.drop_connect_rate, m.drop_u = 0.0, None
    if case.u is not None:
        m.drop_connect_rate, m.drop_u = 1.0 - ar.KEEP, case.u
    xm = case.x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = m(xm)
    (y * case.r.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = OrderedDict(y=y.detach(), dx=xm.grad)
    for k, p in m.named_parameters():
        got['g.' + k] = p.grad
    for k, b in m.named_buffers():
        if 'running' in k:
            got['b.' + k] = b.detach().clone()
    return got


@pytest.mark.parametrize('mode', ('drop', 'eval'))
@pytest.mark.parametrize('kind', ('plain', 'fused'))
def test_styled_affine_block_matches_float64_restatement(kind, mode):
    from tfnas_amd import _lib
    case = _case(kind, mode)
    m = _module(kind, case)
    got = _run_module(m, case)
    d = m._plan.desc(*[case.x.shape[i] for i in (0, 2, 3)])[0]
    assert d.se_style == 0x11 and d.flags & _lib.CELL_SE_STYLE
    assert set(got) == {k for k in case.ref if not k.startswith('_')}
    ratios = ar.compare(got, case.ref)
    print('SESTYLE_F64 %-12s %s' % (case.name, '  '.join('%s %.4f' % kv for kv in ar.classes(ratios).items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad
    # the style is what was computed: the unstyled float64 oracle is far outside the gate
    plain = ar.Case(**dict(case.__dict__, o=S.restyle(copy.deepcopy(case.o))))
    assert ar.compare(got, ar.reference(plain))['y'] > 10.0
    if mode == 'eval':
        for k, b in case.o.named_buffers():
            if 'running' in k:
                assert torch.equal(got['b.' + k].cpu(), b), k


def test_styled_config_builds_and_trains():
    """parse -> derived_config(se_style=...) -> NetworkCfg, one training step (as tests/test_gpu_kinds_search.py's last test)"""
    from tfnas_amd import geometry, model_eval as me, parsing
    mc = geometry.initial_mc_num_dddict()
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j + 4) % 8) for j, b in enumerate(bl) if j < 2))
                       for i, (st, bl) in enumerate(mc.items()))
    style = {'stage%d' % s: S.MNV3 for s in range(2, 7)}
    cfg = parsing.derived_config(arch, mc, 20, se_style=style)
    for s in range(2, 7):
        for b in cfg['stage%d' % s]:
            b['act_func'] = 'h-swish'                                # a MobileNetV3-style network
    net = me.NetworkCfg(20, cfg, None, 0.0, 0.0).cuda()
    assert net.config == cfg and sum(b.se_channels > 0 for s in range(2, 7) for b in getattr(net, 'stage%d' % s)) >= 3
    assert all((b.se_act, b.se_gate) == S.MNV3 for s in range(2, 7) for b in getattr(net, 'stage%d' % s))
    before = {k: v.detach().cpu().clone() for k, v in net.named_parameters()}
    opt = torch.optim.SGD(net.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 32, 32, generator=gen).cuda()
    y = torch.randint(0, 20, (4,), generator=gen).cuda()
    loss, logits = me.train_step(net, x, y, me.CrossEntropyLabelSmooth(20, 0.1), opt, 5.0)
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and torch.isfinite(logits).all()
    styled = [b._plan for s in range(2, 7) for b in getattr(net, 'stage%d' % s) if b.se_channels > 0]
    assert styled and all(p.se_style == 0x11 for p in styled)
    for k, p in net.named_parameters():               # (a bias that starts at 0 behind a dead ReLU unit may stay: weights all move)
        assert torch.isfinite(p).all() and (p.dim() == 1 or not torch.equal(p.detach().cpu(), before[k])), k
