"""CPU: the host side of the parameter-group retrain tail -- optim.param_groups on derived networks with every block kind,
RetrainState.plan as pure inspection, and the binding of TfnasOptGroups / tfnas_opt_groups_step against include/tfnas_hip.h."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')


def _network(num_classes=20):
    """A derived network with a plain block, squeeze-excite blocks, MixConv blocks (stage 4 / 5) and Fused-MBConv blocks (stage 1)."""
    import _mix
    from tfnas_amd import model_eval as me
    cfg = _mix.mix_network_config(num_classes)
    a, b = cfg['stage1']
    a.update(name='FusedMBConvBlock', kernel_size=3, mid_channels=48, se_channels=16)
    b.update(name='FusedMBConvBlock', kernel_size=3, mid_channels=50, se_channels=0)
    torch.manual_seed(0)
    return me.NetworkCfg(num_classes, cfg, None, 0.0, 0.0)


@pytest.fixture(scope='module')
def net():
    return _network()


def test_param_groups_on_a_network_of_every_block_kind(net):
    from tfnas_amd import optim
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock, MixDepthwiseConv2d
    blocks = [m for m in net.modules() if isinstance(m, (MBInvertedResBlock, FusedMBConvBlock))]
    assert any(isinstance(b, FusedMBConvBlock) for b in blocks)
    assert any(b.squeeze_excite is not None for b in blocks) and any(b.squeeze_excite is None for b in blocks)
    mixes = [m for m in net.modules() if isinstance(m, MixDepthwiseConv2d)]
    assert mixes and all(m.weight.ndim == 1 for m in mixes)
    assert net.classifier.linear.bias is not None

    groups = optim.param_groups(net, 4e-5)
    assert [g['weight_decay'] for g in groups] == [4e-5, 0.0]
    decay, rest = ({id(p) for p in g['params']} for g in groups)
    every = {id(p): k for k, p in net.named_parameters()}
    assert not decay & rest and decay | rest == set(every)                       # every parameter in exactly one group
    assert len(groups[0]['params']) + len(groups[1]['params']) == len(every)
    # the no-decay group, derived independently: parameters of BatchNorm modules, and everything named 'bias'
    bn = {id(p) for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d) for p in m.parameters(recurse=False)}
    bias = {i for i, k in every.items() if k.endswith('.bias')}
    assert bn and bias - bn
    assert rest == bn | bias
    for m in mixes:
        assert id(m.weight) in decay                                             # the packed 1-D depthwise weight is decayed
    assert id(net.classifier.linear.bias) in rest and id(net.classifier.linear.weight) in decay
    se = next(b.squeeze_excite for b in blocks if b.squeeze_excite is not None)
    assert id(se.conv_reduce.bias) in rest and id(se.conv_expand.bias) in rest and id(se.conv_reduce.weight) in decay
    # the selectors on their own
    only_bn = optim.param_groups(net, 1e-5, no_decay=('bn',))
    assert {id(p) for p in only_bn[1]['params']} == bn
    only_bias = optim.param_groups(net, 1e-5, no_decay=('bias',))
    assert {id(p) for p in only_bias[1]['params']} == bias
    one = optim.param_groups(net, 1e-5, no_decay=())
    assert len(one) == 1 and len(one[0]['params']) == len(every)
    with pytest.raises(ValueError):
        optim.param_groups(net, 1e-5, no_decay=('ndim',))


def test_plan_is_pure_inspection(net):
    from tfnas_amd import model_eval as me
    from tfnas_amd import optim
    plan, fus = me.RetrainState.plan, me.RetrainState.fusable
    P = list(net.parameters())
    G = lambda: optim.param_groups(net, 4e-5)
    SGD, RMS = torch.optim.SGD, torch.optim.RMSprop

    def both(opt):
        return plan(opt, net), fus(opt, net)

    assert both(SGD(P, 0.1, momentum=0.9, weight_decay=4e-5)) == ('sgd', True)
    assert both(SGD(G(), 0.1, momentum=0.9)) == ('groups', False)
    assert both(SGD(P, 0.1, momentum=0.9, nesterov=True)) == ('groups', False)
    assert both(SGD(G(), 0.1, momentum=0.9, nesterov=True)) == ('groups', False)
    assert both(RMS(G(), 0.01, alpha=0.9, eps=1e-3, momentum=0.9)) == ('groups', False)
    assert both(RMS(P, 0.01)) == ('groups', False)
    assert both(optim.RMSpropTF(G(), 0.01)) == ('groups', False)
    eight = [{'params': P[i::8], 'lr': 0.01 * (i + 1)} for i in range(8)]
    assert both(SGD(eight, 0.1, momentum=0.9)) == ('groups', False)
    # each of these is the torch route
    assert both(SGD(G(), 0.1, momentum=0.9, dampening=0.1)) == (None, False)
    assert both(RMS(G(), 0.01, centered=True)) == (None, False)
    assert both(SGD(G(), 0.1, momentum=0.9, maximize=True)) == (None, False)
    assert both(RMS(G(), 0.01, maximize=True)) == (None, False)
    assert both(SGD(P[:-1], 0.1, momentum=0.9)) == (None, False)                               # a subset
    assert both(RMS([{'params': P[:5]}, {'params': P[6:]}], 0.01)) == (None, False)
    nine = [{'params': P[i::9]} for i in range(9)]
    assert both(SGD(nine, 0.1, momentum=0.9)) == (None, False)
    g = G()
    g[1]['momentum'] = 0.5
    assert both(SGD(g, 0.1, momentum=0.9)) == (None, False)                                    # differing momentum
    g = G()
    g[1]['alpha'] = 0.99
    assert both(RMS(g, 0.01, alpha=0.9)) == (None, False)
    g = G()
    g[1]['eps'] = 1e-8
    assert both(optim.RMSpropTF(g, 0.01)) == (None, False)
    hooked = SGD(G(), 0.1, momentum=0.9)
    hooked.register_step_post_hook(lambda *a: None)
    assert both(hooked) == (None, False)
    hooked = SGD(P, 0.1, momentum=0.9)
    hooked.register_step_pre_hook(lambda *a: None)
    assert both(hooked) == (None, False)
    assert both(torch.optim.Adam(P, 1e-3)) == (None, False)
    P[3].requires_grad_(False)                                                                 # a frozen parameter
    try:
        assert both(SGD(G(), 0.1, momentum=0.9)) == (None, False)
        assert both(SGD(P, 0.1, momentum=0.9)) == (None, False)
    finally:
        P[3].requires_grad_(True)
    # nothing was touched: no state, no arena
    opt = RMS(G(), 0.01, momentum=0.9)
    assert plan(opt, net) == 'groups' and not opt.state and getattr(net, '_retrain_state', None) is None


def test_rmsprop_tf_is_an_ordinary_optimizer():
    from tfnas_amd.optim import RMSpropTF
    torch.manual_seed(1)
    lin = torch.nn.Linear(5, 3)
    opt = RMSpropTF(lin.parameters(), 0.01, weight_decay=1e-4)
    for _ in range(2):
        lin.zero_grad()
        lin(torch.randn(4, 5)).square().sum().backward()
        opt.step()
    st = opt.state[lin.weight]
    assert st['step'] == 2 and set(st) == {'step', 'square_avg', 'momentum_buffer'}
    other = RMSpropTF(torch.nn.Linear(5, 3).parameters(), 0.5)
    other.load_state_dict(opt.state_dict())
    assert other.param_groups[0]['lr'] == 0.01
    assert torch.equal(list(other.state.values())[0]['square_avg'], st['square_avg'])
    for bad in (dict(eps=0.0), dict(alpha=1.5), dict(momentum=-0.1), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            RMSpropTF(lin.parameters(), **bad)


def test_struct_and_symbol_against_the_header():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.lib()
    assert lib.tfnas_abi_version() == 4
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct TfnasOptGroups \{(.*?)\} TfnasOptGroups;', src, flags=re.S).group(1)
    fields = [(t, n, dim) for t, n, dim in re.findall(r'(int32_t|float)\s+(\w+)(?:\[(\w+)\])?;', body)]
    assert [n for _, n, _ in fields] == [n for n, _ in _lib.TfnasOptGroups._fields_]
    assert int(re.search(r'#define TFNAS_OPT_MAX_GROUPS (\d+)', src).group(1)) == _lib.OPT_MAX_GROUPS == 8
    size = sum(4 * (_lib.OPT_MAX_GROUPS if dim else 1) for _, _, dim in fields)
    assert size == C.sizeof(_lib.TfnasOptGroups) == lib.tfnas_sizeof(9) == 4 * (3 + 16 + 6)
    for name, val in (('SGD', _lib.OPT_SGD), ('RMSPROP', _lib.OPT_RMSPROP), ('RMSPROP_TF', _lib.OPT_RMSPROP_TF),
                      ('NESTEROV', _lib.OPT_NESTEROV)):
        assert int(re.search(r'#define TFNAS_OPT_%s (\d+)' % name, src).group(1)) == val
    assert re.search(r'^int tfnas_opt_groups_step\(const TfnasOptGroups \*d,', src, flags=re.M)
    fn = lib.tfnas_opt_groups_step
    assert fn.argtypes[0] is not None and len(fn.argtypes) == 12
    # the first refusals need no GPU: nothing is dereferenced on the device before them
    d = _lib.TfnasOptGroups()
    assert fn(None, None, None, None, None, None, None, 64, None, 1, None, None) == -2
    assert fn(C.byref(d), None, None, None, None, None, None, 64, None, 1, None, None) == -2
