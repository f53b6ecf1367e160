"""Helpers shared by the 7 x 7 depthwise tests (tests/test_k7_*.py, tests/test_gpu_k7.py) and by the generator of their
fixtures (tests/golden/make_golden_k7.py): the block scenarios of the oracle pin, cells with chosen candidates replaced by
other kernel sizes, and the rebuilding of such a cell from a cell_k7_*.npz fixture."""
import itertools
from collections import OrderedDict

import numpy as np
import torch

import _golden
import tfnas_oracle as orc

# ------------------------------------------------------------------------------------------------ oracle pin (blocks)
# stride x activation x SE at 2 x 16 x 9 x 13; mid 24 (an expand convolution exists: mid > in), out 16 (residual at stride 1)
PIN_GEOM = dict(N=2, ic=16, mc=24, oc=16, H=9, W=13, se=8)
PIN_CASES = [(s, act, se) for s, act, se in itertools.product((1, 2), ('relu', 'swish'), (0, PIN_GEOM['se']))]
PIN_DROP = 0.3          # drop-connect rate of the derived form (residual blocks, train mode)


def pin_tag(form, case):
    return '%s_s%d_%s_se%d' % ((form,) + tuple(case))


def randomise_bn(mod, gen):
    """non-trivial gamma / beta / running statistics (fresh BatchNorms are gamma 1, beta 0, mean 0, var 1)"""
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(1.0 + 0.2 * torch.rand(m.running_var.shape, generator=gen))


def pin_oracle_block(form, case, k=7):
    """The oracle's block of one pin case (float64) with seeded weights, and its input / cotangent."""
    s, act, se = case
    q = PIN_GEOM
    seed = 1000 + 97 * PIN_CASES.index(case) + (0 if form == 'search' else 50)
    torch.manual_seed(seed)
    cls = orc.MBConv if form == 'search' else orc.DerivedBlock
    blk = cls(q['ic'], q['mc'], se, q['oc'], k, s, act)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))      # SE biases
    if form == 'derived':
        randomise_bn(blk, gen)
        blk.drop_connect_rate = PIN_DROP
    blk = blk.double().train()
    x = torch.randn(q['N'], q['ic'], q['H'], q['W'], generator=gen).double()
    r = torch.randn(q['N'], q['oc'], (q['H'] - 1) // s + 1, (q['W'] - 1) // s + 1, generator=gen).double()
    return blk, x, r, seed + 2


def pin_run(blk, x, r, rng_seed):
    """Forward + backward of one block (oracle's or reference's: same parameter names, same forward(x)): the output, dx, every
    parameter gradient and (derived form) the buffers after the step, as float64 arrays.  torch's generator is seeded right
    before the forward: the reference draws its drop-connect uniforms from it ([N, 1, 1, 1] in x's dtype); the oracle's block is
    handed the same draws (drop_u)."""
    blk.zero_grad()
    xs = x.clone().requires_grad_(True)
    if hasattr(blk, 'drop_u'):
        torch.manual_seed(rng_seed)
        blk.drop_u = torch.rand((x.size(0), 1, 1, 1), dtype=x.dtype).view(-1)
    torch.manual_seed(rng_seed)
    out = blk(xs)
    (out * r).sum().backward()
    res = OrderedDict(out=out.detach().numpy().copy(), dx=xs.grad.numpy().copy())
    for k, p in blk.named_parameters():
        res['g.' + k] = p.grad.numpy().copy()
    for k, b in blk.named_buffers():
        res['b.' + k] = b.detach().double().numpy().copy()
    return res


def pin_record(res):
    """What the fixture keeps of pin_run's result: the depthwise weight gradient whole (the 49 taps are what the pin is about),
    _golden.probe of every other tensor."""
    out = OrderedDict()
    for k, v in res.items():
        t = torch.from_numpy(np.asarray(v))
        out[k] = np.asarray(v) if k == 'g.depth_conv.conv.weight' else _golden.probe(t)
    return out


# ------------------------------------------------------------------------------------------------ cells
SOFT_KS = (3, 3, 5, 5, 7, 7, 3, 7)       # kernel sizes of the eight candidates of a mixed cell (SE on the last four, as always)


def replace_oracle_ops(o, ks, seed=0):
    """Candidates of the oracle cell whose kernel size differs from ks[i] are rebuilt with kernel size ks[i] (fresh seeded
    weights, non-trivial SE biases)."""
    g = torch.Generator().manual_seed(4242 + seed)
    for i, k in enumerate(ks):
        op = o.m_ops[i]
        if op.kernel_size == k:
            continue
        torch.manual_seed(777 + 13 * i + seed)
        new = orc.MBConv(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, k, op.stride, op.act_func)
        with torch.no_grad():
            for p in new.parameters():
                if p.dim() == 1:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        o.m_ops[i] = new
    return o


def hip_cell_like(o, T=None):
    """The product's MixedOP (on cuda) with the candidates -- kernel sizes included -- and the weights of the oracle cell ``o``."""
    from tfnas_amd.layers import MBInvertedResBlock
    from tfnas_amd.model_search import MixedOP
    op0 = o.m_ops[0]
    m = MixedOP(op0.in_channels, op0.out_channels, op0.stride, False, op0.act_func, 8, o.mc_num_dict, o.lat_lookup)
    for i, op in enumerate(o.m_ops):
        if m.m_ops[i].kernel_size != op.kernel_size:
            m.m_ops[i] = MBInvertedResBlock(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, op.kernel_size,
                                            op.stride, affine=False, act_func=op.act_func)
    m.load_state_dict(o.state_dict())
    m.set_temperature(o.T if T is None else T)
    return m.cuda()


def make_cell_pair(ic, oc, stride, act, mids, ks=SOFT_KS, seed=0):
    """_hipcheck.make_cell_pair with the candidates' kernel sizes replaced by ``ks`` on both sides (weights copied across)."""
    import _hipcheck as hc
    o, _ = hc.make_cell_pair(ic, oc, stride, act, mids, seed=seed)
    replace_oracle_ops(o, ks, seed)
    return o, hip_cell_like(o)


# ------------------------------------------------------------------------------------------------ cell_k7_*.npz
K7_CELL_NAMES = ['k7_s1_swish_res', 'k7_s2_relu_odd']
K7_CELLS = [
    # name, ic, oc, stride, act, H, W, B, mids (8)
    ('k7_s1_swish_res', 24, 24, 1, 'swish', 7, 10, 2, [29, 52, 28, 56, 37, 60, 40, 63]),
    ('k7_s2_relu_odd', 16, 24, 2, 'relu', 9, 13, 2, [24, 40, 20, 36, 29, 44, 24, 47]),
]
K7_SAMPLED = (4, 7)        # the sampled-mode candidates a fixture records (both 7 x 7: SE width ic and 2 * ic)


def cell_lut_for(fx):
    """The synthetic LUT of a cell_k7_*.npz fixture: _golden.cell_lut_for with the candidates' own kernel sizes (fx['ks'])."""
    ic, oc, s, H, W, B = [int(v) for v in fx['geom']]
    lut = {}
    for i, (mid, lat) in enumerate(zip(fx['mids'], fx['lats'])):
        key = 'MBInvertedResBlock_{}_{}_{}_{}_k{}_s{}_{}'.format(W, ic, ic * orc.OP_SE_MULT[i], oc, int(fx['ks'][i]), s,
                                                                str(fx['act']))
        lut.setdefault(key, {})[int(mid)] = float(lat)
    return lut


def oracle_cell_from(fx):
    """_golden.oracle_cell_from for a fixture whose candidates have the kernel sizes fx['ks']."""
    ic, oc, s, H, W, B = [int(v) for v in fx['geom']]
    mc = OrderedDict((i, int(m)) for i, m in enumerate(fx['mids']))
    cell = orc.MixedOP(ic, oc, s, str(fx['act']), mc, cell_lut_for(fx))
    replace_oracle_ops(cell, [int(k) for k in fx['ks']])
    cell.load_state_dict(OrderedDict((k[2:], torch.from_numpy(fx[k])) for k in fx.files if k.startswith('p.')))
    cell.set_temperature(float(fx['T']))
    return cell


# ------------------------------------------------------------------------------------------------ derived network
def base_network_config(num_classes):
    """A ``model.config`` of parsing.derived_config: two blocks per stage, SE and plain candidates (what the k7 / expand-free /
    fused configurations start from)."""
    from tfnas_amd import geometry as g, parsing
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 2))
                       for i, (st, bl) in enumerate(g.initial_mc_num_dddict().items()))
    return parsing.derived_config(arch, g.initial_mc_num_dddict(), num_classes)


def k7_network_config(num_classes=50):
    """base_network_config whose stage-3 and stage-5 blocks have depthwise kernel size 7."""
    cfg = base_network_config(num_classes)
    for st in ('stage3', 'stage5'):
        for blk in cfg[st]:
            blk['kernel_size'] = 7
    return cfg


def _hand_count(cfg, size, block_term, stem, head):
    """The stem, stage-loop and head arithmetic of both hand counters; ``block_term(kind, ic, mc, se, oc, k, hw_in, hw_out)`` is
    what one block adds, kind = 'fused' | 'noexp' | 'plain'.  Independent of parsing.py, whose counters it checks."""
    hw = (size - 1) // 2 + 1
    total = stem(hw)
    for st in ('stage1', 'stage2', 'stage3', 'stage4', 'stage5', 'stage6'):
        for c in cfg[st]:
            ic, mc, se, oc, k, s = (c[n] for n in ('in_channels', 'mid_channels', 'se_channels', 'out_channels', 'kernel_size',
                                                    'stride'))
            kind = 'fused' if c['name'] == 'FusedMBConvBlock' else ('plain' if mc > ic else 'noexp')
            hw_in, hw = hw, (hw - 1) // s + 1
            total += block_term(kind, ic, ic if kind == 'noexp' else mc, se, oc, k, hw_in, hw)
    ncls = cfg['classifier']['out_features']
    return (total + head(hw) + 1280 * ncls + ncls) / 1e6


def hand_macs_in_M(cfg, size):
    """Multiply-accumulates per image, in millions, of the network of ``cfg`` at ``size`` x ``size`` inputs, written out layer
    by layer (the conventions of the reference's flops counter: bias adds and the global average pool count, SE pooling does
    not)."""
    def block(kind, ic, mc, se, oc, k, hw_in, hw):
        lead = {'plain': ic * mc * hw_in * hw_in + k * k * mc * hw * hw,    # expand 1 x 1 at the input resolution + depthwise k x k
                'noexp': k * k * mc * hw * hw,                              # the depthwise alone, at the output resolution
                'fused': 9 * ic * mc * hw * hw}[kind]                       # one dense 3 x 3
        se_macs = 2 * mc * se + se + mc if se else 0                        # the two SE convolutions on the pooled vector, with bias
        return lead + se_macs + mc * oc * hw * hw                           # project 1 x 1

    def stem(hw):                                                           # 3 x 3 / 2, 3 -> 32; second stem: no expand, SE 8
        return 3 * 3 * 3 * 32 * hw * hw + 3 * 3 * 32 * hw * hw + (32 * 8 + 8) + (8 * 32 + 32) + 32 * 16 * hw * hw
    return _hand_count(cfg, size, block, stem, lambda hw: 320 * 1280 * hw * hw + 1280 * hw * hw)    # feature mix, average pool


def hand_params_in_MB(cfg):
    """Parameters of the network of ``cfg`` in millions, BatchNorm gamma / beta included, layer by layer."""
    def block(kind, ic, mc, se, oc, k, hw_in, hw):
        lead = {'plain': ic * mc + 2 * mc + k * k * mc + 2 * mc, 'noexp': k * k * mc + 2 * mc, 'fused': 9 * ic * mc + 2 * mc}[kind]
        return lead + (2 * mc * se + se + mc if se else 0) + mc * oc + 2 * oc

    def stem(hw):                                                           # first stem + its BatchNorm, second stem
        return 3 * 3 * 3 * 32 + 2 * 32 + 3 * 3 * 32 + 2 * 32 + (32 * 8 + 8) + (8 * 32 + 32) + 32 * 16 + 2 * 16
    return _hand_count(cfg, 224, block, stem, lambda hw: 320 * 1280 + 2 * 1280)
