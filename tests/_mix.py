"""Helpers shared by the tests of MixConv candidates (tests/test_mix_*.py, tests/test_gpu_mix*.py) and by the generator of their
fixture (tests/golden/make_golden_mix.py).

A MixConv block (Tan & Le, MixNet) is an MBConv whose depthwise convolution has its channels in two or three contiguous segments
of ascending kernel size -- 'k35': 3 x 3 | 5 x 5, 'k357': 3 x 3 | 5 x 5 | 7 x 7 -- with ONE packed 1-D weight, segment s stored as
[mc_s][k_s * k_s] (include/tfnas_hip.h: TFNAS_CELL_MIXK).  The CPU restatement is the oracle's own block.  ``mixed()`` wraps, in the
way ``_dil.dilated()`` wraps it, exactly one call of ``tfnas_oracle`` for its duration: the grouped ``F.conv2d`` of
``mbconv_forward`` -- the depthwise convolution.  Handed a packed (1-D) weight it becomes split -> grouped ``F.conv2d`` per segment
(padding ``k_s // 2``) -> cat (``mix_conv2d``); with any other weight the call is delegated with the arguments it came with.
Nothing else of the oracle is restated.  ``MixMBConv`` is ``orc.MBConv`` run inside ``mixed()`` whose ``depth_conv.conv`` is a
``PackedDW`` (the holder of the packed weight: the state_dict key stays ``depth_conv.conv.weight``); the oracle's ``DerivedBlock``
runs ``depth_conv.conv`` as a module, so there ``PackedDW.forward`` -- the same ``mix_conv2d`` -- is what runs.

The segment rule is written out here (``split``) from the issue's text, independently of the product's ``_lib.mix_split``."""
import contextlib
import itertools
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

import _dil
import _golden
import _k7
import _kinds
import _skip
import tfnas_oracle as orc
from _rawcell import KINK_TAU

K35, K357 = (3, 5), (3, 5, 7)
WORDS = {(3, 5): 0x53, (3, 7): 0x73, (5, 7): 0x75, (3, 5, 7): 0x753}


def split(mc, n):
    """Channels of the n segments of mc channels: q = ceil(mc / 4) quads, q // n each, the q % n remaining ones to segment 0;
    segment s = [4 Q_s, min(4 Q_s+1, mc))."""
    q = -(-mc // 4)
    assert q >= n
    quads = [q // n + (q % n if s == 0 else 0) for s in range(n)]
    ends = [min(4 * sum(quads[:s + 1]), mc) for s in range(n)]
    return [e - b for b, e in zip([0] + ends[:-1], ends)]


def packed_size(mc, ks):
    return sum(c * k * k for c, k in zip(split(mc, len(ks)), ks))


def segments(w, mc, ks):
    """views [mc_s, 1, k_s, k_s] of the packed weight ``w``"""
    out, o = [], 0
    for c, k in zip(split(mc, len(ks)), ks):
        out.append(w[o:o + c * k * k].view(c, 1, k, k))
        o += c * k * k
    assert o == w.numel()
    return out


def mix_conv2d(conv2d, x, w, ks, stride):
    """split -> grouped conv2d per segment (padding k_s // 2) -> cat"""
    mc = x.shape[1]
    cs = split(mc, len(ks))
    xs = torch.split(x, cs, dim=1)
    return torch.cat([conv2d(xi, wi, None, stride, k // 2, 1, c) for xi, wi, c, k in zip(xs, segments(w, mc, ks), cs, ks)], dim=1)


@contextlib.contextmanager
def mixed(ks):
    """tfnas_oracle's depthwise convolution (the one grouped F.conv2d call of mbconv_forward), handed a packed 1-D weight, runs
    as mix_conv2d over the kernel sizes ``ks``; yields how many calls were rewritten so far (a one-element list)."""
    F0 = orc.F
    hits = [0]

    def conv2d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
        if w.dim() == 1:
            assert bias is None and dilation == 1 and groups == w.shape[0]       # (the depthwise call, as mbconv_forward makes it)
            hits[0] += 1
            return mix_conv2d(F0.conv2d, x, w, ks, stride)
        return F0.conv2d(x, w, bias, stride, padding, dilation, groups)
    orc.F = _dil._Proxy(F0, conv2d=conv2d)
    try:
        yield hits
    finally:
        orc.F = F0


class PackedDW(nn.Module):
    """Holder of the packed depthwise weight of a restatement block (``weight``: 1-D), every segment initialised as nn.Conv2d
    initialises a depthwise convolution of its size; ``forward`` is mix_conv2d (what a DerivedBlock runs)."""

    def __init__(self, mc, ks, stride):
        super().__init__()
        self.channels, self.kernels, self.stride = mc, tuple(ks), stride
        self.weight = nn.Parameter(torch.empty(packed_size(mc, ks)))
        with torch.no_grad():
            for w in segments(self.weight, mc, ks):
                nn.init.kaiming_uniform_(w, a=math.sqrt(5))

    def forward(self, x):
        return mix_conv2d(torch.nn.functional.conv2d, x, self.weight, self.kernels, self.stride)


class MixMBConv(orc.MBConv):
    mix_kernels = None

    def forward(self, x, detail=None):
        with mixed(self.mix_kernels):
            return super().forward(x, detail)


def mixify(block, ks):
    """``block`` (an oracle MBConv or DerivedBlock of kernel size max(ks)) as a MixConv block of kernel sizes ``ks``, in place: a
    fresh packed weight under torch's current seed; returns it."""
    ks = tuple(ks)
    assert ks in WORDS and block.kernel_size == max(ks)
    if isinstance(block, orc.MBConv):
        block.__class__ = MixMBConv
    elif not isinstance(block, orc.DerivedBlock):
        raise TypeError(type(block))
    dw = PackedDW(block.mid_channels, ks, block.stride)
    old = block.depth_conv.conv
    block.depth_conv.conv = dw.to(old.weight.dtype)
    block.mix_kernels = ks
    return block


def mix_of(block):
    return getattr(block, 'mix_kernels', None)


def mix_block(cls, ic, mc, se, oc, ks, stride, act):
    return mixify(cls(ic, mc, se, oc, max(ks), stride, act), ks)


class KTag(int):
    """A kernel size that FORMATS as the latency tables spell a MixConv kernel ('35', so that 'k{}' gives 'k35') and is the plain
    integer -- the largest kernel size -- everywhere else (_dil.KTag is the pattern)."""

    def __new__(cls, ks):
        self = int.__new__(cls, max(ks))
        self.ks = tuple(ks)
        return self

    def __format__(self, spec):
        return ''.join('%d' % k for k in self.ks)

    def __deepcopy__(self, memo):
        return KTag(self.ks)


# ------------------------------------------------------------------------------------------------ oracle pin (blocks)
# 2 x 16 x 9 x 13, out 16 (residual at stride 1): both strides x SE and none x k35 and k357, in both forms; then a ragged width
# (mid 53 -> 24 | 16 | 13 and 24 | 29... see split) and an expand-free block
PIN_GEOM = dict(N=2, ic=16, oc=16, H=9, W=13)
PIN_CASES = [(ks, s, act, se, 44) for ks, s, (act, se) in
             itertools.product((K35, K357), (1, 2), (('swish', 8), ('relu', 0)))]
PIN_EXTRA = [(K357, 1, 'swish', 8, 53), (K35, 2, 'relu', 0, 53), (K357, 2, 'swish', 8, 16), (K35, 1, 'relu', 8, 16)]
PIN_FORMS = ('search', 'derived')
PIN_DROP = _k7.PIN_DROP


def pin_cases(form):
    return PIN_CASES + PIN_EXTRA


def pin_tag(form, case):
    ks, s, act, se, mid = case
    return '%s_k%s_s%d_%s_se%d_m%d' % (form, ''.join(map(str, ks)), s, act, se, mid)


def pin_oracle_block(form, case):
    """The restatement block of one pin case (float64) with seeded weights, its input, cotangent and RNG seed."""
    ks, s, act, se, mid = case
    q = PIN_GEOM
    every = PIN_CASES + PIN_EXTRA
    seed = 11000 + 83 * every.index(case) + (0 if form == 'search' else 41)
    torch.manual_seed(seed)
    cls = orc.MBConv if form == 'search' else orc.DerivedBlock
    blk = mix_block(cls, q['ic'], mid, se, q['oc'], ks, s, act)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.dim() == 1 and 'depth_conv' not in n and '.bn.' not in n:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))      # SE biases
    if form == 'derived':
        _k7.randomise_bn(blk, gen)
        blk.drop_connect_rate = PIN_DROP
    blk = blk.double().train()
    x = torch.randn(q['N'], q['ic'], q['H'], q['W'], generator=gen).double()
    r = torch.randn(q['N'], q['oc'], (q['H'] - 1) // s + 1, (q['W'] - 1) // s + 1, generator=gen).double()
    rng = seed + 2
    if form == 'derived' and s == 1:
        while True:             # (the first draw that keeps one image and drops the other: _dil.pin_oracle_block)
            torch.manual_seed(rng)
            kept = torch.floor(1.0 - PIN_DROP + torch.rand((q['N'], 1, 1, 1), dtype=x.dtype)).view(-1)
            if 0 < float(kept.sum()) < q['N']:
                break
            rng += 1000
    return blk, x, r, rng


pin_run = _k7.pin_run           # forward + backward: out, dx, every parameter gradient, the buffers
pin_record = _k7.pin_record      # what the fixture keeps: the depthwise weight gradient whole, _golden.probe of the rest


# ------------------------------------------------------------------------------------------------ oracle cells (plain MBConv)
# a candidate spec: an int (a plain kernel size), (k, 2) (dilated), or a tuple of 2-3 ascending kernel sizes (MixConv)
SOFT = (3, K35, 5, 7, K35, K357, (3, 2), K357)      # SE on the last four, as in every oracle MixedOP: k35_se, k357_se, k3d2_se, k357_se
MIX_IDX = (1, 4, 5, 7)


def is_mix(spec):
    return isinstance(spec, tuple) and spec in WORDS


def spec_k(spec):
    return spec if isinstance(spec, int) else (max(spec) if is_mix(spec) else spec[0])


def replace_oracle_ops(o, specs, seed=0):
    """candidate i of the oracle cell becomes ``specs[i]``: _k7.replace_oracle_ops for the kernel sizes, then dilations and
    MixConv segments (fresh seeded packed weights)"""
    _k7.replace_oracle_ops(o, [spec_k(s) for s in specs], seed)
    for i, s in enumerate(specs):
        if is_mix(s):
            torch.manual_seed(5100 + 17 * i + seed)
            mixify(o.m_ops[i], s)
        elif not isinstance(s, int):
            _dil.dilate(o.m_ops[i], s[1])
    return o


def hip_cell_like(o, T=None):
    """The product's MixedOP (on cuda) with the candidates -- kernel sizes, dilations and MixConv segments -- and weights of ``o``."""
    from tfnas_amd.layers import MBInvertedResBlock
    from tfnas_amd.model_search import MixedOP
    op0 = o.m_ops[0]
    m = MixedOP(op0.in_channels, op0.out_channels, op0.stride, False, op0.act_func, 8, o.mc_num_dict, o.lat_lookup)
    for i, op in enumerate(o.m_ops):
        if m.m_ops[i].kernel_size != op.kernel_size or _dil.dilation_of(op) != 1 or mix_of(op) is not None:
            m.m_ops[i] = MBInvertedResBlock(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, int(op.kernel_size),
                                            op.stride, affine=False, act_func=op.act_func, dilation=_dil.dilation_of(op),
                                            mix_kernels=mix_of(op))
    m.load_state_dict(o.state_dict())
    m.set_temperature(o.T if T is None else T)
    return m.cuda()


def make_cell_pair(ic, oc, stride, act, mids, specs=SOFT, seed=0):
    import _hipcheck as hc
    o, _ = hc.make_cell_pair(ic, oc, stride, act, mids, seed=seed)
    replace_oracle_ops(o, specs, seed)
    return o, hip_cell_like(o)


# ------------------------------------------------------------------------------------------------ cells of several kinds
# candidates as in _kinds / _skip; ``mixes[g]``: None or the kernel sizes of candidate g (its k is then max of them)
def make_ref(cands, mixes, ic, oc, stride, act, seed):
    o = _skip.make_ref(cands, ic, oc, stride, act, seed)
    for g, (op, ks) in enumerate(zip(o.m_ops, mixes)):
        if ks is not None:
            torch.manual_seed(seed + 31 * (g + 1))
            mixify(op, ks)
    o.mixes = tuple(mixes)
    return o


def case_data(cands, mixes, N, ic, oc, H, W, stride, act, base=300):
    """_kinds.case_data for MixConv candidates: the first seed from ``base`` up whose float64 pre-activations of every candidate
    stay KINK_TAU from every kink (swish takes ``base``) -- no element is ever exempted from a comparison."""
    for seed in range(base, base + 200):
        o = make_ref(cands, mixes, ic, oc, stride, act, seed)
        gen = torch.Generator().manual_seed(seed + 2)
        x = torch.randn(N, ic, H, W, generator=gen)
        r = torch.randn(N, oc, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
        w = torch.softmax(torch.randn(len(cands), generator=gen), -1)
        if _kinds.kink_distance(o, x) >= KINK_TAU:
            return o, x, r, w, seed
    raise AssertionError('no seed keeps the pre-activations clear of the kinks')


def hip_blocks_like(o):
    """_dil.hip_blocks_like with every MBInvertedResBlock given its candidate's MixConv segments"""
    import _fused
    from tfnas_amd.layers import FusedMBConvBlock, IdentityLayer, MBInvertedResBlock
    out = []
    for op in o.m_ops:
        if isinstance(op, _skip.IdentityRef):
            out.append(IdentityLayer(op.in_channels, op.out_channels))
            continue
        if isinstance(op, _fused.FusedRef):
            m = FusedMBConvBlock(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, 3, op.stride, affine=False,
                                 act_func=o.act_func)
        else:
            m = MBInvertedResBlock(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, int(op.kernel_size), op.stride,
                                   affine=False, act_func=o.act_func, dilation=_dil.dilation_of(op), mix_kernels=mix_of(op))
        m.load_state_dict(op.state_dict())
        out.append(m.cuda())
    return out


def hip_plan(o):
    return _kinds.hip_plan(o, hip_blocks_like(o))


# ------------------------------------------------------------------------------------------------ derived network
MIX_STAGES = OrderedDict([('stage4', (K35, K357)), ('stage5', (K357, K35))])


def mix_network_config(num_classes=20):
    """_k7.base_network_config whose stage-4 and stage-5 blocks are MixConv blocks"""
    cfg = _k7.base_network_config(num_classes)
    for st, kss in MIX_STAGES.items():
        for blk, ks in zip(cfg[st], kss):
            blk['kernel_size'], blk['mix_kernels'] = max(ks), list(ks)
    return cfg


def mix_network(net):
    """the oracle DerivedNetwork's stage-4 / stage-5 blocks rebuilt as MixConv blocks (fresh seeded weights)"""
    for st, kss in MIX_STAGES.items():
        blocks = getattr(net, st)
        for i, ks in enumerate(kss):
            b = blocks[i]
            torch.manual_seed(4700 + 10 * int(st[-1]) + i)
            nb = mix_block(orc.DerivedBlock, b.in_channels, b.mid_channels, b.se_channels, b.out_channels, ks, b.stride, b.act_func)
            nb.drop_connect_rate = b.drop_connect_rate
            blocks[i] = nb
    return net


def randomise_packed(mod, gen):
    """_affineref.randomise reaches nn.Conv2d modules only: the packed depthwise weights ~ N(0, 1 / fan_in) per segment"""
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, PackedDW):
                for w in segments(m.weight, m.channels, m.kernels):
                    w.copy_(torch.randn(w.shape, generator=gen) * w[0].numel() ** -0.5)


def record(res):
    return OrderedDict((k, _golden.probe(torch.from_numpy(np.asarray(v)))) for k, v in res.items())
