"""Helpers shared by the tests of dilated depthwise candidates (tests/test_dil_*.py, tests/test_gpu_dil*.py) and by the generator
of their fixture (tests/golden/make_golden_dil.py).

The CPU restatement is the oracle's own block.  ``dilated(d)`` wraps, in the way ``_sestyle.styled()`` and
``_acts.wrapped_oracle()`` wrap theirs, exactly one call of ``tfnas_oracle`` for its duration: the grouped ``F.conv2d`` of
``mbconv_forward`` -- the depthwise convolution -- is given ``padding = d * (k // 2)`` and ``dilation = d``.  Nothing else of the
oracle is restated, and with dilation 1 the call is delegated with the arguments it came with.  ``DilMBConv`` is ``orc.MBConv``
run inside ``dilated(self.dilation)``; the oracle's ``DerivedBlock`` runs its depthwise convolution through its own ``nn.Conv2d``
module, so ``dilate()`` sets that module's padding and dilation (the weight, and every state_dict key, stay).  ``dilate(block, d)``
turns an existing oracle block into its dilated twin in place, ``dilate_network`` the blocks of an oracle ``DerivedNetwork``."""
import contextlib
import itertools
from collections import OrderedDict

import numpy as np
import torch

import _golden
import _k7
import _kinds
import tfnas_oracle as orc
from _rawcell import KINK_TAU

PAIRS = ((3, 2), (5, 2))                # the (kernel size, dilation) pairs the library takes


class _Proxy:
    """A module whose attributes are ``base``'s except the ones given"""

    def __init__(self, base, **over):
        self.__dict__.update(over)
        self._base = base

    def __getattr__(self, name):
        return getattr(self._base, name)


@contextlib.contextmanager
def dilated(d):
    """tfnas_oracle's depthwise convolution (the one grouped F.conv2d call of mbconv_forward) runs with padding d * (k // 2) and
    dilation d; yields how many calls were rewritten so far (a one-element list)."""
    F0 = orc.F
    hits = [0]

    def conv2d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
        if d != 1 and groups > 1 and groups == w.shape[0] and w.shape[1] == 1:
            hits[0] += 1
            return F0.conv2d(x, w, bias, stride, d * (w.shape[-1] // 2), d, groups)
        return F0.conv2d(x, w, bias, stride, padding, dilation, groups)
    orc.F = _Proxy(F0, conv2d=conv2d)
    try:
        yield hits
    finally:
        orc.F = F0


class DilMBConv(orc.MBConv):
    dilation = 1

    def forward(self, x, detail=None):
        with dilated(self.dilation):
            return super().forward(x, detail)


def dilate(block, d):
    """``block`` (an oracle MBConv or DerivedBlock) with its depthwise taps ``d`` pixels apart, in place; returns it."""
    assert d in (1, 2)
    k = block.kernel_size
    if isinstance(block, orc.MBConv):
        block.__class__ = DilMBConv
    elif not isinstance(block, orc.DerivedBlock):
        raise TypeError(type(block))
    conv = block.depth_conv.conv       # (DerivedBlock runs this module; for an MBConv it only keeps the record straight)
    conv.padding, conv.dilation = (d * (k // 2),) * 2, (d, d)
    block.dilation = d
    return block


def dilation_of(block):
    return getattr(block, 'dilation', 1)


class KTag(int):
    """A kernel size that FORMATS as the latency tables spell a dilated kernel ('3d2', so that 'k{}' gives 'k3d2') and is the
    plain integer everywhere else.  Given to a dilated restatement block inside an oracle MixedOP / Network, it lets the oracle's
    own get_lookup_latency -- which writes 'k{}'.format(op.kernel_size) -- ask the table for the dilated block's key, the key the
    product asks for (tests/test_dil_abi.py pins its text)."""

    def __new__(cls, k, d):
        self = int.__new__(cls, k)
        self.d = d
        return self

    def __format__(self, spec):
        return int.__format__(int(self), spec) + ('' if self.d == 1 else 'd%d' % self.d)

    def __deepcopy__(self, memo):
        return KTag(int(self), self.d)


# ------------------------------------------------------------------------------------------------ oracle pin (blocks)
# 2 x 16 x 9 x 13, out 16 (residual at stride 1).  Per (k, d) pair and stride a half factorial of activation x SE x expand, in both
# forms; then the image sizes at which the reference's block was checked to run with a dilated depth_conv: 1 x 1, 3 x 5 (smaller
# than both extents) and 12 x 10 at stride 2 (even), search form, dilated 5 x 5.
PIN_GEOM = dict(N=2, ic=16, oc=16, H=9, W=13, se=8)
PIN_MIX = (('relu', 0, 24), ('swish', 8, 24), ('relu', 8, 16), ('swish', 0, 16))          # (act, se, mid): mid 16 = no expand
PIN_CASES = [(k, d, s, act, se, mid, PIN_GEOM['N'], PIN_GEOM['H'], PIN_GEOM['W'])
             for (k, d), s, (act, se, mid) in itertools.product(PAIRS, (1, 2), PIN_MIX)]
PIN_EXTRA = [(5, 2, 1, 'swish', 8, 24, 3, 1, 1), (5, 2, 1, 'relu', 8, 24, 2, 3, 5), (5, 2, 2, 'swish', 8, 24, 2, 12, 10),
             (3, 2, 2, 'relu', 0, 16, 2, 12, 10)]
PIN_FORMS = ('search', 'derived')
PIN_DROP = _k7.PIN_DROP


def pin_cases(form):
    return PIN_CASES + (PIN_EXTRA if form == 'search' else [])


def pin_tag(form, case):
    return '%s_k%dd%d_s%d_%s_se%d_m%d_n%d_%dx%d' % ((form,) + tuple(case))


def pin_oracle_block(form, case, dilation=None):
    """The oracle's block of one pin case (float64, dilated as the case says, or by ``dilation``) with seeded weights, its
    input, cotangent and RNG seed."""
    k, d, s, act, se, mid, N, H, W = case
    q = PIN_GEOM
    every = PIN_CASES + PIN_EXTRA
    seed = 7000 + 83 * every.index(case) + (0 if form == 'search' else 41)
    torch.manual_seed(seed)
    cls = orc.MBConv if form == 'search' else orc.DerivedBlock
    blk = cls(q['ic'], mid, se, q['oc'], k, s, act)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))      # SE biases
    if form == 'derived':
        _k7.randomise_bn(blk, gen)
        blk.drop_connect_rate = PIN_DROP
    blk = dilate(blk.double().train(), d if dilation is None else dilation)
    x = torch.randn(N, q['ic'], H, W, generator=gen).double()
    r = torch.randn(N, q['oc'], (H - 1) // s + 1, (W - 1) // s + 1, generator=gen).double()
    rng = seed + 2
    if form == 'derived' and s == 1:
        # the residual block's drop-connect draws come from torch's generator under this seed (_k7.pin_run): take the first one
        # that keeps one image and drops the other -- with both dropped the block is the identity and pins nothing
        while True:
            torch.manual_seed(rng)
            kept = torch.floor(1.0 - PIN_DROP + torch.rand((N, 1, 1, 1), dtype=x.dtype)).view(-1)
            if 0 < float(kept.sum()) < N:
                break
            rng += 1000
    return blk, x, r, rng


pin_run = _k7.pin_run           # forward + backward: out, dx, every parameter gradient, the buffers
pin_record = _k7.pin_record      # what the fixture keeps: the depthwise weight gradient whole, _golden.probe of the rest


# ------------------------------------------------------------------------------------------------ oracle cells (plain MBConv)
SOFT = ((3, 1), (3, 2), (5, 1), (5, 2), (7, 1), (3, 2), (5, 2), (5, 2))      # (k, d) of the eight candidates of the mixed cell: SE on
                                                                             # the last four, as in every oracle MixedOP


def replace_oracle_ops(o, kds, seed=0):
    """_k7.replace_oracle_ops (kernel sizes), then dilations: candidate i of the oracle cell gets (k, d) = kds[i]"""
    _k7.replace_oracle_ops(o, [k for k, _ in kds], seed)
    for i, (_, d) in enumerate(kds):
        if d != 1:
            dilate(o.m_ops[i], d)
    return o


def hip_cell_like(o, T=None):
    """The product's MixedOP (on cuda) with the candidates -- kernel sizes and dilations included -- and weights of ``o``."""
    from tfnas_amd.layers import MBInvertedResBlock
    from tfnas_amd.model_search import MixedOP
    op0 = o.m_ops[0]
    m = MixedOP(op0.in_channels, op0.out_channels, op0.stride, False, op0.act_func, 8, o.mc_num_dict, o.lat_lookup)
    for i, op in enumerate(o.m_ops):
        if m.m_ops[i].kernel_size != op.kernel_size or dilation_of(op) != 1:
            m.m_ops[i] = MBInvertedResBlock(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, op.kernel_size,
                                            op.stride, affine=False, act_func=op.act_func, dilation=dilation_of(op))
    m.load_state_dict(o.state_dict())
    m.set_temperature(o.T if T is None else T)
    return m.cuda()


def make_cell_pair(ic, oc, stride, act, mids, kds=SOFT, seed=0):
    """_hipcheck.make_cell_pair with the candidates' (kernel size, dilation) replaced by ``kds`` on both sides"""
    import _hipcheck as hc
    o, _ = hc.make_cell_pair(ic, oc, stride, act, mids, seed=seed)
    replace_oracle_ops(o, kds, seed)
    return o, hip_cell_like(o)


# ------------------------------------------------------------------------------------------------ cells of several kinds
def make_ref(cands, dils, ic, oc, stride, act, seed):
    """_skip.make_ref (the weighted sum of restatement blocks of any kind, ('S',) = the identity candidate) with candidate g
    dilated by dils[g]"""
    import _skip
    o = _skip.make_ref(cands, ic, oc, stride, act, seed)
    for op, d in zip(o.m_ops, dils):
        if d != 1:
            dilate(op, d)
    o.dils = tuple(dils)
    return o


def case_data(cands, dils, N, ic, oc, H, W, stride, act, base=300):
    """_kinds.case_data for dilated candidates: the first seed from ``base`` up whose float64 pre-activations of every candidate
    stay KINK_TAU from every kink (swish takes ``base``) -- no element is ever exempted from a comparison."""
    for seed in range(base, base + 200):
        o = make_ref(cands, dils, ic, oc, stride, act, seed)
        gen = torch.Generator().manual_seed(seed + 2)
        x = torch.randn(N, ic, H, W, generator=gen)
        r = torch.randn(N, oc, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
        w = torch.softmax(torch.randn(len(cands), generator=gen), -1)
        if _kinds.kink_distance(o, x) >= KINK_TAU:
            return o, x, r, w, seed
    raise AssertionError('no seed keeps the pre-activations clear of the kinks')


def hip_blocks_like(o):
    """_kinds.hip_blocks_like with every MBInvertedResBlock given its candidate's dilation"""
    import _fused
    import _skip
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
            m = MBInvertedResBlock(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, op.kernel_size, op.stride,
                                   affine=False, act_func=o.act_func, dilation=dilation_of(op))
        m.load_state_dict(op.state_dict())
        out.append(m.cuda())
    return out


def hip_plan(o):
    return _kinds.hip_plan(o, hip_blocks_like(o))


# pin of the mix: the reference's MixedOP.forward over replaced candidates (tests/golden/make_golden_dil.py), in float64
MIX_CANDS = [('M', 22, 3, 0), ('M', 30, 5, 8), ('N', 3, 0), ('M', 24, 3, 8), ('N', 5, 8), ('M', 28, 5, 0), ('M', 20, 7, 0), ('N', 3, 8)]
MIX_DILS = (2, 1, 2, 1, 2, 2, 1, 1)
MIX_CASES = [('swish', 1), ('relu', 2)]


def mix_tag(case):
    return 'mix_%s_s%d' % case


def mix_case(case):
    """_kinds.pin_case for the dilated mix: restatement (float64), input, cotangent, log_alphas, the noise seed"""
    act, s = case
    N, ic, oc, H, W = _kinds.SMALL_SHAPE
    seed = 9500 + 97 * MIX_CASES.index(case)
    o = make_ref(MIX_CANDS, MIX_DILS, ic, oc if s == 1 else 12, s, act, seed).double()
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(N, ic, H, W, generator=gen).double()
    r = torch.randn(N, o.out_channels, (H - 1) // s + 1, (W - 1) // s + 1, generator=gen).double()
    la = torch.log_softmax(0.5 * torch.randn(len(MIX_CANDS), generator=gen), -1).double()
    return o, x, r, la, seed + 3


# ------------------------------------------------------------------------------------------------ derived network
DIL_STAGE5 = ((5, 2), (3, 2))          # (k, dilation) of the two stage-5 blocks of dil_network_config


def dil_network_config(num_classes=20):
    """_k7.base_network_config whose two stage-5 blocks are dilated (a dilated 5 x 5 at stride 2, a dilated 3 x 3 residual)"""
    cfg = _k7.base_network_config(num_classes)
    for blk, (k, d) in zip(cfg['stage5'], DIL_STAGE5):
        blk['kernel_size'], blk['dilation'] = k, d
    return cfg


def dilate_network(net, stage='stage5', kds=DIL_STAGE5):
    """the oracle DerivedNetwork's blocks of ``stage`` rebuilt with (k, d) = kds (fresh seeded weights where k changes)"""
    blocks = getattr(net, stage)
    for i, (k, d) in enumerate(kds):
        b = blocks[i]
        if b.kernel_size != k:
            torch.manual_seed(4300 + i)
            nb = orc.DerivedBlock(b.in_channels, b.mid_channels, b.se_channels, b.out_channels, k, b.stride, b.act_func)
            nb.drop_connect_rate = b.drop_connect_rate
            blocks[i] = b = nb
        dilate(b, d)
    return net


def record(res):
    return OrderedDict((k, _golden.probe(torch.from_numpy(np.asarray(v)))) for k, v in res.items())
