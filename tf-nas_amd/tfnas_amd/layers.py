"""Layer library with the reference's class / attribute / parameter names (models/layers.py).

Only what the search hot path touches is provided:
  MBInvertedResBlock  (models/layers.py:431-561)  -- parameter container with the reference's sub-module names
                      (``inverted_bottleneck.conv``, ``depth_conv.conv``, ``squeeze_excite.conv_reduce/conv_expand``,
                      ``point_linear.conv``) so that train_search.py:164-193's ``exec`` weight slicing and the
                      state_dict keys (:244-258) keep working.  Its arithmetic runs in the HIP library.
  FusedMBConvBlock    (no counterpart in the reference) -- the Fused-MBConv block of EfficientNetV2 / MobileNet-EdgeTPU / MnasNet:
                      one dense 3x3 convolution in place of the 1x1 expand plus the depthwise; sub-modules ``fused_conv.conv``,
                      ``squeeze_excite.conv_reduce/conv_expand``, ``point_linear.conv``.
  ConvLayer / LinearLayer (models/layers.py:190-271, :322-428) -- parameter containers of the stems and the head; inside
                      Network they run as HIP cells (TFNAS_MODE_STEM / _HEAD), the classifier is an nn.Linear.
  IdentityLayer       (models/layers.py:274-319) -- the skip candidate of a residual cell and the skipped block of a derived
                      network: no parameters, ``forward(x)`` is ``x``.
  Swish               (models/layers.py:26-35)
BatchNorm of the search net has no affine and no running statistics (layers.py:101-103,469,498,533): it is
a pure function of the batch and therefore has no module/state here.
"""
from collections import OrderedDict
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import act_id, se_style_id, check_mix_kernels, mix_split, MBCONV, NOEXPAND, FUSED
from .functions import CellPlan, MixedOpFn, BN_EPS


class Swish(nn.Module):
    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = inplace

    def forward(self, x):
        return x.mul_(x.sigmoid()) if self.inplace else x * x.sigmoid()


def get_same_padding(kernel_size):
    assert kernel_size % 2 > 0, 'kernel size should be odd number'
    return kernel_size // 2


class ConvLayer(nn.Module):
    """conv -> BN -> act of the stems / head: the parameter container (the arithmetic runs in Network's stem / head HIP cells)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, affine=False, act_func='relu'):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.act_func = kernel_size, stride, act_func
        self.affine = affine
        if affine:           # derived network (models/model_eval.py): BatchNorm2d(affine, running stats); registered before
            self.bn = nn.BatchNorm2d(out_channels, affine=True, track_running_stats=True)      # conv, like BasicLayer
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, get_same_padding(kernel_size),
                              bias=False)

    @property
    def name(self):
        return 'ConvLayer'

    def forward(self, x):
        # Inside Network (search and derived) the stems and the feature-mix head run as HIP cells (TFNAS_MODE_STEM / _HEAD:
        # model_search.Network._stem / _head, model_eval._DerivedBase); this module is their parameter container.  There is
        # deliberately NO stock-torch body here: a caller invoking the layer on its own would silently get MIOpen / rocBLAS
        # arithmetic instead of the HIP path.
        raise RuntimeError('tfnas_amd: ConvLayer runs only as part of Network (stem / head HIP cells: Network._stem, '
                           'Network._head); it has no standalone forward')


class LinearLayer(nn.Module):
    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.linear = nn.Linear(in_features, out_features, bias)

    @property
    def name(self):
        return 'LinearLayer'

    def forward(self, x):
        return self.linear(x)


class IdentityLayer(nn.Module):
    """The reference's IdentityLayer (models/layers.py:274-319) as it stands in a MixedOP: no parameters, no buffers, ``forward``
    returns its input itself.  As a candidate of a residual cell it is the library's TFNAS_GROUP_SKIP group (a mix weight that adds
    to the residual term, nothing else); it has no ``kind`` (_lib.BlockKind) because it binds no field and has no BatchNorm site."""

    kind = None
    mid_channels = se_channels = kernel_size = 0       # (what a TfnasGroup of it holds)
    stride = 1
    act_func = None

    def __init__(self, in_channels, out_channels, use_bn=False, affine=False, act_func=None, ops_order='weight_bn_act'):
        super().__init__()
        if use_bn or affine or act_func is not None or ops_order != 'weight_bn_act':
            raise NotImplementedError('tfnas_amd: IdentityLayer is the plain identity (no BatchNorm, no activation)')
        self.in_channels, self.out_channels = in_channels, out_channels

    @property
    def name(self):
        return 'IdentityLayer'

    @property
    def config(self):
        return {'name': 'IdentityLayer', 'in_channels': self.in_channels, 'out_channels': self.out_channels,
                'use_bn': False, 'affine': False, 'act_func': None, 'ops_order': 'weight_bn_act'}

    def forward(self, x):
        return x

    def hip_params(self):
        return []

    def set_se_style(self, style):
        """No squeeze-excite branch: a style never conflicts with it."""


def _seq(**mods):
    return nn.Sequential(OrderedDict(mods))


class MixDepthwiseConv2d(nn.Module):
    """The depthwise convolution of a MixConv block (Tan & Le, MixNet): the channels in two or three contiguous segments, segment s
    a depthwise ``kernels[s]`` x ``kernels[s]`` convolution (padding ``k // 2``, no bias).  ONE 1-D parameter ``weight`` holds the
    segments back to back, segment s as [mc_s][k_s * k_s] -- the packed w_dw of a TFNAS_CELL_MIXK group (include/tfnas_hip.h), so
    the state_dict key stays ``...depth_conv.conv.weight``.  ``segment_weights()`` are its views [mc_s, 1, k_s, k_s];
    ``splits`` the segment widths (_lib.mix_split).  ``forward`` is the stock-torch CPU form (split -> grouped conv2d per segment
    -> cat): inside a block the HIP library runs it, this is what a test or an export compares with."""

    def __init__(self, channels, kernels, stride=1):
        super().__init__()
        self.kernels = check_mix_kernels(kernels)
        self.channels, self.stride = channels, stride
        self.splits = mix_split(channels, len(self.kernels))
        self.weight = nn.Parameter(torch.empty(sum(c * k * k for c, k in zip(self.splits, self.kernels))))
        self.bias = None
        self.reset_parameters()

    def segment_weights(self, weight=None):
        w = self.weight if weight is None else weight
        out, o = [], 0
        for c, k in zip(self.splits, self.kernels):
            out.append(w[o:o + c * k * k].view(c, 1, k, k))
            o += c * k * k
        return out

    def reset_parameters(self):
        """Every segment as nn.Conv2d initialises a depthwise convolution of its size (the networks' _initialization leaves
        convolution weights at that default)."""
        with torch.no_grad():
            for w in self.segment_weights():
                nn.init.kaiming_uniform_(w, a=math.sqrt(5))

    def forward(self, x):
        xs = torch.split(x, self.splits, dim=1)
        return torch.cat([F.conv2d(xi, w, None, self.stride, k // 2, 1, c)
                          for xi, w, c, k in zip(xs, self.segment_weights(), self.splits, self.kernels)], dim=1)

    def extra_repr(self):
        return '%d, kernels=%r, splits=%r, stride=%d' % (self.channels, self.kernels, self.splits, self.stride)


class _HipBlock(nn.Module):
    """What the blocks that run as ONE cell of the HIP library share: everything after the leading convolutions (squeeze-excite,
    the project convolution, the residual), the parameter / BatchNorm lists in the order of the library's fields, the launch
    (search form through ``tfnas_mixedop_fwd``, ``affine=True`` through ``tfnas_mbconv_fwd``) and drop-connect.  A subclass
    validates its arguments, registers its leading convolution modules through ``lead(mid_channels)`` (an ordered
    {name: module or None}) and names its ``kind`` (_lib.BlockKind: which fields and BatchNorm sites such a cell has)."""

    kind = MBCONV

    def __init__(self, in_channels, mid_channels, se_channels, out_channels, kernel_size, stride, affine, act_func, lead,
                 se_act=None, se_gate='sigmoid'):
        super().__init__()
        act_id(act_func)                                   # (ValueError for a name the library has no kernels for)
        se_style_id(se_act, se_gate)                       # (... or a squeeze-excite style it has none for)
        # squeeze-excite style (TfnasCellDesc.se_style): hidden activation (None: act_func) and gate of the SE branch; plain
        # attributes -- no parameter, module or state_dict key depends on them.  MobileNetV3: ('relu', 'h-sigmoid').  (What the
        # hard-sigmoid gate costs beside the logistic one on the chip has not been measured; the latency tables ignore the style.)
        self.se_act, self.se_gate = se_act, se_gate
        self.in_channels, self.mid_channels = in_channels, mid_channels
        self.se_channels, self.out_channels = max(se_channels, 0), out_channels
        self.kernel_size, self.stride, self.act_func = kernel_size, stride, act_func
        self.affine = affine
        self.drop_connect_rate = 0.0
        leading = lead(mid_channels)
        for name, mod in leading.items():
            setattr(self, name, mod)
        if se_channels > 0:
            self.squeeze_excite = _seq(conv_reduce=nn.Conv2d(mid_channels, se_channels, 1, 1, 0, bias=True),
                                       conv_expand=nn.Conv2d(se_channels, mid_channels, 1, 1, 0, bias=True))
        else:
            self.squeeze_excite = None
        self.point_linear = _seq(conv=nn.Conv2d(mid_channels, out_channels, 1, 1, 0, bias=False), **self.bn(out_channels))
        self.has_residual = (in_channels == out_channels) and (stride == 1)
        # the conv (+ bn) modules in the order of the library's fields: the leading ones that are there, then the project
        self._convs = [m for m in leading.values() if m is not None] + [self.point_linear]
        self._plan = None

    def set_se_style(self, style):
        """Give the block the squeeze-excite style ``(se_act, se_gate)`` (None: the default) -- before its first forward: the
        plan of a launch reads the style when it is made."""
        from ._lib import se_style_pair
        self.se_act, self.se_gate = se_style_pair(style)
        self._plan = None

    def bn(self, ch):
        """affine=True: the derived network's BatchNorm2d(affine, running statistics), layers.py:468,497,533"""
        return dict(bn=nn.BatchNorm2d(ch, affine=True, track_running_stats=True)) if self.affine else {}

    def forward(self, x):
        if self._plan is None:
            self._plan = CellPlan(self.in_channels, self.out_channels, self.stride, self.act_func, [self])
        if self.affine:
            return self._affine_forward(x)
        return MixedOpFn.apply(self._plan, x, None, *self.hip_params())

    def hip_params(self):
        """Weights in the order of the TfnasGroup pointer fields this kind binds."""
        ps = [m.conv.weight for m in self._convs]
        se = self.squeeze_excite
        if se is not None:
            ps += [se.conv_reduce.weight, se.conv_reduce.bias, se.conv_expand.weight, se.conv_expand.bias]
        return ps

    def bn_modules(self):
        """The block's BatchNorm modules in order (affine form): one per BatchNorm site of its kind."""
        return [m.bn for m in self._convs]

    def bn_sites(self):
        """The three BatchNorm sites of the cell: the block's modules, None where a site does not exist."""
        sites = [None, None, None]
        for i, m in zip(self.kind.bn_sites, self._convs):
            sites[i] = m.bn
        return sites

    def _drop_scale(self, x):
        """Per-image drop-connect scale of the residual block in training (tools/utils.py:77-86), else None."""
        if not (self.training and self.has_residual and self.drop_connect_rate > 0.0):
            return None
        keep = 1.0 - self.drop_connect_rate
        u = getattr(self, 'drop_u', None)                   # (tests inject the uniform draws)
        u = torch.rand(x.size(0), dtype=x.dtype, device=x.device) if u is None else u.to(x.device)
        return torch.floor(keep + u) / keep

    def _affine_forward(self, x):
        """Derived-network block (layers.py:539-561 with affine BatchNorm; drop_connect of tools/utils.py:77-86 on the residual
        branch in training) -- tfnas_mbconv_fwd/bwd."""
        from .functions import MBConvAffineFn
        conv = self.hip_params()
        bnp = [t for m in self.bn_modules() for t in (m.weight, m.bias)]
        return MBConvAffineFn.apply(self._plan, x, self._drop_scale(x), self.bn_sites(), self.training, len(conv), *conv, *bnp)


class MBInvertedResBlock(_HipBlock):
    """MBConv block: 1x1 expand -> BN -> act -> depthwise kxk -> BN -> act -> [SE] -> 1x1 project -> BN [-> +x].

    ``forward`` runs the fused HIP path (sampled mode of ``tfnas_mixedop_fwd``; ``affine=True``: ``tfnas_mbconv_fwd``).  With
    ``mid_channels <= in_channels`` there is no expand convolution (``inverted_bottleneck is None``, mid normalised to in: the
    reference's layers.py:463-482): depthwise -> BN -> act -> [SE] -> project -> BN [+ x], the library's TFNAS_CELL_NOEXPAND cell
    with two BatchNorm sites.  (``Network._stem`` runs ``second_stem`` fused with ``first_stem`` instead.)

    ``dilation`` (1 | 2; 2 with kernel size 3 or 5 only): the spacing of the depthwise taps, padding ``dilation * (k // 2)`` so the
    output size does not depend on it -- TfnasGroup.dil under TFNAS_CELL_DILATION.  The weight stays [mc, 1, k, k]: no parameter,
    module or state_dict key depends on it.

    ``mix_kernels`` ((3, 5) | (3, 7) | (5, 7) | (3, 5, 7); not with dilation 2): a MixConv block -- ``depth_conv.conv`` is a
    MixDepthwiseConv2d whose channel segments have these kernel sizes (a packed TfnasGroup.k under TFNAS_CELL_MIXK);
    ``kernel_size`` is then the largest of them.  A block without it is what it always was, down to every state_dict key."""

    def __init__(self, in_channels, mid_channels, se_channels, out_channels, kernel_size=3, stride=1,
                 affine=False, act_func='relu', *, se_act=None, se_gate='sigmoid', dilation=1, mix_kernels=None):
        if mix_kernels is not None:
            mix_kernels = check_mix_kernels(mix_kernels)
            if dilation != 1:
                raise ValueError('tfnas_amd: a MixConv block (mix_kernels) has no dilation')
            kernel_size = max(mix_kernels)
        self.mix_kernels = mix_kernels
        if type(dilation) is not int or dilation not in (1, 2):
            raise ValueError('tfnas_amd: depthwise dilation is 1 or 2 (got %r)' % (dilation,))
        if dilation == 2 and kernel_size == 7:
            raise ValueError('tfnas_amd: dilation 2 goes with kernel size 3 or 5, not 7')
        self.dilation = dilation
        expand = mid_channels > in_channels
        if not expand:
            mid_channels = in_channels
            self.kind = NOEXPAND

        def depthwise(mc):
            if mix_kernels is not None:
                return MixDepthwiseConv2d(mc, mix_kernels, stride)
            return nn.Conv2d(mc, mc, kernel_size, stride, padding=dilation * get_same_padding(kernel_size), dilation=dilation,
                             groups=mc, bias=False)

        def lead(mc):       # (modules are made in the order of the fields: a seeded construction draws its weights in that order)
            return OrderedDict(
                inverted_bottleneck=_seq(conv=nn.Conv2d(in_channels, mc, 1, 1, 0, bias=False), **self.bn(mc)) if expand else None,
                depth_conv=_seq(conv=depthwise(mc), **self.bn(mc)))
        super().__init__(in_channels, mid_channels, se_channels, out_channels, kernel_size, stride, affine, act_func, lead,
                         se_act=se_act, se_gate=se_gate)

    @property
    def name(self):
        return 'MBInvertedResBlock'


class FusedMBConvBlock(_HipBlock):
    """Fused-MBConv block: dense 3x3 conv (stride, padding 1, no bias) -> BN -> act -> [SE] -> 1x1 project -> BN [-> +x].

    ``forward`` runs the HIP path as an MBInvertedResBlock does -- the library's TFNAS_CELL_FUSED cell (three implicit GEMMs of
    csrc/conv_kernels.hip where the depthwise passes stand), two BatchNorm sites; the search form through ``tfnas_mixedop_fwd``,
    ``affine=True`` (derived form, drop-connect on the residual branch in training) through ``tfnas_mbconv_fwd``.  Only as a
    block of its own: not a candidate of a multi-candidate MixedOP, kernel size 3 only, always with a project convolution."""

    kind = FUSED

    def __init__(self, in_channels, mid_channels, se_channels, out_channels, kernel_size=3, stride=1,
                 affine=False, act_func='relu', *, se_act=None, se_gate='sigmoid'):
        act_id(act_func)                                   # (first, as ever: ValueError for a name the library has no kernels for)
        if kernel_size != 3:
            raise NotImplementedError('tfnas_amd: FusedMBConvBlock has kernel size 3 only (got %r)' % (kernel_size,))
        if in_channels % 4 or mid_channels < 1:
            raise ValueError('tfnas_amd: FusedMBConvBlock wants in_channels a multiple of 4 and mid_channels >= 1')

        def lead(mc):
            return OrderedDict(fused_conv=_seq(conv=nn.Conv2d(in_channels, mc, 3, stride, 1, bias=False), **self.bn(mc)))
        super().__init__(in_channels, mid_channels, se_channels, out_channels, kernel_size, stride, affine, act_func, lead,
                         se_act=se_act, se_gate=se_gate)

    @property
    def name(self):
        return 'FusedMBConvBlock'
