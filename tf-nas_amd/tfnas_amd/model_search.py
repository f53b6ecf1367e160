"""Supernet for the TF-NAS search -- drop-in for the reference's ``models/model_search.py``.

Same classes, constructor signatures, ``forward(x, sampling, mode)`` signatures, parameter names/order and
helper methods as the reference (Network :213-365, MixedStage :125-210, MixedOP :32-122); the arithmetic of
every MixedOP cell, of the Gumbel-softmax over the arch parameters and of the sink-connecting stage mix runs
in hand-written HIP kernels (libtfnas_hip.so, C ABI in include/tfnas_hip.h).

Differences a caller can see (all optional):
  * ``forward`` accepts two extra keyword arguments, ``exp_noise`` (Exp(1) draws, [ncell, 8]) and ``rand_pos``
    (positions for mode 'random'), so tests / data-parallel ranks can inject identical noise.  When omitted,
    Exp(1) noise is drawn on the device with torch's generator and 'random' uses python's ``random`` exactly
    like the reference (models/model_search.py:79).
  * tensors must live on the GPU; there is no CPU path (the oracle in oracle/ is test infrastructure).
"""
import os
import weakref
import random

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .functions import ArchFn, CellPlan, HeadFn, MixedOpFn, SinkFn, StemFn, arch_sample
from .geometry import SKIP, kernel_tag
from .layers import ConvLayer, FusedMBConvBlock, IdentityLayer, LinearLayer, MBInvertedResBlock

PRIMITIVES = [
    'MBI_k3_e3', 'MBI_k3_e6', 'MBI_k5_e3', 'MBI_k5_e6',
    'MBI_k3_e3_se', 'MBI_k3_e6_se', 'MBI_k5_e3_se', 'MBI_k5_e6_se',
]

# (kernel, SE width as multiple of ic); the e3/e6 ratio only enters through mc_num_dict (model_search.py:19-29)
_OP_SPEC = {
    'MBI_k3_e3': (3, 0), 'MBI_k3_e6': (3, 0), 'MBI_k5_e3': (5, 0), 'MBI_k5_e6': (5, 0),
    'MBI_k3_e3_se': (3, 1), 'MBI_k3_e6_se': (3, 2), 'MBI_k5_e3_se': (5, 1), 'MBI_k5_e6_se': (5, 2),
}

OPS = {
    name: (lambda ic, mc, oc, s, aff, act, _k=k, _se=se:
           MBInvertedResBlock(ic, mc, ic * _se, oc, _k, s, affine=aff, act_func=act))
    for name, (k, se) in _OP_SPEC.items()
}

# Named primitives beside the eight defaults (PRIMITIVES itself stays the reference's): chosen per cell with ``primitives=``.
#   MBI_k7_*  the 7 x 7 twins of the defaults
#   FMB_k3_*  Fused-MBConv (dense 3 x 3 convolution), width from mc_num_dict[i] and SE = ic x {1, 2} like their MBI twins
#   DS_k*     expand-free (depthwise-separable) blocks: mid = ic whatever mc_num_dict[i] says, SE = ic
OPS.update({
    'MBI_k7_%s%s' % (e, '_se' if se else ''): (lambda ic, mc, oc, s, aff, act, _se=se:
                                               MBInvertedResBlock(ic, mc, ic * _se, oc, 7, s, affine=aff, act_func=act))
    for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))})
OPS.update({
    'FMB_k3_%s%s' % (e, '_se' if se else ''): (lambda ic, mc, oc, s, aff, act, _se=se:
                                               FusedMBConvBlock(ic, mc, ic * _se, oc, 3, s, affine=aff, act_func=act))
    for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))})
OPS.update({
    'DS_k%d%s' % (k, '_se' if se else ''): (lambda ic, mc, oc, s, aff, act, _k=k, _se=se:
                                            MBInvertedResBlock(ic, ic, ic * _se, oc, _k, s, affine=aff, act_func=act))
    for k in (3, 5) for se in (0, 1)})


# The dilated primitives, in a table of their own with the same signature (OPS keeps exactly the names it had): the taps of the
# depthwise convolution two pixels apart -- a 3 x 3 covers 5 x 5 with 9 taps, a 5 x 5 covers 9 x 9 with 25.
#   MBI_k3d2_* / MBI_k5d2_*  the dilated twins of the defaults (width from mc_num_dict[i], SE = ic x {1, 2})
#   DS_k3d2* / DS_k5d2*      expand-free: the dil_conv_3x3 / dil_conv_5x5 of the DARTS-family spaces
DILATED_OPS = {
    'MBI_k%dd2_%s%s' % (k, e, '_se' if se else ''): (lambda ic, mc, oc, s, aff, act, _k=k, _se=se:
                                                     MBInvertedResBlock(ic, mc, ic * _se, oc, _k, s, affine=aff, act_func=act,
                                                                        dilation=2))
    for k in (3, 5) for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))}
DILATED_OPS.update({
    'DS_k%dd2%s' % (k, '_se' if se else ''): (lambda ic, mc, oc, s, aff, act, _k=k, _se=se:
                                              MBInvertedResBlock(ic, ic, ic * _se, oc, _k, s, affine=aff, act_func=act, dilation=2))
    for k in (3, 5) for se in (0, 1)})


# The MixConv primitives (Tan & Le, the MixNet family), in a table of their own with the same signature: ONE depthwise whose channel
# segments are 3 x 3 | 5 x 5 (k35) or 3 x 3 | 5 x 5 | 7 x 7 (k357) -- the 5 x 5 / 7 x 7 receptive field on a part of the channels at
# 17 / 27.7 taps per channel on average instead of 25 / 49.
#   MBI_k35_* / MBI_k357_*   width from mc_num_dict[i], SE = ic x {1, 2}
#   DS_k35* / DS_k357*       expand-free
MIX_OPS = {
    'MBI_k%s_%s%s' % (tag, e, '_se' if se else ''): (lambda ic, mc, oc, s, aff, act, _ks=ks, _se=se:
                                                     MBInvertedResBlock(ic, mc, ic * _se, oc, max(_ks), s, affine=aff, act_func=act,
                                                                        mix_kernels=_ks))
    for tag, ks in (('35', (3, 5)), ('357', (3, 5, 7))) for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))}
MIX_OPS.update({
    'DS_k%s%s' % (tag, '_se' if se else ''): (lambda ic, mc, oc, s, aff, act, _ks=ks, _se=se:
                                              MBInvertedResBlock(ic, ic, ic * _se, oc, max(_ks), s, affine=aff, act_func=act,
                                                                 mix_kernels=_ks))
    for tag, ks in (('35', (3, 5)), ('357', (3, 5, 7))) for se in (0, 1)})


def primitive_factory(name):
    """The factory (ic, mc, oc, stride, affine, act) -> block of a registered primitive, from any of the three tables."""
    return OPS[name] if name in OPS else DILATED_OPS[name] if name in DILATED_OPS else MIX_OPS[name]


def check_primitives(primitives):
    """The candidate names of one MixedOP: None -> the defaults; else a list of exactly len(PRIMITIVES) registered names
    (the architecture kernels and noise tensors are 8 wide).  ValueError names the legal ones."""
    if primitives is None:
        return list(PRIMITIVES)
    names = list(primitives)
    if len(names) != len(PRIMITIVES):
        raise ValueError('tfnas_amd: a MixedOP takes exactly %d primitives, got %d' % (len(PRIMITIVES), len(names)))
    for n in names:
        if n not in OPS and n not in DILATED_OPS and n not in MIX_OPS and n != SKIP:
            raise ValueError('tfnas_amd: unknown primitive %r (one of %s, or %r in a residual cell)'
                             % (n, ', '.join(sorted(list(OPS) + list(DILATED_OPS) + list(MIX_OPS))), SKIP))
    return names


def _check_skips(names, in_channels, out_channels, stride):
    """What a cell asks of its 'skip' candidates (the library's rules for TFNAS_GROUP_SKIP groups); ValueError names the reason."""
    if SKIP not in names:
        return
    if stride != 1 or in_channels != out_channels:
        raise ValueError('tfnas_amd: a %r candidate needs a residual cell (stride 1, in_channels == out_channels); this one has '
                         'stride %d, %d -> %d channels' % (SKIP, stride, in_channels, out_channels))
    if all(n == SKIP for n in names):
        raise ValueError('tfnas_amd: a cell needs at least one candidate that is not %r' % SKIP)
    first = names.index(SKIP)
    if any(n != SKIP for n in names[first:]):
        raise ValueError('tfnas_amd: %r candidates stand after every other candidate of a cell (got %s)' % (SKIP, ', '.join(names)))


def _cell_primitives(primitives, stage, block):
    """``primitives`` of a MixedStage / Network for one cell ('stage3', 'block2'): one list for every cell, or a
    {stage: {block: list}} mapping whose missing entries mean the defaults (a MixedStage built on its own, without a stage
    name, takes its {block: list} part)."""
    if not isinstance(primitives, dict):
        return primitives
    per_stage = primitives if stage is None else (primitives.get(stage) or {})
    return per_stage.get(block)


def _cell_se_style(se_style, name):
    """``se_style`` of a MixedStage / Network for one of its parts: one (se_act, se_gate) pair (or None) for every part, or a
    {name: pair} mapping -- {block: pair} for a MixedStage, {stage: pair} (or {stage: {block: pair}}) for a Network -- whose
    missing entries mean the default."""
    return se_style.get(name) if isinstance(se_style, dict) else se_style


_SAMPLE_MODES = {'gumbel': 0, 'gumbel_2': 0, 'min_alphas': 1, 'max_alphas': 2}


class MixedOP(nn.Module):
    def __init__(self, in_channels, out_channels, stride, affine, act_func, num_ops, mc_num_dict, lat_lookup, primitives=None,
                 se_style=None):
        super().__init__()
        self.primitives = check_primitives(primitives)
        # squeeze-excite style of the cell, one for all its candidates: None (the reference's: hidden activation = act_func,
        # logistic gate) or a (se_act, se_gate) pair, e.g. MobileNetV3's ('relu', 'h-sigmoid') -- layers._HipBlock.  The latency
        # tables know no style: a styled candidate is looked up under the key of its logistic twin (nobody has measured the
        # hard-sigmoid forward beside the logistic one on this chip).
        self.se_style = _lib.se_style_pair(se_style)
        self.num_ops = num_ops
        self.lat_lookup = lat_lookup
        self.mc_num_dict = mc_num_dict
        self.in_channels, self.out_channels, self.stride, self.act_func = in_channels, out_channels, stride, act_func
        _check_skips(self.primitives[:num_ops], in_channels, out_channels, stride)
        self.m_ops = nn.ModuleList()
        for i in range(num_ops):
            if self.primitives[i] == SKIP:                 # (no width: mc_num_dict[i] is ignored)
                self.m_ops.append(IdentityLayer(in_channels, out_channels))
                continue
            self.m_ops.append(primitive_factory(self.primitives[i])(in_channels, self.mc_num_dict[i], out_channels, stride,
                                                                    affine, act_func))
            self.m_ops[-1].set_se_style(self.se_style)     # (the registry's factories keep their signature: applied here,
                                                           #  before any plan of the cell exists)
        self._initialize_log_alphas()
        self.reset_switches()
        self.T = 1.0
        self._plans = {}
        self._lat_cache = {}
        self._pre = None           # (w_row, cell_lat) or sampled position handed down by Network.forward

    # ---- reference helpers -------------------------------------------------------------------------
    def fink_ori_idx(self, idx):
        count = 0
        for ori_idx in range(len(self.switches)):
            if self.switches[ori_idx]:
                count += 1
                if count == (idx + 1):
                    break
        return ori_idx

    def get_lookup_latency(self, size):
        lats = []
        for op in self.m_ops:
            if op.name == 'IdentityLayer':                 # (models/model_search.py:96-97: the skip costs nothing)
                lats.append(0)
                continue
            key = '{}_{}_{}_{}_{}_{}_s{}_{}'.format(op.name, size, op.in_channels, op.se_channels, op.out_channels,
                                                    kernel_tag(op.kernel_size, getattr(op, 'dilation', 1), getattr(op, 'mix_kernels', None)),
                                                    op.stride, op.act_func)
            lats.append(self.lat_lookup[key][op.mid_channels])
        return lats

    def _initialize_log_alphas(self):
        self.register_parameter('log_alphas', nn.Parameter(F.log_softmax(torch.zeros((self.num_ops,)), dim=-1)))

    def reset_switches(self):
        self.switches = [True] * self.num_ops

    def set_temperature(self, T):
        self.T = T

    # ---- HIP plumbing --------------------------------------------------------------------------------
    def _plan(self, idxs):
        key = tuple(idxs)
        p = self._plans.get(key)
        if p is not None and p.blocks[0] is not self.m_ops[key[0]]:
            # this module is a shallow copy (nn.DataParallel.replicate shares plain attributes between replicas): the
            # cached plans hold the ORIGINAL module's blocks, i.e. another device's weights -- start a private cache
            self._plans, p = {}, None
        if p is None:
            p = CellPlan(self.in_channels, self.out_channels, self.stride, self.act_func,
                         [self.m_ops[i] for i in idxs], mixed_kinds=True)
            self._plans[key] = p
        return p

    def lat_tensor(self, size, device):
        """Looked-up latencies of the 8 candidates as a device tensor (cached per input size / widths)."""
        key = (size, str(device), tuple(getattr(op, 'mid_channels', 0) for op in self.m_ops))
        t = self._lat_cache.get(key)
        if t is None:
            t = torch.tensor(self.get_lookup_latency(size), dtype=torch.float32, device=device)
            self._lat_cache = {key: t}
        return t

    def sample_index(self, mode, exp_noise=None, rand_pos=None, pos=None):
        """Bi-sampling bookkeeping of models/model_search.py:59-81; returns the chosen original op index.
        ``pos`` is the device-computed position for the gumbel / min / max modes."""
        nactive = sum(self.switches)
        if mode in _SAMPLE_MODES:
            if pos is None:
                if mode.startswith('gumbel') and exp_noise is None:
                    exp_noise = torch.empty(8, device=self.log_alphas.device).exponential_()
                pos = arch_sample([self.log_alphas], [[int(s) for s in self.switches]],
                                  None if exp_noise is None else exp_noise.reshape(1, -1)[:, :8], self.T,
                                  _SAMPLE_MODES[mode])[0]
            if not 0 <= pos < nactive:
                raise ValueError('sampled position %d outside the %d switched-on candidates' % (pos, nactive))
            if mode == 'gumbel':
                idx = pos                      # raw position, exactly as the reference (model_search.py:63-64)
                self.switches[idx] = False
            else:
                idx = self.fink_ori_idx(pos)
                self.reset_switches()
        elif mode == 'random':
            p = random.choice(range(nactive)) if rand_pos is None else int(rand_pos)
            if not 0 <= p < nactive:
                raise ValueError('random position %d outside the %d switched-on candidates' % (p, nactive))
            idx = self.fink_ori_idx(p)
            self.reset_switches()
        else:
            raise ValueError('invalid sampling mode...')
        return idx

    def forward(self, x, sampling, mode, exp_noise=None, rand_pos=None):
        pre, self._pre = self._pre, None            # (consumed exactly once; Network.forward clears leftovers on error)
        if sampling:
            idx = pre if pre is not None else self.sample_index(mode, exp_noise, rand_pos)
            self.last_idx = idx
            op = self.m_ops[idx]
            if op.kind is None:                            # a sampled skip: the input itself, no launch (as the reference)
                return x, 0
            return MixedOpFn.apply(self._plan((idx,)), x, None, *op.hip_params()), 0
        if pre is not None:
            w, out_lat = pre
        else:
            if exp_noise is None:
                exp_noise = torch.empty(8, device=x.device).exponential_()
            lat = self.lat_tensor(x.size(-1), x.device)
            W, CL = ArchFn.apply(exp_noise.reshape(1, 8).to(x.device), lat.reshape(1, 8), self.T, self.log_alphas)
            w, out_lat = W[0], CL[0]
        plan = self._plan(tuple(range(self.num_ops)))
        out = MixedOpFn.apply(plan, x, w, *plan.params())
        self.last_w = w
        return out, out_lat


class MixedStage(nn.Module):
    def __init__(self, ics, ocs, ss, affs, acts, mc_num_ddict, lat_lookup, stage_type, primitives=None, stage_name=None,
                 se_style=None):
        super().__init__()
        self.lat_lookup = lat_lookup
        self.mc_num_ddict = mc_num_ddict
        self.stage_type = stage_type   # 0 for stage6 || 1 for stage1 || 2 for stage2 || 3 for stage3/4/5
        self.start_res = 0 if ((ics[0] == ocs[0]) and (ss[0] == 1)) else 1
        self.num_res = len(ics) - self.start_res + 1
        nblocks = {0: 1, 1: 2, 2: 3, 3: 4}.get(stage_type)
        if nblocks is None:
            raise ValueError('invalid stage_type...')
        self.nblocks = nblocks
        for b in range(nblocks):
            names = _cell_primitives(primitives, stage_name, 'block%d' % (b + 1))
            try:
                _check_skips(check_primitives(names), ics[b], ocs[b], ss[b])
            except ValueError as e:
                if names is None or SKIP not in list(names):
                    raise
                # (the first block of a stage that changes width or stride cannot hold a skip: one list for every cell cannot work)
                raise ValueError('%s -- %s block%d; give the skip to the residual cells only: primitives={stage: {block: list}}, '
                                 'e.g. from geometry.residual_cells()' % (e, stage_name or 'stage', b + 1)) from None
            setattr(self, 'block%d' % (b + 1),
                    MixedOP(ics[b], ocs[b], ss[b], affs[b], acts[b], len(PRIMITIVES), mc_num_ddict['block%d' % (b + 1)],
                            lat_lookup, primitives=names,
                            se_style=_cell_se_style(se_style, 'block%d' % (b + 1))))
        self._initialize_betas()

    def blocks(self):
        return [getattr(self, 'block%d' % (b + 1)) for b in range(self.nblocks)]

    def forward(self, x, sampling, mode, exp_noise=None, rand_pos=None):
        res_list, lat_list = [x], []
        for b, blk in enumerate(self.blocks()):
            out, lat = blk(res_list[-1], sampling, mode,
                           None if exp_noise is None else exp_noise[b],
                           None if rand_pos is None else rand_pos[b])
            res_list.append(out)
            lat_list.append(lat)
        res = res_list[self.start_res:]
        if sampling:
            cell_lat = None
        else:
            cell_lat = torch.stack(lat_list)
            if self.start_res == 0:            # the stage input is a depth choice of latency 0
                cell_lat = torch.cat([cell_lat.new_zeros(1), cell_lat])
        out, out_lat = SinkFn.apply(self.betas, cell_lat, *res)
        return out, out_lat

    def _initialize_betas(self):
        self.register_parameter('betas', nn.Parameter(torch.zeros((self.num_res))))


# Network.forward on the path level when it can (GPU model, tfnas_amd.search.USE_PATHS): TFNAS_MODULE_PATHS=0
# keeps the per-cell route (one autograd node per MixedOP: what the stage-by-stage tests hook into)
MODULE_PATHS = os.environ.get('TFNAS_MODULE_PATHS', '1') != '0'
SECOND_PATH_ON_SIDE_STREAM = True       # the 'random' forward of a bi-sampling pair on a second HIP stream (tests flip it)




class Network(nn.Module):
    def __init__(self, num_classes, mc_num_dddict, lat_lookup, primitives=None, se_style=None, extended_paths=False):
        super().__init__()
        self.se_style = se_style               # (of the MixedOP cells; the stems keep the reference's squeeze-excite)
        # extended_paths=True: a network with candidates beside the plain MBConv ones (other kinds, MixConv, dilated, skip) runs on
        # the path level and the weight arena too (path_capable).  Off by default: such a network then takes the per-cell route in
        # every step, as it always did.  A routing switch of this object alone: not handed to the stages, not in state_dict.
        self.extended_paths = bool(extended_paths)
        self.lat_lookup = lat_lookup
        self.mc_num_dddict = mc_num_dddict

        self.first_stem = ConvLayer(3, 32, kernel_size=3, stride=2, affine=False, act_func='relu')
        self.second_stem = MBInvertedResBlock(32, 32, 8, 16, kernel_size=3, stride=1, affine=False, act_func='relu')
        cfg = [
            ('stage1', [16, 24], [24, 24], [2, 1], 'relu', 1),
            ('stage2', [24, 40, 40], [40, 40, 40], [2, 1, 1], 'swish', 2),
            ('stage3', [40, 80, 80, 80], [80, 80, 80, 80], [2, 1, 1, 1], 'swish', 3),
            ('stage4', [80, 112, 112, 112], [112, 112, 112, 112], [1, 1, 1, 1], 'swish', 3),
            ('stage5', [112, 192, 192, 192], [192, 192, 192, 192], [2, 1, 1, 1], 'swish', 3),
            ('stage6', [192], [320], [1], 'swish', 0),
        ]
        self._stage_names = [c[0] for c in cfg]
        for name, ics, ocs, ss, act, st in cfg:
            setattr(self, name, MixedStage(ics=ics, ocs=ocs, ss=ss, affs=[False] * len(ics), acts=[act] * len(ics),
                                           mc_num_ddict=mc_num_dddict[name], lat_lookup=lat_lookup, stage_type=st,
                                           primitives=primitives, stage_name=name, se_style=_cell_se_style(se_style, name)))
        self.feature_mix_layer = ConvLayer(320, 1280, kernel_size=1, stride=1, affine=False, act_func='swish')
        self.global_avg_pooling = nn.AdaptiveAvgPool2d(1)
        self.classifier = LinearLayer(1280, num_classes)
        self._initialization()
        self._cells = None
        self._lat_stack = None
        self._stem_plan = None
        self._head_plan = None
        from .functions import adopt_modes
        adopt_modes(self)                      # self.hip_modes (functions.HipModes), shared by every sub-module's plans

    def set_hip_modes(self, **kw):
        """e.g. set_hip_modes(gemm='f32'): this model's launches only (TfnasCellDesc.gemm_mode; functions.HipModes)."""
        for k, v in kw.items():
            if not hasattr(self.hip_modes, k):
                raise AttributeError(k)
            setattr(self.hip_modes, k, v)

    # ---- stems / head on the HIP path -------------------------------------------------------------------
    class _StemBlock:
        """Adapter presenting first_stem.conv + second_stem as one candidate block of a TFNAS_MODE_STEM cell."""

        def __init__(self, first, second):
            self.first, self.second = first, second
            self.mid_channels, self.kernel_size, self.se_channels = second.mid_channels, second.kernel_size, second.se_channels

        def hip_params(self):
            se = self.second.squeeze_excite
            return [self.first.conv.weight, self.second.depth_conv.conv.weight, self.second.point_linear.conv.weight,
                    se.conv_reduce.weight, se.conv_reduce.bias, se.conv_expand.weight, se.conv_expand.bias]

    class _HeadBlock:
        def __init__(self, conv_layer):
            self.layer = conv_layer
            self.mid_channels, self.kernel_size, self.se_channels = conv_layer.out_channels, 3, 0

        def hip_params(self):
            return [self.layer.conv.weight]

    def stem_plan(self):
        fs, ss = self.first_stem, self.second_stem
        if (fs.kernel_size, fs.stride, fs.in_channels, fs.act_func, ss.act_func, ss.stride) != (3, 2, 3, 'relu', 'relu', 1) \
                or ss.inverted_bottleneck is not None or ss.squeeze_excite is None:
            raise NotImplementedError('stem geometry differs from models/model_search.py:219-220')
        if self._stem_plan is None:
            self._stem_plan = CellPlan(27, ss.out_channels, 1, 'relu', [Network._StemBlock(fs, ss)], mode=_lib.MODE_STEM, modes=self.hip_modes)
        return self._stem_plan

    def _stem(self, x):
        plan = self.stem_plan()
        return StemFn.apply(plan, x, None, *plan.params())

    def head_plan(self):
        fm = self.feature_mix_layer
        if self._head_plan is None:
            self._head_plan = CellPlan(fm.in_channels, 4, 1, fm.act_func, [Network._HeadBlock(fm)], mode=_lib.MODE_HEAD, modes=self.hip_modes)
        return self._head_plan

    def _head(self, x):
        return HeadFn.apply(self.head_plan(), x, self.feature_mix_layer.conv.weight)

    def stages(self):
        return [getattr(self, n) for n in self._stage_names]

    def cells(self):
        if self._cells is None:
            self._cells = [blk for st in self.stages() for blk in st.blocks()]
        return self._cells

    def arch_weights(self, size, dev, exp_noise=None):
        """(W [ncell, 8], CL [ncell]): gumbel-softmax weights of every cell and their expected latencies for a stem output
        of spatial ``size`` -- F.gumbel_softmax + get_lookup_latency + sum(w*lat) of MixedOP.forward (model_search.py:87-90)
        for the whole network in one launch."""
        cells = self.cells()
        if exp_noise is None:
            exp_noise = torch.empty(len(cells), 8, device=dev).exponential_()
        key = (size, str(dev), tuple(getattr(op, 'mid_channels', 0) for c in cells for op in c.m_ops))
        if self._lat_stack is None or self._lat_stack[0] != key:
            lats = []
            for st in self.stages():
                for blk in st.blocks():
                    lats.append(blk.lat_tensor(size, dev))
                    size = (size - 1) // blk.stride + 1
            self._lat_stack = (key, torch.stack(lats))
        T = cells[0].T
        if any(c.T != T for c in cells):
            raise ValueError('all MixedOPs must share one temperature (Network.set_temperature)')
        return ArchFn.apply(exp_noise.to(dev), self._lat_stack[1], T, *[c.log_alphas for c in cells])

    def _prepare(self, x, sampling, mode, exp_noise, rand_pos, pos=None):
        """All arch-parameter work of one forward in ONE launch (and at most one device->host copy)."""
        cells = self.cells()
        n = len(cells)
        dev = x.device
        if not sampling:
            W, CL = self.arch_weights(x.size(-1), dev, exp_noise)
            # unbind, not W[i]: 18 selects cost 18 zero-filled [18, 8] buffers + 18 slice copies + 17 adds in backward
            # (on the alpha-step's single dependency chain); unbind's backward is one stack
            for c, w_c, cl_c in zip(cells, W.unbind(0), CL.unbind(0)):
                c._pre = (w_c, cl_c)
            return
        if mode in _SAMPLE_MODES:
            if pos is not None:                       # positions already chosen (host-side sampling of search.w_step)
                if len(pos) != n:
                    raise ValueError('pos must hold one position per MixedOP')
                self._require_all_switches_on()
                for i, c in enumerate(cells):
                    c._pre = c.sample_index(mode, pos=int(pos[i]))
                return
            if mode.startswith('gumbel') and exp_noise is None:
                exp_noise = torch.empty(n, 8, device=dev).exponential_()
            pos = arch_sample([c.log_alphas for c in cells], [[int(s) for s in c.switches] for c in cells],
                              None if exp_noise is None else exp_noise.to(dev), cells[0].T, _SAMPLE_MODES[mode])
            for i, c in enumerate(cells):
                c._pre = c.sample_index(mode, pos=pos[i])
        elif mode == 'random':
            for i, c in enumerate(cells):
                c._pre = c.sample_index(mode, rand_pos=None if rand_pos is None else rand_pos[i])
        else:
            raise ValueError('invalid sampling mode...')

    def _require_all_switches_on(self):
        """Host-sampled gumbel positions are computed over all 8 candidates; a caller that skipped reset_switches()
        (e.g. after an exception mid-step) would otherwise switch off the wrong op silently."""
        if not all(all(c.switches) for c in self.cells()):
            raise RuntimeError('host-sampled positions need every switch on: call reset_switches() first')

    def stem_features(self, x):
        """first_stem + second_stem output; may be passed back as ``forward(..., stem_out=)`` so that several forwards
        of the same batch (the two sampled paths of a w-step) share one evaluation of the candidate-free stems."""
        return self._stem(x)

    def forward_bisample(self, x, pos_g, rand_pos, side_stream):
        """Both sampled paths of a bi-sampling w-step in ONE sweep over the cells: the 'gumbel' candidate of a cell runs on
        the current stream, its 'random' candidate on ``side_stream``, cell by cell.  Same kernels, same inputs and the
        same per-cell switch bookkeeping as forward(x, True, 'gumbel', pos=pos_g) followed by
        forward(x, True, 'random', rand_pos=rand_pos) -- but the host enqueues the two paths interleaved, so both streams
        have work from the first cell on, and because autograd replays nodes newest-first the two paths' backward
        passes are interleaved too (after the sequential forwards the whole backward of the second path is enqueued
        before the first kernel of the first path's).  The stems are evaluated once.
        Returns (logits_gumbel, logits_random); the second lives on ``side_stream``."""
        cells = self.cells()
        if len(pos_g) != len(cells) or len(rand_pos) != len(cells):
            raise ValueError('pos_g / rand_pos must hold one entry per MixedOP')
        self._require_all_switches_on()
        cur = torch.cuda.current_stream(x.device)
        feat = self._stem(x)
        side_stream.wait_stream(cur)
        feat.record_stream(side_stream)
        xa = xb = feat
        ci = 0
        for st in self.stages():
            ra, rb = [xa], [xb]
            for blk in st.blocks():
                ia = blk.sample_index('gumbel', pos=int(pos_g[ci]))
                ib = blk.sample_index('random', rand_pos=rand_pos[ci])
                blk.last_idx = ib                          # (what two sequential forwards leave behind)
                # (a sampled skip is the path's input itself: no launch)
                ra.append(ra[-1] if blk.m_ops[ia].kind is None else
                          MixedOpFn.apply(blk._plan((ia,)), ra[-1], None, *blk.m_ops[ia].hip_params()))
                with torch.cuda.stream(side_stream):
                    rb.append(rb[-1] if blk.m_ops[ib].kind is None else
                              MixedOpFn.apply(blk._plan((ib,)), rb[-1], None, *blk.m_ops[ib].hip_params()))
                ci += 1
            xa, _ = SinkFn.apply(st.betas, None, *ra[st.start_res:])
            with torch.cuda.stream(side_stream):
                xb, _ = SinkFn.apply(st.betas, None, *rb[st.start_res:])
        la = self.classifier(self._head(xa))
        with torch.cuda.stream(side_stream):
            lb = self.classifier(self._head(xb))
        return la, lb

    # ---- path level behind the module API ----------------------------------------------------------------------------
    def _path_state(self):
        """The SearchState (weight arena + path runner, search.py / path.py) the drop-in ``forward`` runs on: the one a caller
        built with ``search.SearchState(model)`` if there is one (it registers itself), else a private one."""
        from . import search
        st = self.__dict__.get('_pstate')
        if st is None or st.runner is None or st.model is not self:
            # a private state per model, owned by the model: it holds the model weakly, so it is freed (path contexts, arenas,
            # weight arena -- GBs at B = 128) with the model, by reference counting, and never while another model that is still in
            # use would need it (a teacher and a student, an EMA copy evaluated between forward and backward, ...)
            st = search.SearchState(self, weak_model=True)
            if st.runner is None:
                return None
        if not st.arena.intact():                       # (p.data = ... of a different tensor: the epoch boundary)
            st.build_paths()
        return st

    def close(self):
        """Release the path-level state of the drop-in forward (weight arena views stay valid: the parameters keep their
        storages; the next forward rebuilds what it needs)."""
        st = self.__dict__.pop('_pstate', None)
        if st is not None:
            st.release()

    def __getstate__(self):
        # ctypes contexts, HIP streams and events of the path-level state are process-local: copy.deepcopy(model) /
        # torch.save(model) carry the module only
        state = self.__dict__.copy()
        state.pop('_pstate', None)
        return state

    def _use_paths(self, x):
        from . import search
        if not (MODULE_PATHS and search.USE_PATHS and x.is_cuda):
            return False
        if not self.path_capable():                   # (plain candidates; every candidate with extended_paths)
            return False
        p = self.first_stem.conv.weight
        return p.is_cuda and p.is_leaf and p.device == x.device

    def _forward_paths(self, x, sampling, mode, exp_noise, rand_pos, stem_out, pos):
        """``forward`` on the path level (tfnas_paths_fwd / _bwd: ONE C call per direction for the 18 cells + 6 sinks instead
        of one autograd node per cell) -- what closes the gap between the two-line import swap and tfnas_amd.search's own
        steps.  Same kernels, bit-identical results.  Sampled mode: the cells' weight gradients are stored by the backward
        straight into the weight arena and exposed as ``.grad`` views, with autograd's semantics: written where ``.grad`` is
        None, added to it otherwise (several backward passes or micro-batches without a zero_grad in between are summed)."""
        st = self._path_state()
        if st is None:
            return None
        runner = st.runner
        cells = self.cells()
        if not sampling and any(p.requires_grad for p in cells[0].m_ops[0].parameters()):
            return None                                       # soft-mode weight gradients: per-cell route
        if sampling and torch.is_grad_enabled() and any(stg.betas.requires_grad for stg in self.stages()):
            return None                                       # d betas of a sampled forward: per-cell route (SinkFn)
        if sampling:
            return self._sampled_on_paths(st, x, stem_out, mode, exp_noise, rand_pos, pos)
        feat = self._stem(x) if stem_out is None else stem_out
        W, CL = self.arch_weights(feat.size(-1), x.device, exp_noise)
        out, stage_lat = runner.soft(feat, W, CL)
        lat = stage_lat.sum() + self.lat_lookup['base']
        return self.classifier(self._head(out)), lat

    def _host_positions(self, st, mode, exp_noise, pos):
        """'gumbel' positions of all cells from the host mirror of the log_alphas (search.SearchState.alpha_host: an asynchronous
        pinned copy, re-staged only when a log_alphas tensor was replaced or modified) -- no blocking device->host copy inside a
        weight step whose architecture parameters did not change since the last one, so the host can run ahead of the GPU.  Only
        when the caller passes no noise of its own (the noise is then drawn on the host, seeded from torch.initial_seed()) and
        every switch is on; otherwise the device-side sampler of ``_prepare``."""
        from . import search
        if mode != 'gumbel' or exp_noise is not None or pos is not None or not search.HOST_SAMPLING:
            return pos
        cells = self.cells()
        if not all(all(c.switches) for c in cells):
            return pos
        rng = st.__dict__.get('_host_rng')
        if rng is None:
            import numpy as np
            rng = st._host_rng = np.random.default_rng(torch.initial_seed() & 0xffffffff)
        e = rng.standard_exponential((len(cells), 8), dtype='float32')
        return search.host_gumbel_positions(st.alpha_host().numpy(), e, cells[0].T)

    def _sampled_on_paths(self, st, x, feat, mode, exp_noise, rand_pos, pos):
        runner = st.runner
        cells = self.cells()
        dev = x.device
        cur = torch.cuda.current_stream(dev)
        # second forward of a bi-sampling pair (train_search.py:375-379: model(x, True, 'gumbel') then model(x, True, 'random') on
        # the SAME batch, one backward of the summed loss): enqueue it on a second HIP stream so that its kernels -- and, autograd
        # replaying every node on its forward stream, its backward -- run beside the first path's (a sampled
        # path's launches fill a fraction of the chip).  It may start as soon as what the FIRST forward could start on is ready
        # (the event recorded when that forward was entered), provided x and the weights are what they were then.
        key = (x.data_ptr(), x._version, tuple(x.shape), st.weights_epoch, self.first_stem.conv.weight._version)
        first = st.__dict__.get('_fwd_first')
        side = None
        if (SECOND_PATH_ON_SIDE_STREAM and mode == 'random' and torch.is_grad_enabled() and first is not None and first[0] == key and first[2] == cur
                and feat is None):
            side = st.side_stream(dev)
        if mode == 'gumbel':
            st.throttle(dev)                    # (nothing in a host-sampled step blocks the host: keep it <= 1 step ahead)
            st.mark_step(dev)
            ev = torch.cuda.Event()
            ev.record(cur)
            st._fwd_first = (key, ev, cur)
        else:
            st._fwd_first = None
        if side is None:
            feat = self._stem(x) if feat is None else feat
            self._prepare(feat, True, mode, exp_noise, rand_pos, self._host_positions(st, mode, exp_noise, pos))
            idxs = []
            for c in cells:
                idxs.append(int(c._pre))
                c.last_idx, c._pre = int(c._pre), None
            # two sampled forwards may be alive at once (the bi-sampling pair runs gumbel, random, then ONE backward)
            out = runner.sampled(feat, idxs, name='A' if mode == 'gumbel' else 'B', expose=st)
            return self.classifier(self._head(out)), 0.0
        side.wait_event(first[1])
        # device tensors the caller made AFTER the first forward was entered (rand_pos / exp_noise of this call) are produced on
        # the caller's stream: the side stream must see them finished -- one more event, recorded now
        late = [t for t in (exp_noise, rand_pos) if torch.is_tensor(t) and t.is_cuda]
        if late:
            ev2 = torch.cuda.Event()
            ev2.record(cur)
            side.wait_event(ev2)
            for t in late:
                t.record_stream(side)
        x.record_stream(side)
        if not st.__dict__.get('_warned_off'):
            # the stems' AccumulateGrad nodes now receive one of their two gradients from the side stream -- intended (the engine
            # synchronises them); torch >= 2.9 warns about exactly this on every backward.  NB the switch is process-wide: it
            # also silences the diagnostic for other models in the process (set SECOND_PATH_ON_SIDE_STREAM = False to keep it)
            off = getattr(torch.autograd.graph, 'set_warn_on_accumulate_grad_stream_mismatch', None)
            if off is not None:
                off(False)
            st._warned_off = True
        with torch.cuda.stream(side):
            feat = self._stem(x)
            self._prepare(feat, True, mode, exp_noise, rand_pos, pos)
            idxs = []
            for c in cells:
                idxs.append(int(c._pre))
                c.last_idx, c._pre = int(c._pre), None
            out = runner.sampled(feat, idxs, name='B', expose=st, main_stream=cur)
        cur.wait_stream(side)
        out.record_stream(cur)
        # (both heads on the caller's stream: the shared head / classifier parameters accumulate their two gradients there)
        return self.classifier(self._head(out)), 0.0

    def forward(self, x, sampling, mode='max', exp_noise=None, rand_pos=None, stem_out=None, pos=None):
        if self._use_paths(x):
            try:
                res = self._forward_paths(x, sampling, mode, exp_noise, rand_pos, stem_out, pos)
            except BaseException:
                for c in self.cells():
                    c._pre = None
                raise
            if res is not None:
                return res
        out_lat = self.lat_lookup['base'] if not sampling else 0.0
        # first_stem + second_stem run as one "stem cell" of the HIP library (stock PyTorch-ROCm ops cost 70 ms per
        # iteration pair here: MIOpen's fp32 NHWC path falls back to naive_conv_*, torch's BN backward is slow)
        x = self._stem(x) if stem_out is None else stem_out
        try:
            self._prepare(x, sampling, mode, exp_noise, rand_pos, pos)
            for st in self.stages():
                x, lat = st(x, sampling, mode)
                out_lat += lat
        except BaseException:
            for c in self.cells():           # a forward that aborts must not leave hand-down state for the next one
                c._pre = None
            raise
        x = self._head(x)                      # feature_mix_layer + global_avg_pooling (HIP), [N, 1280]
        x = self.classifier(x)
        return x, out_lat

    def plain_candidates(self):
        """Every candidate of every cell is a plain MBConv block (what the path level and the epoch boundary are built for)."""
        hit = self.__dict__.get('_plain')
        if hit is None:
            hit = self.__dict__['_plain'] = all(op.kind is _lib.MBCONV and getattr(op, 'mix_kernels', None) is None
                                                for c in self.cells() for op in c.m_ops)      # (a MixConv block: per-cell route)
        return hit

    def path_capable(self):
        """The path level (tfnas_path_plan) takes this network: every candidate plain -- or, with ``extended_paths``, every cell one
        the library's path plan accepts: candidates of the three block kinds (MixConv and dilated ones included) and skips."""
        if self.plain_candidates():
            return True
        if not self.extended_paths:
            return False
        hit = self.__dict__.get('_path_ok')
        if hit is None:
            hit = self.__dict__['_path_ok'] = all(op.kind is None or op.kind in _lib.KINDS for c in self.cells() for op in c.m_ops)
        return hit

    def set_temperature(self, T):
        for m in self.modules():
            if isinstance(m, MixedOP):
                m.set_temperature(T)

    def weight_parameters(self):
        return [v for k, v in self.named_parameters() if not (k.endswith('log_alphas') or k.endswith('betas'))]

    def arch_parameters(self):
        return [v for k, v in self.named_parameters() if k.endswith('log_alphas') or k.endswith('betas')]

    def log_alphas_parameters(self):
        return [v for k, v in self.named_parameters() if k.endswith('log_alphas')]

    def betas_parameters(self):
        return [v for k, v in self.named_parameters() if k.endswith('betas')]

    def reset_switches(self):
        for m in self.modules():
            if isinstance(m, MixedOP):
                m.reset_switches()

    def _initialization(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)) and m.bias is not None:
                nn.init.constant_(m.bias, 0)
