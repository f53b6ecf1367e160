"""ctypes binding of libtfnas_hip.so (C ABI: include/tfnas_hip.h).

The shared library is built in-tree by ``tf-nas_amd/csrc/Makefile`` (``__graft_entry__.build()``).  There is
NO fallback: if the library is missing or an entry point returns non-zero, a RuntimeError is raised.
"""
import collections
import ctypes as C
import os

# torch FIRST: the PyTorch-ROCm wheel bundles its own libamdhip64.so.  If libtfnas_hip.so were loaded before torch, the dynamic
# loader would bind it to the system ROCm's HIP runtime instead, the process would hold two HIP runtimes, and every launch on a
# torch-allocated pointer would fail with hipErrorNoDevice (100) -- seen when build() and smoke() ran in one process.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TFNAS_LIB') or os.path.join(_HERE, 'libtfnas_hip.so')     # (TFNAS_LIB: an experiment build of the same ABI)

MAX_GROUPS, MAX_SINK, MAX_CELLS = 8, 4, 32
ACT = {'relu': 0, 'swish': 1, 'relu6': 2, 'h-swish': 3}       # the reference's spellings (models/layers.py:38-47); TFNAS_ACT_*
MODE_CELL, MODE_STEM, MODE_HEAD = 0, 1, 2
BN_EPS = 1e-5                # TfnasCellDesc.eps of every descriptor (the reference's BatchNorm eps)

_W_FIELDS = ('w_expand', 'w_dw', 'w_proj', 'w_se_r', 'b_se_r', 'w_se_e', 'b_se_e')
_G_FIELDS = ('g_expand', 'g_dw', 'g_proj', 'g_se_r', 'gb_se_r', 'g_se_e', 'gb_se_e')


GEMM_EXPLICIT, GEMM_EVERYWHERE, CELL_LAZY_JOIN = 0x1000, 0x100, 1
CELL_ACCUM_WGRAD = 0x20      # TfnasCellDesc.flags: the backward adds its weight gradients to their destinations
CELL_K7 = 0x80               # TfnasCellDesc.flags: groups may have depthwise kernel size 7 (refused without the bit)
CELL_ACTS = 0x100            # TfnasCellDesc.flags: act may be 'relu6' / 'h-swish' (refused without the bit)
CELL_NOEXPAND = 0x200        # TfnasCellDesc.flags: the one group has no expand convolution (mid == in channels; refused without the bit)
CELL_FUSED = 0x400           # TfnasCellDesc.flags: the one group is a Fused-MBConv block (dense 3 x 3 weight in w_expand, no depthwise)
CELL_KINDS = 0x800           # TfnasCellDesc.flags: every group names its own kind in TfnasGroup.kind (group_kind_id; refused without the bit)
CELL_SE_STYLE = 0x1000       # TfnasCellDesc.flags: se_style may be non-zero (se_style_id; refused without the bit)
CELL_SKIP = 0x2000           # TfnasCellDesc.flags: groups may be GROUP_SKIP, the identity candidate (with CELL_KINDS, residual cells only)
CELL_DILATION = 0x8000       # TfnasCellDesc.flags: groups may have depthwise dilation 2 (TfnasGroup.dil; not read without the bit)
CELL_MIXK = 0x10000          # TfnasCellDesc.flags: TfnasGroup.k may be a packed word -- a MixConv group (mix_k_word; refused without the bit)
PATH_EXTENDED = 1            # TfnasPathDesc.path_flags: the path may hold cells beside the plain ones (tfnas_path_plan refuses them without)
GROUP_SKIP = 3               # TfnasGroup.kind of a skip group: no width, no weights, no columns -- not a BlockKind (KINDS stays three)
SE_GATE = {'sigmoid': 0, 'h-sigmoid': 1}      # gate function of a squeeze-excite branch (bits 4-7 of TfnasCellDesc.se_style)
# TfnasCellDesc.route (include/tfnas_hip.h: TFNAS_ROUTE_*) -- every kernel-variant switch of a launch; 0 = the library's policy
ROUTE_FX_OFF, ROUTE_FOLD_OFF, ROUTE_DWWG_OFF, ROUTE_DWWG2_OFF, ROUTE_XG_OFF, ROUTE_XG_ALL = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
ROUTE_DW = {'auto': 0, 'direct': 1 << 6, 'lds': 2 << 6, 'tiled': 3 << 6}
ROUTE_SE = {'wave': 0, 'fused': 1 << 8, 'gemm': 2 << 8}
ROUTE_WGRAD_INLINE, ROUTE_GRAM2 = 0x400, 0x800
ROUTE_TAKEN_VALID, ROUTE_TAKEN_FX = 1, 2
GEMM_MODES = {'f32': 0, 'bf16': 1, 'x2': 3, 'x3': 6}


def act_id(name):
    """TFNAS_ACT_* of an activation name; ValueError (naming the legal ones) for any other."""
    try:
        return ACT[name]
    except (KeyError, TypeError):
        raise ValueError('tfnas_amd: unknown activation %r (one of %s)' % (name, ', '.join(repr(a) for a in ACT))) from None


def act_flags(act):
    """TfnasCellDesc.flags bit a descriptor with activation id ``act`` needs (the library takes the two newer activations only
    from callers that say they know them)."""
    return CELL_ACTS if act in (ACT['relu6'], ACT['h-swish']) else 0


def se_style_id(se_act=None, se_gate='sigmoid'):
    """TfnasCellDesc.se_style of a squeeze-excite style: ``se_act`` the hidden activation (None: the block's own; else one of
    ACT's names), ``se_gate`` 'sigmoid' or 'h-sigmoid'.  0 is the reference's branch.  ValueError names the legal spellings."""
    if se_act is not None and (not isinstance(se_act, str) or se_act not in ACT):
        raise ValueError('tfnas_amd: unknown squeeze-excite activation %r (None for the block\'s own, or one of %s)'
                         % (se_act, ', '.join(repr(a) for a in ACT)))
    if not isinstance(se_gate, str) or se_gate not in SE_GATE:
        raise ValueError('tfnas_amd: unknown squeeze-excite gate %r (one of %s)' % (se_gate, ', '.join(repr(g) for g in SE_GATE)))
    return (0 if se_act is None else 1 + ACT[se_act]) | (SE_GATE[se_gate] << 4)


def se_style_flags(style):
    """TfnasCellDesc.flags bits a descriptor with ``se_style == style`` needs: CELL_SE_STYLE, and CELL_ACTS for an explicit
    'relu6' / 'h-swish' hidden activation."""
    if not style:
        return 0
    hidden = style & 0xf
    return CELL_SE_STYLE | (act_flags(hidden - 1) if hidden else 0)


def se_style_pair(style, what='se_style'):
    """A caller's ``(se_act, se_gate)`` pair, validated (None: the default pair)."""
    if style is None:
        return (None, 'sigmoid')
    try:
        se_act, se_gate = style
    except (TypeError, ValueError):
        raise ValueError('tfnas_amd: %s must be None or a (se_act, se_gate) pair, got %r' % (what, style)) from None
    se_style_id(se_act, se_gate)
    return (se_act, se_gate)


class BlockKind(collections.namedtuple('BlockKind', 'name flag fields bn_sites has_E')):
    """One kind of one-block cell -- THE table of what a kind is (its C twin: cell_kind() and the two predicates next to it in
    csrc/kernels.h).  ``flag``: its TfnasCellDesc.flags bit; ``fields``: the indices into _W_FIELDS / _G_FIELDS it binds, with SE
    (without: those below 3); ``bn_sites``: which of the three BatchNorm sites exist; ``has_E``: whether it has an E buffer."""
    __slots__ = ()

    def bound(self, se):
        """The TfnasGroup field indices a block of this kind binds, in hip_params() order (``se``: it has squeeze-excite)."""
        return self.fields if se else tuple(k for k in self.fields if k < 3)


MBCONV = BlockKind('MBCONV', 0, (0, 1, 2, 3, 4, 5, 6), (0, 1, 2), True)                    # expand, depthwise, project
NOEXPAND = BlockKind('NOEXPAND', CELL_NOEXPAND, (1, 2, 3, 4, 5, 6), (1, 2), False)         # no expand convolution: D = dw(x)
FUSED = BlockKind('FUSED', CELL_FUSED, (0, 2, 3, 4, 5, 6), (1, 2), False)                  # dense 3 x 3 weight in w_expand, no depthwise
KINDS = (MBCONV, NOEXPAND, FUSED)


def group_kind_id(kind):
    """TFNAS_GROUP_* of a BlockKind: what TfnasGroup.kind holds in a descriptor with CELL_KINDS (a cell whose candidates differ
    in kind -- not a fourth kind: every group of it has one of the three)."""
    return KINDS.index(kind)


def dilation_flags(dils):
    """TfnasCellDesc.flags bit a descriptor whose groups have the depthwise dilations ``dils`` needs: CELL_DILATION when one of
    them is dilated, nothing otherwise (an undilated descriptor is what it always was)."""
    return CELL_DILATION if any(int(v) > 1 for v in dils) else 0


MIX_KERNELS = ((3, 5), (3, 7), (5, 7), (3, 5, 7))      # the kernel sizes of a MixConv depthwise, segment by segment (ascending)


def check_mix_kernels(mix_kernels):
    """``mix_kernels`` as a tuple of ints, one of MIX_KERNELS; ValueError otherwise."""
    try:
        ks = tuple(mix_kernels)
    except TypeError:
        ks = None
    if ks not in MIX_KERNELS or not all(type(k) is int for k in ks):
        raise ValueError('tfnas_amd: mix_kernels is one of %s (got %r)' % (', '.join(map(repr, MIX_KERNELS)), mix_kernels))
    return ks


def mix_k_word(mix_kernels):
    """The packed TfnasGroup.k of a MixConv group: nibble s = the kernel size of channel segment s (0x53, 0x73, 0x75, 0x753)."""
    return sum(k << (4 * s) for s, k in enumerate(check_mix_kernels(mix_kernels)))


def mix_split(mc, n):
    """Channels of the ``n`` segments of a MixConv depthwise of ``mc`` channels (include/tfnas_hip.h, TFNAS_CELL_MIXK): the
    (mc + 3) // 4 channel quads in equal parts, the remaining quads to segment 0, the last segment cut at mc.  Where mc is a
    multiple of 4 n this is MixNet's _split_channels.  ValueError when a segment would get no quad."""
    q = (mc + 3) // 4
    if q < n:
        raise ValueError('tfnas_amd: %d channels are too few for %d kernel-size segments (a segment is at least 4 channels)' % (mc, n))
    bounds = [0] + [min(4 * (s * (q // n) + q % n), mc) for s in range(1, n + 1)]
    return [bounds[s + 1] - bounds[s] for s in range(n)]


def mixk_flags(ks):
    """TfnasCellDesc.flags bit a descriptor whose groups have the TfnasGroup.k words ``ks`` needs: CELL_MIXK when one of them is
    packed, nothing otherwise (a descriptor of plain kernel sizes is what it always was)."""
    return CELL_MIXK if any(int(k) > 0xf for k in ks) else 0


def block_k_word(block):
    """TfnasGroup.k of a block module: its kernel size, the packed word of a MixConv block (``mix_kernels``)."""
    mk = getattr(block, 'mix_kernels', None)
    return block.kernel_size if mk is None else mix_k_word(mk)


def describe_block(kind, N, H, W, ic, mc, se, oc, k, stride, act, dilation=1, mix_kernels=None):
    """A one-block TFNAS_MODE_CELL descriptor of ``kind``, before tfnas_cell_plan: the geometry words, has_res, eps and the flags
    the geometry itself asks for (CELL_K7, CELL_DILATION, CELL_MIXK, the activation's bit, the kind's bit).  ``act``: a TFNAS_ACT_*
    id; ``mix_kernels``: a MixConv block, ``k`` its largest kernel size.  Pure host code."""
    d = TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, H, W, ic, oc, stride, act, 1, MODE_CELL
    d.has_res, d.eps = int(ic == oc and stride == 1), BN_EPS
    d.g[0].mc, d.g[0].k, d.g[0].se = mc, k, se
    d.flags = (CELL_K7 if k == 7 else 0) | act_flags(act) | kind.flag
    if mix_kernels is not None:                    # (``k`` is then the largest of them: CELL_K7 above where it is 7)
        d.g[0].k = mix_k_word(mix_kernels)
        d.flags |= CELL_MIXK
    if dilation != 1:
        d.g[0].dil = dilation
        d.flags |= dilation_flags((dilation,))
    return d


class TfnasGroup(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ('mc', 'k', 'se', 'mcp', 'off', 'se_off', 'kind', 'dil')]
                + [(n, C.c_void_p) for n in _W_FIELDS] + [(n, C.c_void_p) for n in _G_FIELDS])


class TfnasCellDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ('N', 'H', 'W', 'ic', 'oc', 'stride', 'act', 'has_res', 'G', 'need_wgrad',
                                          'Ho', 'Wo', 'M', 'SE')]
                + [('eps', C.c_float), ('mode', C.c_int32), ('Hi', C.c_int32), ('Wi', C.c_int32),
                   ('stor', C.c_int32), ('gemm_mode', C.c_int32), ('flags', C.c_int32), ('g', TfnasGroup * MAX_GROUPS),
                   ('sync_fn', C.c_void_p), ('sync_user', C.c_void_p), ('sync_world', C.c_int32), ('route', C.c_int32),
                   ('fwd_route', C.c_int32), ('pad_route', C.c_int32), ('wgrad_stream', C.c_void_p * 3)])
    # TfnasCellDesc.se_style (TFNAS_SE_*: se_style_id) lives in the word that was padding before it.  The mirror keeps that word's
    # historical field name in _fields_ -- recorded descriptor dumps (tests/golden/block_kind_pin.json) list the int32 fields by
    # name -- and exposes it under the header's name.
    se_style = property(lambda self: self.pad_route, lambda self, v: setattr(self, 'pad_route', v))


class TfnasCellWs(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        'E', 'D', 'Pr', 'fsmall', 'off_pooled', 'off_gate', 'off_hpre', 'stats', 'off_stats1', 'off_stats2',
        'off_stats3', 'out', 'dZ', 'dEh', 'bsmall', 'off_dgate', 'off_dpooled', 'off_dgl', 'off_dhpre', 'off_cb1',
        'red', 'off_red3', 'off_red2', 'off_red1', 'off_resdot', 'part', 'dx', 'dxp')]


MAX_STAGES = 8


class TfnasStage(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ('ncell', 'start_res', 'first_cell', 'nres')]
                + [('betas', C.c_void_p), ('dbetas', C.c_void_p)])


class TfnasPathDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ('ncell', 'nstage', 'soft', 'need_dx0', 'efree_mask_lo', 'path_flags')]
                + [('stage', TfnasStage * MAX_STAGES), ('cell', TfnasCellDesc * MAX_CELLS)])


class TfnasPathWs(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ('saved', 'scratch', 'total', 'out_count')]
                + [(n, C.c_int32) for n in ('out_h', 'out_w', 'out_c', 'pad')])


class TfnasBnAffine(C.Structure):
    _fields_ = ([(n, C.c_void_p * 3) for n in ('weight', 'bias', 'g_weight', 'g_bias', 'running_mean', 'running_var')]
                + [('momentum', C.c_float), ('eval', C.c_int32)])


OPT_MAX_GROUPS = 8
OPT_SGD, OPT_RMSPROP, OPT_RMSPROP_TF = 0, 1, 2      # TfnasOptGroups.kind
OPT_NESTEROV = 1                                    # TfnasOptGroups.flags


class TfnasOptGroups(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ('kind', 'flags', 'ngroups')]
                + [('lr', C.c_float * OPT_MAX_GROUPS), ('wd', C.c_float * OPT_MAX_GROUPS)]
                + [(n, C.c_float) for n in ('momentum', 'alpha', 'eps', 'max_norm', 'grad_scale', 'ema_alpha')])


_P = C.c_void_p
_PP = C.POINTER(C.c_void_p)
_PROTOS = {
    'tfnas_abi_version': (C.c_int, []),
    'tfnas_shutdown': (C.c_int, []),
    'tfnas_sizeof': (C.c_uint64, [C.c_int]),
    'tfnas_cell_plan': (C.c_int, [C.POINTER(TfnasCellDesc)]),
    'tfnas_cell_ws': (C.c_int, [C.POINTER(TfnasCellDesc), C.POINTER(TfnasCellWs)]),
    'tfnas_mixedop_fwd': (C.c_int, [C.POINTER(TfnasCellDesc)] + [_P] * 10),
    'tfnas_mixedop_bwd': (C.c_int, [C.POINTER(TfnasCellDesc)] + [_P] * 17),
    'tfnas_mbconv_fwd': (C.c_int, [C.POINTER(TfnasCellDesc), C.POINTER(TfnasBnAffine)] + [_P] * 10),
    'tfnas_mbconv_bwd': (C.c_int, [C.POINTER(TfnasCellDesc), C.POINTER(TfnasBnAffine)] + [_P] * 17),
    'tfnas_head_affine_fwd': (C.c_int, [C.POINTER(TfnasCellDesc), C.POINTER(TfnasBnAffine)] + [_P] * 6),
    'tfnas_head_affine_bwd': (C.c_int, [C.POINTER(TfnasCellDesc), C.POINTER(TfnasBnAffine)] + [_P] * 11),
    'tfnas_head_fwd': (C.c_int, [C.POINTER(TfnasCellDesc)] + [_P] * 6),
    'tfnas_head_bwd': (C.c_int, [C.POINTER(TfnasCellDesc)] + [_P] * 11),
    'tfnas_head_wgrad': (C.c_int, [C.POINTER(TfnasCellDesc)] + [_P] * 6),
    'tfnas_cls_ce': (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_float, _P, _P, _P, _P, _P]),
    'tfnas_cls_wgrad': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _PP, _PP, _PP, C.c_float, _P, _P, _P, _P]),
    'tfnas_cls_wgrad_ex': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _PP, _PP, _PP, _P, C.c_float, _P, _P, _P, _P, _P]),
    'tfnas_cls_ce_ex': (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P]),
    'tfnas_cls_reduce': (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    'tfnas_add_into': (C.c_int, [_P, _P, C.c_uint64, _P]),
    'tfnas_path_create': (C.c_int, [C.POINTER(C.c_void_p)]),
    'tfnas_path_destroy': (C.c_int, [C.c_void_p]),
    'tfnas_path_set_side_stream': (C.c_int, [C.c_void_p, C.c_void_p]),
    'tfnas_path_set_wgrad_accum': (C.c_int, [C.c_void_p, C.c_uint32]),
    'tfnas_set_stats_sync': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    'tfnas_path_plan': (C.c_int, [C.c_void_p, C.POINTER(TfnasPathDesc), C.POINTER(TfnasPathWs)]),
    'tfnas_paths_fwd': (C.c_int, [C.c_int] + [_PP] * 8),
    'tfnas_paths_bwd': (C.c_int, [C.c_int] + [_PP] * 11 + [C.c_int, C.c_int]),
    'tfnas_pack_ranges': (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _P]),
    'tfnas_sgd_clip_step': (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64), C.c_float, C.c_float,
                                      C.c_float, C.c_float, C.c_float, _P, C.c_uint64, _P, _P]),
    'tfnas_sgd_clip_ema_step': (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64), C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                          _P, C.c_float, _P, C.c_uint64, _P, _P]),
    'tfnas_ema_lerp': (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_float, _P]),
    'tfnas_opt_groups_step': (C.c_int, [C.POINTER(TfnasOptGroups), _P, _P, _P, _P, _P, _P, C.c_uint64, _P, C.c_uint64, _P, _P]),
    'tfnas_arch_adam_project': (C.c_int, [C.c_int, _PP, _PP, C.POINTER(C.c_int32), _P, _P, C.c_float, C.c_float, C.c_float,
                                          C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, _P, _P]),
    'tfnas_arch_fwd': (C.c_int, [C.c_int, C.POINTER(_P), _P, _P, C.c_float, _P, _P, _P]),
    'tfnas_arch_bwd': (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_float, C.POINTER(_P), _P]),
    'tfnas_efree_supported': (C.c_int, [C.POINTER(TfnasCellDesc)]),
    'tfnas_fx_supported': (C.c_int, [C.POINTER(TfnasCellDesc)]),
    'tfnas_cell_route': (C.c_int, [C.POINTER(TfnasCellDesc)]),
    'tfnas_arch_project': (C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(C.c_int32), _P]),
    'tfnas_arch_sample': (C.c_int, [C.c_int, C.POINTER(_P), _P, _P, C.c_float, C.c_int, _P, _P]),
    'tfnas_sink_fwd': (C.c_int, [C.c_int, _P, C.POINTER(_P), _P, C.c_uint64, _P, _P, _P, _P]),
    'tfnas_prof_enable': (C.c_int, [C.c_uint]),
    'tfnas_set_lazy_join': (C.c_int, [C.c_int]),
    'tfnas_set_gemm_mode': (C.c_int, [C.c_int]),
    'tfnas_gemm_mode': (C.c_int, []),
    'tfnas_side_stream': (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    'tfnas_side_join': (C.c_int, [_P]),
    'tfnas_prof_count': (C.c_int, []),
    'tfnas_prof_name': (C.c_char_p, [C.c_int]),
    'tfnas_prof_collect': (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    'tfnas_prof_last_split': (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    'tfnas_sink_bwd': (C.c_int, [C.c_int, _P, C.POINTER(_P), _P, _P, _P, C.c_uint64, C.POINTER(_P), _P, _P, _P, _P]),
}

_lib_handle = None


def lib():
    """Load (once) and return the shared library; raises RuntimeError when it is absent."""
    global _lib_handle
    l = _lib_handle
    if l is None:
        path = LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                'tfnas_amd: HIP extension %s is missing -- run `python -c "import __graft_entry__ as g; g.build()"` '
                '(or `make -C tf-nas_amd/csrc`). There is no CPU/PyTorch fallback for the MixedOP hot path.' % path)
        l = C.CDLL(path)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(l, name)        # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if l.tfnas_abi_version() != 4:
            raise RuntimeError('tfnas_amd: ABI version mismatch')
        for which, st in enumerate((TfnasGroup, TfnasCellDesc, TfnasCellWs, TfnasStage, TfnasPathDesc, TfnasPathWs, TfnasBnAffine)):
            if l.tfnas_sizeof(which) != C.sizeof(st):
                raise RuntimeError('tfnas_amd: struct layout mismatch for %s' % st.__name__)
        if l.tfnas_sizeof(9) != C.sizeof(TfnasOptGroups):
            raise RuntimeError('tfnas_amd: struct layout mismatch for TfnasOptGroups')
        # the library reads no environment variable (ABI 4): TFNAS_GEMM only seeds its process-wide default here
        g = os.environ.get('TFNAS_GEMM')
        if g is not None:
            if g not in GEMM_MODES:
                raise RuntimeError('tfnas_amd: TFNAS_GEMM must be one of %s' % sorted(GEMM_MODES))
            if l.tfnas_set_gemm_mode(GEMM_MODES[g]) != 0:
                raise RuntimeError('tfnas_amd: tfnas_set_gemm_mode failed')
        _lib_handle = l
    return l


def check(rc, what):
    if rc != 0:
        raise RuntimeError('tfnas_hip: %s failed with code %d (%s)' % (
            what, rc, 'invalid argument' if rc < 0 else 'hipError_t'))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def raw_array(values):
    """(void* x n) from raw integers / None."""
    arr = (C.c_void_p * len(values))()
    for i, v in enumerate(values):
        arr[i] = v
    return arr


def exported_names():
    return list(_PROTOS)
