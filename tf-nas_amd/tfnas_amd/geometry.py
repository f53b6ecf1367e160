"""Supernet geometry tables for the TF-NAS search space.

The reference keeps these as ~400 lines of literal tables (``tools/config.py:4-197`` ``mc_mask_dddict``
and ``tools/config.py:200-393`` ``lat_lookup_key_dddict``).  Here they are *derived* from the cell geometry
that ``models/model_search.py:219-275`` hard-codes, so that the HIP planner, the oracle and the latency API
all read one source of truth.  ``tests/test_oracle_vs_reference.py`` proves the derived tables equal the
reference's literal ones (container only).

Vocabulary (reference's): a *stage* holds K *blocks* (= MixedOP *cells*); every cell has 8 candidate
*ops*; each op has a *mid_channels* width that the search may shrink/expand ("elasticity scaling").
"""
from collections import OrderedDict

# candidate order == index into m_ops / log_alphas (model_search.py:7-29)
PRIMITIVES = [
    'MBI_k3_e3', 'MBI_k3_e6', 'MBI_k5_e3', 'MBI_k5_e6',
    'MBI_k3_e3_se', 'MBI_k3_e6_se', 'MBI_k5_e3_se', 'MBI_k5_e6_se',
]
NUM_OPS = len(PRIMITIVES)

# per-candidate static attributes: kernel size, nominal expand ratio, SE width as a multiple of ic
OP_KERNEL = (3, 3, 5, 5, 3, 3, 5, 5)
OP_EXPAND = (3, 6, 3, 6, 3, 6, 3, 6)
OP_SE_MULT = (0, 0, 0, 0, 1, 2, 1, 2)

# Every named primitive a cell may hold (model_search.OPS builds the modules; ``primitives=`` of MixedOP / MixedStage / Network
# chooses 8 per cell, PRIMITIVES by default): name -> (layer class, kernel size, SE width as a multiple of ic, own width).
# own width False: the block is as wide as mc_num_dict[i] says; True ('DS_*', expand-free): mid = ic whatever it says.
PRIMITIVE_SPECS = OrderedDict(
    [(n, ('MBInvertedResBlock', OP_KERNEL[i], OP_SE_MULT[i], False)) for i, n in enumerate(PRIMITIVES)]
    + [('MBI_k7_%s%s' % (e, '_se' if se else ''), ('MBInvertedResBlock', 7, se, False)) for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))]
    + [('FMB_k3_%s%s' % (e, '_se' if se else ''), ('FusedMBConvBlock', 3, se, False)) for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))]
    + [('DS_k%d%s' % (k, '_se' if se else ''), ('MBInvertedResBlock', k, se, True)) for k in (3, 5) for se in (0, 1)])

# The dilated primitives (model_search.DILATED_OPS builds the modules): depthwise taps two pixels apart, everything else like their
# undilated twins -- 'MBI_k3d2_e6_se' is 'MBI_k3_e6_se' with dilation 2, 'DS_k5d2' is 'DS_k5' with dilation 2 (the dil_conv_3x3 /
# dil_conv_5x5 of the DARTS-family spaces).  They have the same four words in PRIMITIVE_SPECS as every primitive; the dilation is
# a table of its own (primitive_dilation), 1 for every name that is not in it.
PRIMITIVE_DILATION = OrderedDict(
    [('MBI_k%dd2_%s%s' % (k, e, '_se' if se else ''), 2) for k in (3, 5) for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))]
    + [('DS_k%dd2%s' % (k, '_se' if se else ''), 2) for k in (3, 5) for se in (0, 1)])
PRIMITIVE_SPECS.update(
    [('MBI_k%dd2_%s%s' % (k, e, '_se' if se else ''), ('MBInvertedResBlock', k, se, False))
     for k in (3, 5) for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))]
    + [('DS_k%dd2%s' % (k, '_se' if se else ''), ('MBInvertedResBlock', k, se, True)) for k in (3, 5) for se in (0, 1)])

# The MixConv primitives (model_search.MIX_OPS builds the modules): one depthwise convolution whose channel segments have the kernel
# sizes of PRIMITIVE_MIX -- 'MBI_k35_e6_se' is 'MBI_k5_e6_se' with channel segments 3 x 3 | 5 x 5, 'DS_k357' an expand-free block
# with 3 x 3 | 5 x 5 | 7 x 7.  The same four words in PRIMITIVE_SPECS as every primitive (the kernel size: the largest of them);
# the segments are a table of its own (primitive_mix_kernels), None for every name that is not in it.
PRIMITIVE_MIX = OrderedDict(
    [('MBI_k%s_%s%s' % (tag, e, '_se' if se else ''), ks)
     for tag, ks in (('35', (3, 5)), ('357', (3, 5, 7))) for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))]
    + [('DS_k%s%s' % (tag, '_se' if se else ''), ks) for tag, ks in (('35', (3, 5)), ('357', (3, 5, 7))) for se in (0, 1)])
PRIMITIVE_SPECS.update(
    [('MBI_k%s_%s%s' % (tag, e, '_se' if se else ''), ('MBInvertedResBlock', max(ks), se, False))
     for tag, ks in (('35', (3, 5)), ('357', (3, 5, 7))) for e, se in (('e3', 0), ('e6', 0), ('e3', 1), ('e6', 2))]
    + [('DS_k%s%s' % (tag, '_se' if se else ''), ('MBInvertedResBlock', max(ks), se, True))
       for tag, ks in (('35', (3, 5)), ('357', (3, 5, 7))) for se in (0, 1)])


SKIP = 'skip'        # the identity candidate (the reference's commented-out primitive): recognised NEXT to PRIMITIVE_SPECS -- it
                     # has no layer spec (no kernel, no width, no SE) and only residual cells can hold it (residual_cells)


def cell_primitives(primitives, stage, block):
    """The 8 candidate names of cell (stage, block) under a ``primitives`` argument: None -> PRIMITIVES; one list -> that list for
    every cell; a {stage: {block: list}} mapping -> its entry, PRIMITIVES where it has none."""
    if isinstance(primitives, dict):
        primitives = (primitives.get(stage) or {}).get(block)
    return list(PRIMITIVES) if primitives is None else list(primitives)


def cell_se_style(se_style, stage, block):
    """The (se_act, se_gate) pair of cell (stage, block) under an ``se_style`` argument: None -> the default (None, 'sigmoid');
    one pair -> that pair for every cell; a {stage: pair} or {stage: {block: pair}} mapping -> its entry, the default where it
    has none."""
    if isinstance(se_style, dict):
        se_style = se_style.get(stage)
        if isinstance(se_style, dict):
            se_style = se_style.get(block)
    if se_style is None:
        return (None, 'sigmoid')
    se_act, se_gate = se_style
    return (se_act, se_gate)


def se_style_keys(se_act, se_gate):
    """The keys a block's config carries for its squeeze-excite style: only what differs from the default, so that the config of
    an unstyled block is what it always was."""
    keys = {}
    if se_act is not None:
        keys['se_act'] = se_act
    if se_gate != 'sigmoid':
        keys['se_gate'] = se_gate
    return keys


def primitive_block(name, ic, mc):
    """(layer class name, mid_channels, se_channels, kernel_size) of primitive ``name`` in a cell of ``ic`` input channels whose
    width table says ``mc``; ValueError (naming the legal ones) for an unknown name.  'skip': ('IdentityLayer', 0, 0, 0) -- the
    same four words with nothing in them, so callers that unpack the answer keep working and fork on the layer name."""
    if name == SKIP:
        return 'IdentityLayer', 0, 0, 0
    if name not in PRIMITIVE_SPECS:
        raise ValueError('tfnas_amd: unknown primitive %r (one of %s)' % (name, ', '.join(sorted(PRIMITIVE_SPECS))))
    layer, k, se_mult, own = PRIMITIVE_SPECS[name]
    return layer, (ic if own else mc), ic * se_mult, k


def primitive_dilation(name):
    """Depthwise dilation of primitive ``name``: 2 for the dilated ones (PRIMITIVE_DILATION), 1 for every other registered name
    and for 'skip'; ValueError for an unknown name, as primitive_block."""
    primitive_block(name, 4, 4)
    return PRIMITIVE_DILATION.get(name, 1)


def dilation_keys(dilation):
    """The key a block's config carries for its depthwise dilation: only where it is not 1, so that the config of an undilated
    block is what it always was (se_style_keys is the pattern)."""
    return {'dilation': dilation} if dilation != 1 else {}


def primitive_mix_kernels(name):
    """Kernel sizes of the channel segments of primitive ``name``: (3, 5) / (3, 5, 7) for the MixConv ones (PRIMITIVE_MIX), None
    for every other registered name and for 'skip'; ValueError for an unknown name, as primitive_block."""
    primitive_block(name, 4, 4)
    return PRIMITIVE_MIX.get(name)


def mix_keys(mix_kernels):
    """The key a block's config carries for its MixConv segments: only where it has them, so that the config of every other block
    is what it always was (dilation_keys is the pattern)."""
    return {'mix_kernels': [int(k) for k in mix_kernels]} if mix_kernels is not None else {}


def kernel_tag(k, dilation=1, mix_kernels=None):
    """How a latency-table key spells a depthwise kernel: 'k3', 'k5', 'k7'; 'k3d2' / 'k5d2' with dilation 2; 'k35' / 'k357' (the
    segments' sizes in a row) for a MixConv block."""
    if mix_kernels is not None:
        return 'k' + ''.join('%d' % v for v in mix_kernels)
    return 'k%d' % k if dilation == 1 else 'k%dd%d' % (k, dilation)


# stage -> (in_channels[], out_channels[], strides[], act, stage_type)   (model_search.py:221-275)
STAGES = OrderedDict([
    ('stage1', dict(ics=[16, 24], ocs=[24, 24], ss=[2, 1], act='relu', stage_type=1)),
    ('stage2', dict(ics=[24, 40, 40], ocs=[40, 40, 40], ss=[2, 1, 1], act='swish', stage_type=2)),
    ('stage3', dict(ics=[40, 80, 80, 80], ocs=[80, 80, 80, 80], ss=[2, 1, 1, 1], act='swish', stage_type=3)),
    ('stage4', dict(ics=[80, 112, 112, 112], ocs=[112, 112, 112, 112], ss=[1, 1, 1, 1], act='swish', stage_type=3)),
    ('stage5', dict(ics=[112, 192, 192, 192], ocs=[192, 192, 192, 192], ss=[2, 1, 1, 1], act='swish', stage_type=3)),
    ('stage6', dict(ics=[192], ocs=[320], ss=[1], act='swish', stage_type=0)),
])

INPUT_SIZE_AFTER_STEMS = 112  # 224 / 2 (first_stem stride 2; second_stem stride 1)


def iter_cells(input_size=INPUT_SIZE_AFTER_STEMS):
    """Yield (stage, block, ic, oc, stride, act, in_size) for the 18 cells in module order."""
    size = input_size
    for stage, cfg in STAGES.items():
        for b, (ic, oc, s) in enumerate(zip(cfg['ics'], cfg['ocs'], cfg['ss']), start=1):
            yield stage, 'block%d' % b, ic, oc, s, cfg['act'], size
            size = (size + s - 1) // s if s > 1 else size


def residual_cells():
    """Yield the (stage, block) pairs whose cell has a residual connection (in == out channels, stride 1): the cells that can hold
    a 'skip' candidate.  {st: {b: names} for st, b in residual_cells()}-style mappings are what ``primitives=`` takes."""
    for stage, block, ic, oc, s, act, size in iter_cells():
        if ic == oc and s == 1:
            yield stage, block


def max_mid_channels(ic, op_idx):
    """Upper width bound of a candidate: ic*4 for e3 ops, ic*8 for e6 ops (tools/config.py:7-14)."""
    return ic * (4 if OP_EXPAND[op_idx] == 3 else 8)


def init_mid_channels(ic, op_idx):
    """Initial active width = 3/4 of the max (ic*3 / ic*6)."""
    return ic * OP_EXPAND[op_idx]


def se_channels(ic, op_idx):
    return ic * OP_SE_MULT[op_idx]


def make_mc_mask_dddict():
    """Equivalent of tools/config.py ``mc_mask_dddict``: 0/1 float masks over the max width."""
    import torch
    d = OrderedDict()
    for stage, block, ic, oc, s, act, size in iter_cells():
        d.setdefault(stage, OrderedDict())[block] = OrderedDict(
            (i, torch.cat((torch.ones(init_mid_channels(ic, i)),
                           torch.zeros(max_mid_channels(ic, i) - init_mid_channels(ic, i)))))
            for i in range(NUM_OPS))
    return d


def lut_key(size, ic, se, oc, k, stride, act, dilation=1, mix_kernels=None):
    """LUT key format of MixedOP.get_lookup_latency (model_search.py:99-107); a dilated block writes 'k3d2' / 'k5d2' where an
    undilated one writes 'k3' / 'k5', a MixConv block 'k35' / 'k357'."""
    return 'MBInvertedResBlock_{}_{}_{}_{}_{}_s{}_{}'.format(size, ic, se, oc, kernel_tag(k, dilation, mix_kernels), stride, act)


def make_lat_lookup_key_dddict():
    """Equivalent of tools/config.py ``lat_lookup_key_dddict``."""
    d = OrderedDict()
    for stage, block, ic, oc, s, act, size in iter_cells():
        d.setdefault(stage, OrderedDict())[block] = OrderedDict(
            (i, lut_key(size, ic, se_channels(ic, i), oc, OP_KERNEL[i], s, act)) for i in range(NUM_OPS))
    return d


def get_mc_num_dddict(mc_mask_dddict, is_max=False):
    """Mask -> channel counts (same contract as parsing_model.py:76-88)."""
    out = OrderedDict()
    for stage, blocks in mc_mask_dddict.items():
        out[stage] = OrderedDict()
        for block, ops in blocks.items():
            out[stage][block] = OrderedDict(
                (i, int(m.size(0)) if is_max else int(m.sum().item())) for i, m in ops.items())
    return out


def uniform_mc_num_dddict(e3_mult, e6_mult):
    """Widths ic*e3_mult / ic*e6_mult for every cell (BASELINE config 4 width sweep)."""
    d = OrderedDict()
    for stage, block, ic, oc, s, act, size in iter_cells():
        d.setdefault(stage, OrderedDict())[block] = OrderedDict(
            (i, ic * (e3_mult if OP_EXPAND[i] == 3 else e6_mult)) for i in range(NUM_OPS))
    return d


def initial_mc_num_dddict():
    return uniform_mc_num_dddict(3, 6)
