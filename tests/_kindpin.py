"""What tests/golden/block_kind_pin.json records and tests/test_block_kind.py replays: the descriptor words, workspace, pointer
binding and BatchNorm-site pattern of every block kind's plan (plain MBConv, expand-free, Fused-MBConv), of a two-candidate plan
and of the stem and head plans; the blocks' state_dict keys and seeded initialisation; the hand-written MAC / parameter counts of
the three derived-network configurations.  Only names that exist before and after the block-kind table are used here (CellPlan,
.desc, .bind, hip_params, bn_sites, functions._bn_struct, Network.stem_plan / head_plan), so the generator records the code that
was there before the table (tests/golden/make_golden_kind.py) and the test replays the same calls on the code that is there now."""
import itertools
from collections import OrderedDict

import torch

GEOM = dict(N=2, ic=16, H=9, W=13, mid=40)
KINDS = ('plain', 'noexp', 'fused')
BLOCK_CASES = [(kind, se, s, aff, 3, 'relu') for kind, se, s, aff in itertools.product(KINDS, (0, 8), (1, 2), (False, True))]
BLOCK_CASES += [('plain', 8, 1, False, 7, 'relu'), ('plain', 0, 2, False, 3, 'h-swish')]
FORMS = [(kind, aff) for kind in KINDS for aff in (False, True)]        # the six block forms (SE 8, stride 1)


def case_tag(case):
    return '%s_se%d_s%d_%s_k%d_%s' % (case[0], case[1], case[2], 'affine' if case[3] else 'search', case[4], case[5])


def make_block(kind, se, stride, affine, k=3, act='relu'):
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock
    cls = FusedMBConvBlock if kind == 'fused' else MBInvertedResBlock
    mid = GEOM['ic'] if kind == 'noexp' else GEOM['mid']
    return cls(GEOM['ic'], mid, se, 16 if stride == 1 else 24, k, stride, affine=affine, act_func=act)


def _int_fields(st):
    import ctypes as C
    return OrderedDict((n, int(getattr(st, n))) for n, t in st._fields_ if t is C.c_int32)


def _index(ptr, tensors):
    hits = [i for i, t in enumerate(tensors) if t.data_ptr() == ptr]
    assert len(hits) <= 1
    return hits[0] if hits and ptr else -1


def record_plan(plan, N, H, W, params, bns=None):
    """The recorded facts of one launch's descriptor: after desc() + bind(params, grads) (and _bn_struct of the sites ``bns``)."""
    from tfnas_amd import _lib, functions
    grads = [torch.empty_like(p) for p in params]
    d, ws = plan.desc(N, H, W)
    plan.bind(d, params, grads)
    out = OrderedDict(ints=_int_fields(d))
    out['groups'] = [list(_int_fields(d.g[g]).values()) for g in range(_lib.MAX_GROUPS)]
    out['ws'] = OrderedDict((n, int(getattr(ws, n))) for n, _ in ws._fields_)
    out['ptr'] = [[_index(getattr(d.g[g], f), params) for f in _lib._W_FIELDS]
                  + [_index(getattr(d.g[g], f), grads) for f in _lib._G_FIELDS] for g in range(d.G)]
    out['bn'] = None
    if bns is not None:
        gbn = [torch.zeros_like(t) for m in bns if m is not None for t in (m.weight, m.bias)]
        a = functions._bn_struct(bns, True, gbn)
        out['bn'] = OrderedDict((n, [int(bool(getattr(a, n)[i])) for i in range(3)])
                                for n in ('weight', 'bias', 'g_weight', 'g_bias', 'running_mean', 'running_var'))
    return out


def record_block_case(case):
    from tfnas_amd.functions import CellPlan
    kind, se, stride, affine, k, act = case
    blk = make_block(kind, se, stride, affine, k, act)
    plan = CellPlan(blk.in_channels, blk.out_channels, blk.stride, blk.act_func, [blk])
    return record_plan(plan, GEOM['N'], GEOM['H'], GEOM['W'], blk.hip_params(), blk.bn_sites() if affine else None)


def record_other_plans():
    """A two-candidate plain plan, and the stem and head plans as model_search.Network builds them."""
    from tfnas_amd import geometry
    from tfnas_amd.functions import CellPlan
    from tfnas_amd.layers import MBInvertedResBlock
    from tfnas_amd.model_search import Network
    out = OrderedDict()
    blocks = [MBInvertedResBlock(16, 40, 8, 24, 3, 2), MBInvertedResBlock(16, 52, 0, 24, 5, 2)]
    plan = CellPlan(16, 24, 2, 'relu', blocks)
    out['two_candidates'] = record_plan(plan, GEOM['N'], GEOM['H'], GEOM['W'], plan.params())
    net = Network(10, geometry.initial_mc_num_dddict(), {'base': 0.0})
    plan = net.stem_plan()
    out['stem'] = record_plan(plan, 2, 18, 26, plan.params())
    out['head'] = record_plan(net.head_plan(), 2, 5, 7, [net.feature_mix_layer.conv.weight])
    return out


def record_forms():
    """state_dict keys and the seeded initialisation (probes of the first and the last parameter) of the six block forms."""
    import _golden
    keys, seeded = OrderedDict(), OrderedDict()
    for kind, affine in FORMS:
        tag = '%s_%s' % (kind, 'affine' if affine else 'search')
        torch.manual_seed(0)
        blk = make_block(kind, 8, 1, affine)
        keys[tag] = list(blk.state_dict())
        ps = list(blk.parameters())
        seeded[tag] = [_golden.probe(ps[0]).tolist(), _golden.probe(ps[-1]).tolist()]
    return keys, seeded


def network_configs():
    import _fused
    import _k7
    import _noexp
    return OrderedDict(k7=_k7.k7_network_config(), noexp=_noexp.noexp_network_config(), fused=_fused.fused_network_config())


HAND_SIZES = (64, 224)
