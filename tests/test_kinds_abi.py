"""CPU-side checks of TFNAS_CELL_KINDS (include/tfnas_hip.h: a kind per group -- plain, expand-free and Fused-MBConv candidates in
ONE cell), through ctypes as tests/test_fused_abi.py does: the constant and the struct sizes; every rule of the plan, accepted with
the bit and refused without it exactly as before; the all-plain flagged descriptor and the one-group flagged descriptor plan, size
and route like their unflagged twins at the supernet's 18 cell geometries; E = 0 without a plain group; the affine entry points
refuse the bit; then the Python side: the CellPlan keyword and its binding, the registry names, ``primitives=`` as a list and as a
mapping, the state_dict order."""
import ctypes as C
import os
import re

import pytest

import _kinds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL, ENULL, ERANGE = -1, -2, -3
GEO = dict(N=2, H=7, W=9, ic=8, oc=8)


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _fields(st):
    return {f: getattr(st, f) for f, _ in st._fields_}


def _ws(lib, d):
    from tfnas_amd import _lib
    ws = _lib.TfnasCellWs()
    assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == 0
    return ws


def test_header_defines_the_flag_and_keeps_version_and_sizes(lib):
    from tfnas_amd import _lib
    src = open(HEADER).read()
    m = re.search(r'#define TFNAS_CELL_KINDS (0x[0-9a-fA-F]+)', src)
    assert m and int(m.group(1), 16) == _lib.CELL_KINDS == 0x800
    for name, val in (('MBCONV', 0), ('NOEXPAND', 1), ('FUSED', 2)):
        assert re.search(r'#define TFNAS_GROUP_%s %d\b' % (name, val), src)
        assert _lib.group_kind_id(getattr(_lib, name)) == val
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src) and lib.tfnas_abi_version() == 4
    # the word that became TfnasGroup.kind was padding: no struct moved
    assert (int(lib.tfnas_sizeof(0)), int(lib.tfnas_sizeof(1)), int(lib.tfnas_sizeof(2))) == (144, C.sizeof(_lib.TfnasCellDesc), 224)
    assert C.sizeof(_lib.TfnasGroup) == 144 and _lib.TfnasGroup.kind.offset == 24
    assert [k.name for k in _lib.KINDS] == ['MBCONV', 'NOEXPAND', 'FUSED']           # "mixed" is not a fourth kind


@pytest.mark.parametrize('cands', [_kinds.EIGHT, _kinds.THREE, _kinds.TILE5, [('F', 22, 0), ('N', 3, 0)],
                                   [('F', m, 0) for m in (5, 9, 22, 31, 8, 13, 50, 7)]], ids=lambda c: 'G%d' % len(c))
@pytest.mark.parametrize('stride', (1, 2))
def test_plan_accepts_mixed_cells_and_refuses_them_without_the_bit(lib, cands, stride):
    from tfnas_amd import _lib
    d = _kinds.mixed_desc(cands, stride=stride, act=1, **GEO)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    off = 0
    for g, c in enumerate(cands):
        mc = d.g[g].mc
        assert d.g[g].mcp == (mc + 3) & ~3 and d.g[g].off == off and off % 32 == 0
        off = (off + d.g[g].mcp + 31) & ~31
    assert d.M >= off and d.SE == sum(d.g[g].se for g in range(len(cands)))
    ws = _ws(lib, d)
    P = 2 * 7 * 9
    has_plain = any(c[0] == 'M' for c in cands)
    assert ws.E == (P * d.M if has_plain else 0)                           # E = 0 without a plain group
    assert ws.dEh == P * d.M and ws.dx == P * 8 and ws.D == 2 * d.Ho * d.Wo * d.M
    if not has_plain:
        assert ws.dxp == 4
    assert lib.tfnas_efree_supported(C.byref(d)) == 0 and lib.tfnas_fx_supported(C.byref(d)) == 0
    assert lib.tfnas_cell_route(C.byref(d)) == 1
    # without the bit the kind word is not read: the same words are a cell of plain groups, and what is no plain group is refused
    # as it always was (a one-block kind bit with G > 1)
    for flags in (_lib.CELL_NOEXPAND, _lib.CELL_FUSED):
        e = _kinds.mixed_desc(cands, stride=stride, act=1, flags=flags | _lib.CELL_K7, **GEO)
        assert lib.tfnas_cell_plan(C.byref(e)) == EINVAL
    e = _kinds.mixed_desc(cands, stride=stride, act=1, flags=_lib.CELL_K7, **GEO)
    p = _kinds.mixed_desc(cands, stride=stride, act=1, flags=_lib.CELL_K7, kinds=[0] * len(cands), **GEO)
    assert lib.tfnas_cell_plan(C.byref(e)) == 0 and lib.tfnas_cell_plan(C.byref(p)) == 0
    assert _fields(_ws(lib, e)) == _fields(_ws(lib, p)) and _ws(lib, e).E == P * e.M


def test_refusals(lib):
    from tfnas_amd import _lib
    K = _lib.CELL_KINDS
    ok = lambda **kw: _kinds.mixed_desc(_kinds.THREE, **dict(GEO, **kw))      # noqa: E731
    assert lib.tfnas_cell_plan(C.byref(ok())) == 0
    # either one-block bit beside it
    for bit in (_lib.CELL_NOEXPAND, _lib.CELL_FUSED):
        assert lib.tfnas_cell_plan(C.byref(ok(flags=K | bit))) == EINVAL
    # a kind outside 0..2
    for bad in (-1, 3, 77):
        assert lib.tfnas_cell_plan(C.byref(ok(kinds=[0, bad, 2]))) == EINVAL
    # NOEXPAND: mc == ic, no expand pointer
    d = ok()
    d.g[1].mc = 12
    assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    for field in ('w_expand', 'g_expand'):
        d = ok()
        setattr(d.g[1], field, 256)
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    # FUSED: k == 3, no depthwise pointer
    d = ok(flags=K | _lib.CELL_K7)
    for k in (5, 7):
        d.g[2].k = k
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    for field in ('w_dw', 'g_dw'):
        d = ok()
        setattr(d.g[2], field, 256)
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    # the other opt-in bits apply as before
    assert lib.tfnas_cell_plan(C.byref(_kinds.mixed_desc(_kinds.EIGHT, flags=K, **GEO))) == EINVAL         # k = 7 without its bit
    assert lib.tfnas_cell_plan(C.byref(ok(act=2, flags=K))) == EINVAL                                        # relu6 without its bit
    assert lib.tfnas_cell_plan(C.byref(ok(act=2))) == 0 and lib.tfnas_cell_plan(C.byref(ok(act=3))) == 0
    # cell mode only
    stem = _kinds.mixed_desc([('M', 32, 3, 8)], 2, 0, 0, 27, 16, mode=_lib.MODE_STEM)
    stem.Hi = stem.Wi = 32
    assert lib.tfnas_cell_plan(C.byref(stem)) == EINVAL
    stem.flags = 0
    assert lib.tfnas_cell_plan(C.byref(stem)) == 0
    head = _kinds.mixed_desc([('M', 320, 3, 0)], 2, 7, 7, 320, 4, mode=_lib.MODE_HEAD)
    assert lib.tfnas_cell_plan(C.byref(head)) == EINVAL
    head.flags = 0
    assert lib.tfnas_cell_plan(C.byref(head)) == 0
    # the entry points re-check a descriptor changed after its plan, before any pointer is looked at
    one = C.c_void_p(16)
    d = ok()
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d.g[2].k = 5
    assert lib.tfnas_mixedop_fwd(C.byref(d), one, one, one, one, one, one, one, one, one, None) == EINVAL
    d.g[2].k, d.g[1].kind = 3, 3
    assert lib.tfnas_mixedop_bwd(C.byref(d), one, one, one, one, one, one, one, one, one, one, one, one, one, None, None, None,
                                 None) == EINVAL
    # a plain group needs its E buffer: no E-free form of a mixed cell
    d = ok()
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    assert lib.tfnas_mixedop_fwd(C.byref(d), one, one, None, one, one, one, one, one, one, None) == ENULL
    # the affine entry points refuse the bit, even on a one-group descriptor they would otherwise run
    bn = _lib.TfnasBnAffine()
    for cands in ([('M', 22, 3, 0)], [('N', 3, 0)], [('F', 22, 0)]):
        d = _kinds.mixed_desc(cands, **GEO)
        assert lib.tfnas_cell_plan(C.byref(d)) == 0
        assert lib.tfnas_mbconv_fwd(C.byref(d), C.byref(bn), None, one, one, one, one, one, one, one, one, None) == EINVAL
        assert lib.tfnas_mbconv_bwd(C.byref(d), C.byref(bn), None, one, one, one, one, one, one, one, None, one, one, one, one,
                                    one, None, None, None) == EINVAL


def test_size_limits_hold_per_group(lib):
    part = int(lib.tfnas_sizeof(7)) - int(lib.tfnas_sizeof(8))
    geo = dict(N=1, H=4, W=4, ic=1024, oc=16)
    # The documented rule of a Fused-MBConv block, for the SECOND fused group of a mixed cell (beside a plain group and a narrow
    # fused one): its partial row 9 ic mc, and its repacked weight 9 ic mcp (rounded up to 64 floats) next to 128 statistics rows
    # of 2 M floats, M being the cell's
    last = part // (9 * 1024)
    seen = set()
    for mc in range(last - 96, last + 8, 4):
        d = _kinds.mixed_desc([('M', 2048, 3, 0), ('F', 8, 0), ('F', mc, 0)], **geo)
        rc = lib.tfnas_cell_plan(C.byref(d))
        fits = 9 * 1024 * mc <= part and (9 * 1024 * d.g[2].mcp + 63) // 64 * 64 + 128 * 2 * d.M <= part
        assert rc == (0 if fits else ERANGE), (mc, rc, d.M)
        if rc:
            from tfnas_amd import _lib
            assert lib.tfnas_cell_ws(C.byref(d), C.byref(_lib.TfnasCellWs())) == ERANGE
        seen.add(rc)
    assert seen == {0, ERANGE}
    # the depthwise weight-gradient row (sum of mc k k) of the expand-free groups alone: eight 7 x 7 groups of 12 288 channels
    # are 4.8 M floats against the 4 Mi - 1024 of the region; seven are 4.2 M, six fit
    from tfnas_amd import _lib
    big = dict(N=1, H=4, W=4, ic=12288, oc=16)
    for n, want in ((6, 0), (7, ERANGE)):
        d = _kinds.mixed_desc([('M', 12292, 3, 0)] + [('N', 7, 0)] * n, **big)
        assert lib.tfnas_cell_plan(C.byref(d)) == want, n


def test_all_plain_and_one_group_flagged_descriptors_equal_their_unflagged_twins(lib):
    from tfnas_amd import _lib, geometry as g
    import _fused
    import _noexp
    mcs = g.initial_mc_num_dddict()
    n = 0
    for stage, block, ic, oc, s, act, size in g.iter_cells():
        for N, need_w in ((128, 0), (4, 1)):
            ds = []
            for flagged in (False, True):
                d = _lib.TfnasCellDesc()
                d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, size, size, ic, oc, s, _lib.act_id(act), 8, 0
                d.has_res, d.eps, d.need_wgrad = int(ic == oc and s == 1), _lib.BN_EPS, need_w
                for i in range(8):
                    d.g[i].mc, d.g[i].k, d.g[i].se = mcs[stage][block][i], g.OP_KERNEL[i], g.se_channels(ic, i)
                    d.g[i].kind = 0 if flagged else 2            # (not read without the bit)
                d.flags = _lib.CELL_KINDS if flagged else 0
                assert lib.tfnas_cell_plan(C.byref(d)) == 0
                ds.append(d)
            a, b = ds
            assert (a.Ho, a.Wo, a.M, a.SE) == (b.Ho, b.Wo, b.M, b.SE)
            assert [(a.g[i].mcp, a.g[i].off, a.g[i].se_off) for i in range(8)] == [(b.g[i].mcp, b.g[i].off, b.g[i].se_off)
                                                                                   for i in range(8)]
            assert _fields(_ws(lib, a)) == _fields(_ws(lib, b))
            for fn in (lib.tfnas_cell_route, lib.tfnas_efree_supported, lib.tfnas_fx_supported):
                assert fn(C.byref(a)) == fn(C.byref(b))
            n += 1
        # one group of each non-plain kind at this cell's geometry: the flagged descriptor against the one-block bit
        for cand, old in ((('N', 5, ic), _noexp.cell_desc(4, size, size, ic, oc, 5, s, _lib.act_id(act), ic)),
                          (('F', 3 * ic, 0), _fused.cell_desc(4, size, size, ic, oc, 3 * ic, s, _lib.act_id(act), 0))):
            d = _kinds.mixed_desc([cand], 4, size, size, ic, oc, s, _lib.act_id(act))
            assert lib.tfnas_cell_plan(C.byref(d)) == 0 and lib.tfnas_cell_plan(C.byref(old)) == 0
            assert (d.M, d.SE, d.g[0].mcp) == (old.M, old.SE, old.g[0].mcp)
            assert _fields(_ws(lib, d)) == _fields(_ws(lib, old)) and _ws(lib, d).E == 0
            assert lib.tfnas_cell_route(C.byref(d)) == lib.tfnas_cell_route(C.byref(old)) == 1
    assert n == 36


@pytest.mark.gpu          # (tfnas_path_create makes streams and events: it needs a device; nothing is launched)
def test_path_level_refuses_the_bit(lib):
    from tfnas_amd import _lib
    ctx = C.c_void_p(None)
    assert lib.tfnas_path_create(C.byref(ctx)) == 0
    try:
        beta = C.c_void_p(256)
        for flags, want in ((0, 0), (_lib.CELL_KINDS, EINVAL)):
            pd = _lib.TfnasPathDesc()
            pd.ncell, pd.nstage, pd.soft, pd.need_dx0 = 1, 1, 1, 1
            pd.stage[0].ncell, pd.stage[0].start_res, pd.stage[0].betas = 1, 0, beta
            src = _kinds.mixed_desc([('M', 22 + 4 * i, 3, 0) for i in range(8)], 2, 9, 13, 16, 16, flags=flags)
            C.memmove(C.byref(pd.cell[0]), C.byref(src), C.sizeof(src))
            ws = _lib.TfnasPathWs()
            assert lib.tfnas_path_plan(ctx, C.byref(pd), C.byref(ws)) == want
    finally:
        lib.tfnas_path_destroy(ctx)


# ------------------------------------------------------------------------------------------------ Python side (host only)
def _blocks(cands, ic=8, oc=8, stride=1, act='swish'):
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock
    out = []
    for c in cands:
        if c[0] == 'M':
            out.append(MBInvertedResBlock(ic, c[1], c[3], oc, c[2], stride, act_func=act))
        elif c[0] == 'N':
            out.append(MBInvertedResBlock(ic, ic, c[2], oc, c[1], stride, act_func=act))
        else:
            out.append(FusedMBConvBlock(ic, c[1], c[2], oc, 3, stride, act_func=act))
    return out


def test_cellplan_keyword_and_binding(lib):
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan
    blocks = _blocks(_kinds.EIGHT)
    with pytest.raises(NotImplementedError):                     # without the keyword: as before
        CellPlan(8, 8, 1, 'swish', blocks)
    with pytest.raises(NotImplementedError):
        CellPlan(8, 8, 1, 'swish', blocks, mixed_kinds=False)
    plan = CellPlan(8, 8, 1, 'swish', blocks, mixed_kinds=True)
    assert plan.kind is _lib.MBCONV and plan.group_kinds == tuple(_kinds.kind_of(c) for c in _kinds.EIGHT)
    d, ws = plan.desc(2, 7, 9)
    assert d.flags & _lib.CELL_KINDS and d.flags & _lib.CELL_K7 and not d.flags & (_lib.CELL_FUSED | _lib.CELL_NOEXPAND)
    assert [d.g[g].kind for g in range(8)] == [0, 2, 1, 0, 2, 1, 0, 2]
    assert ws.E == 2 * 7 * 9 * d.M
    params = plan.params()
    plan.bind(d, params, params)                                 # (pointers only: nothing is launched)
    k = 0
    for g, b in enumerate(blocks):
        fields = b.kind.bound(b.se_channels > 0)
        for f in range(7):
            w, gr = getattr(d.g[g], _lib._W_FIELDS[f]), getattr(d.g[g], _lib._G_FIELDS[f])
            if f in fields:
                assert w == gr == params[k].data_ptr()
                k += 1
            else:
                assert w is None and gr is None                  # each group binds the fields of its OWN kind
    assert k == len(params)
    assert d.g[1].w_expand == blocks[1].fused_conv.conv.weight.data_ptr() and d.g[2].w_dw == blocks[2].depth_conv.conv.weight.data_ptr()
    # a plan whose blocks are all plain sets no flag, with or without the keyword; a one-block plan keeps its one-block bit
    plain = CellPlan(8, 8, 1, 'swish', _blocks([('M', 22, 3, 0), ('M', 30, 5, 8)]), mixed_kinds=True)
    assert plain.group_kinds is None and not plain.desc(2, 7, 9)[0].flags & _lib.CELL_KINDS
    one = CellPlan(8, 8, 1, 'swish', _blocks([('F', 22, 0)]), mixed_kinds=True)
    assert one.kind is _lib.FUSED and one.desc(2, 7, 9)[0].flags & _lib.CELL_FUSED and not one.desc(2, 7, 9)[0].flags & _lib.CELL_KINDS


def test_registry_and_primitives(lib):
    from tfnas_amd import _lib, model_search as ms, geometry as g
    assert ms.PRIMITIVES == g.PRIMITIVES and len(ms.PRIMITIVES) == 8
    new = ['FMB_k3_e3', 'FMB_k3_e6', 'FMB_k3_e3_se', 'FMB_k3_e6_se', 'DS_k3', 'DS_k5', 'DS_k3_se', 'DS_k5_se',
           'MBI_k7_e3', 'MBI_k7_e6', 'MBI_k7_e3_se', 'MBI_k7_e6_se']
    assert sorted(ms.OPS) == sorted(ms.PRIMITIVES + new)
    want = {'FMB_k3_e3': (_lib.FUSED, 3, 48, 0), 'FMB_k3_e6_se': (_lib.FUSED, 3, 48, 32), 'DS_k5': (_lib.NOEXPAND, 5, 16, 0),
            'DS_k3_se': (_lib.NOEXPAND, 3, 16, 16), 'MBI_k7_e3_se': (_lib.MBCONV, 7, 48, 16), 'MBI_k7_e6': (_lib.MBCONV, 7, 48, 0)}
    for name, (kind, k, mid, se) in want.items():
        b = ms.OPS[name](16, 48, 24, 2, False, 'swish')
        assert (b.kind, b.kernel_size, b.mid_channels, b.se_channels, b.stride, b.out_channels) == (kind, k, mid, se, 2, 24)
    mc = dict(enumerate([48, 96, 48, 96, 48, 96, 48, 96]))
    names = ['MBI_k3_e3', 'FMB_k3_e6', 'DS_k5', 'MBI_k7_e6', 'FMB_k3_e3_se', 'DS_k3_se', 'MBI_k5_e3_se', 'MBI_k5_e6_se']
    op = ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {}, primitives=names)
    assert op.num_ops == 8 and op.primitives == names and [b.kind.name[0] for b in op.m_ops] == list('MFNMFNMM')
    assert [b.name for b in op.m_ops][:3] == ['MBInvertedResBlock', 'FusedMBConvBlock', 'MBInvertedResBlock']
    assert op._plan(tuple(range(8))).group_kinds is not None and op._plan((1,)).kind is _lib.FUSED
    default = ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {})
    assert default.primitives == ms.PRIMITIVES and default._plan(tuple(range(8))).group_kinds is None
    assert list(default.state_dict()) == list(ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {}, primitives=None).state_dict())
    with pytest.raises(ValueError, match='FMB_k3_e3.*MBI_k3_e3'):
        ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {}, primitives=names[:7] + ['MBI_k9_e3'])
    with pytest.raises(ValueError):
        ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {}, primitives=names[:7])


def test_network_primitives_list_and_mapping_keep_the_state_dict_order(lib):
    from tfnas_amd import model_search as ms, geometry as g
    mcs = g.initial_mc_num_dddict()
    names = ['MBI_k3_e3', 'FMB_k3_e6', 'DS_k5', 'MBI_k7_e6', 'FMB_k3_e3_se', 'DS_k3_se', 'MBI_k5_e3_se', 'MBI_k5_e6_se']
    ref = ms.Network(10, mcs, {})
    assert ref.plain_candidates()
    every = ms.Network(10, mcs, {}, primitives=names)
    assert all(c.primitives == names for c in every.cells()) and not every.plain_candidates()
    some = ms.Network(10, mcs, {}, primitives={'stage2': {'block2': names}, 'stage6': {'block1': names}})
    hit = [(st, b) for st, b, *_ in g.iter_cells() if getattr(getattr(some, st), b).primitives == names]
    assert hit == [('stage2', 'block2'), ('stage6', 'block1')]
    assert all(getattr(getattr(some, st), b).primitives == ms.PRIMITIVES for st, b, *_ in g.iter_cells() if (st, b) not in hit)
    assert not some.plain_candidates()
    # arch parameters and stems / head keep their places; a cell's keys are its blocks' own, in candidate order
    def skeleton(model):
        return [k for k in model.state_dict() if '.m_ops.' not in k]
    assert skeleton(ref) == skeleton(every) == skeleton(some)
    keys = list(some.state_dict())
    plain_keys = list(ref.state_dict())
    untouched = [k for k in plain_keys if not k.startswith(('stage2.block2.m_ops', 'stage6.block1.m_ops'))]
    assert [k for k in keys if not k.startswith(('stage2.block2.m_ops', 'stage6.block1.m_ops'))] == untouched
    cell = [k for k in keys if k.startswith('stage2.block2.m_ops.')]
    assert [int(k.split('.')[3]) for k in cell] == sorted(int(k.split('.')[3]) for k in cell)
    assert 'stage2.block2.m_ops.1.fused_conv.conv.weight' in cell and 'stage2.block2.m_ops.2.inverted_bottleneck.conv.weight' not in cell
    st = ms.MixedStage([24, 40, 40], [40, 40, 40], [2, 1, 1], [False] * 3, ['swish'] * 3, mcs['stage2'], {}, 2,
                       primitives={'block3': names})
    assert [b.primitives == names for b in st.blocks()] == [False, False, True]
    with pytest.raises(ValueError):
        ms.Network(10, mcs, {}, primitives={'stage1': {'block1': ['nope'] * 8}})
    # a network with any non-plain candidate does not take the path level
    import torch
    assert every._use_paths(torch.zeros(1)) is False


def test_derived_config_round_trip_on_the_host(lib):
    from tfnas_amd import geometry as g, model_eval as me, parsing
    names = ['MBI_k3_e3', 'FMB_k3_e6', 'DS_k5', 'MBI_k7_e6', 'FMB_k3_e3_se', 'DS_k3_se', 'MBI_k5_e3_se', 'MBI_k5_e6_se']
    prim = {'stage2': {'block1': names, 'block2': names}, 'stage4': {'block1': names}, 'stage6': {'block1': names}}
    mcs = g.initial_mc_num_dddict()
    parsed = {'stage1': {'block1': 0}, 'stage2': {'block1': 1, 'block2': 2}, 'stage3': {'block1': 7}, 'stage4': {'block1': 3},
              'stage5': {'block1': 4}, 'stage6': {'block1': 5}}
    cfg = parsing.derived_config(parsed, mcs, 10, primitives=prim)
    got = [(b['name'], b['in_channels'], b['mid_channels'], b['se_channels'], b['kernel_size']) for st in sorted(parsed)
           for b in cfg[st]]
    assert got == [('MBInvertedResBlock', 16, 48, 0, 3),                      # default cell, op 0
                   ('FusedMBConvBlock', 24, 144, 0, 3), ('MBInvertedResBlock', 40, 40, 0, 5),      # FMB_k3_e6, DS_k5 (mid = in)
                   ('MBInvertedResBlock', 40, 240, 80, 5),                    # default cell, op 7
                   ('MBInvertedResBlock', 80, 480, 0, 7),                     # MBI_k7_e6
                   ('MBInvertedResBlock', 112, 336, 112, 3),                  # default cell, op 4
                   ('MBInvertedResBlock', 192, 192, 192, 3)]                  # DS_k3_se
    assert parsing.derived_config(parsed, mcs, 10) == parsing.derived_config(parsed, mcs, 10, primitives=None)
    net = me.NetworkCfg(10, cfg)
    twin = me.Network(10, parsed, mcs, primitives=prim)
    assert list(net.state_dict()) == list(twin.state_dict()) and net.config == cfg == twin.config
    assert [type(b).__name__ for b in net.stage2] == ['FusedMBConvBlock', 'MBInvertedResBlock']
    assert net.stage2[1].inverted_bottleneck is None and net.stage4[0].kernel_size == 7
    assert parsing.count_params_in_MB(cfg) > 0 and parsing.count_macs_in_M(cfg) > 0
    with pytest.raises(ValueError, match='unknown primitive'):
        parsing.derived_config(parsed, mcs, 10, primitives=['MBI_k9'] * 8)


def test_epoch_boundary_refuses_a_non_default_set_by_name(lib):
    from tfnas_amd import epoch, geometry as g, model_search as ms
    names = ['MBI_k3_e3', 'FMB_k3_e6'] + g.PRIMITIVES[2:]
    mcs = g.initial_mc_num_dddict()
    model = ms.Network(10, mcs, {}, primitives={'stage3': {'block2': names}})
    masks = g.make_mc_mask_dddict()
    for call in (lambda: epoch.slice_weights_from_max(model, {}, masks),
                 lambda: epoch.scatter_weights_to_max({}, model, masks),
                 lambda: epoch.remask_by_l1({}, mcs, masks, {}, primitives={'stage3': {'block2': names}}),
                 lambda: epoch.search_epoch(0, {}, masks, {}, [], None, primitives=names),
                 lambda: epoch.run_search('/nonexistent/never-made', {}, None, None, primitives=names)):
        with pytest.raises(NotImplementedError, match='FMB_k3_e6'):
            call()
    # the defaults, spelled out, are the defaults
    epoch.require_default_primitives('x', list(g.PRIMITIVES))
    epoch.require_default_primitives('x', None, ms.Network(10, mcs, {}))
    assert epoch.remask_by_l1({}, mcs, masks, {}, primitives=list(g.PRIMITIVES)) == []
