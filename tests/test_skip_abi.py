"""CPU-side checks of TFNAS_CELL_SKIP / TFNAS_GROUP_SKIP (include/tfnas_hip.h: the identity candidate of a residual cell), through
ctypes as tests/test_kinds_abi.py does: the two constants; every rule of the plan in both directions; what stays refused; the
workspace of a skip cell against the descriptor without its skip groups; the route queries.  Then the Python side: the name next to
the registry, MixedOP's three refusals and the stage / block in Network's message, geometry.residual_cells(), CellPlan's flags,
kinds and params(), the state_dict, the latency row and the epoch boundary's refusal."""
import ctypes as C
import os
import re

import pytest
import torch

import _kinds
import _skip
from _skip import M, N, F, S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL, ENULL, ERANGE = -1, -2, -3
GEO = dict(N=2, H=7, W=9, ic=8, oc=8)
ONE = C.c_void_p(16)


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _ws(lib, d):
    from tfnas_amd import _lib
    ws = _lib.TfnasCellWs()
    assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == 0
    return ws


def _fwd(lib, d, E=ONE):
    return lib.tfnas_mixedop_fwd(C.byref(d), ONE, ONE, E, ONE, ONE, ONE, ONE, ONE, ONE, None)


def _bwd(lib, d, E=ONE):
    return lib.tfnas_mixedop_bwd(C.byref(d), ONE, ONE, E, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, None, None, None)


def test_header_defines_the_two_constants_and_nothing_moved(lib):
    from tfnas_amd import _lib
    src = open(HEADER).read()
    m = re.search(r'#define TFNAS_CELL_SKIP (0x[0-9a-fA-F]+)', src)
    assert m and int(m.group(1), 16) == _lib.CELL_SKIP == 0x2000
    assert re.search(r'#define TFNAS_GROUP_SKIP 3\b', src) and _lib.GROUP_SKIP == 3
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src) and lib.tfnas_abi_version() == 4
    assert (int(lib.tfnas_sizeof(0)), int(lib.tfnas_sizeof(1)), int(lib.tfnas_sizeof(2))) == (144, C.sizeof(_lib.TfnasCellDesc), 224)
    assert [k.name for k in _lib.KINDS] == ['MBCONV', 'NOEXPAND', 'FUSED']           # a skip is not a BlockKind


@pytest.mark.parametrize('cands', [_skip.MNFS, _skip.EIGHT_S, _skip.EIGHT_SS, _skip.MSS, [M, S], [N, S], [F, S],
                                   [('M', 22, 3, 8), ('M', 30, 5, 0), S]], ids=lambda c: ''.join(x[0] for x in c))
def test_plan_accepts_trailing_skips_and_gives_them_nothing(lib, cands):
    from tfnas_amd import _lib
    d = _skip.skip_desc(cands, act=1, **GEO)
    d.flags |= _lib.CELL_K7
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    comp = _skip.computing(cands)
    e = _kinds.mixed_desc(comp, act=1, **GEO)
    e.flags |= _lib.CELL_K7
    assert lib.tfnas_cell_plan(C.byref(e)) == 0
    # M, SE and the computing groups' columns are those of the cell without its skips; a skip group has mcp = 0
    assert (d.M, d.SE, d.Ho, d.Wo) == (e.M, e.SE, e.Ho, e.Wo)
    for g in range(len(comp)):
        assert (d.g[g].mcp, d.g[g].off, d.g[g].se_off) == (e.g[g].mcp, e.g[g].off, e.g[g].se_off)
    for g in range(len(comp), len(cands)):
        assert d.g[g].mcp == 0 and d.g[g].kind == _lib.GROUP_SKIP
    # always a mixed cell: no E-free, no fused per-image route, the plain groups' E is needed
    assert lib.tfnas_efree_supported(C.byref(d)) == 0 and lib.tfnas_fx_supported(C.byref(d)) == 0
    assert lib.tfnas_cell_route(C.byref(d)) == _lib.ROUTE_TAKEN_VALID
    if any(c[0] == 'M' for c in comp):
        assert _fwd(lib, d, None) == ENULL and _bwd(lib, d, None) == ENULL
    # without the bit: kind 3 stays EINVAL under TFNAS_CELL_KINDS alone
    d.flags &= ~_lib.CELL_SKIP
    assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    # the bit without TFNAS_CELL_KINDS is EINVAL, whatever the groups say
    d.flags = _lib.CELL_SKIP | _lib.CELL_K7
    assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    p = _kinds.mixed_desc([M, ('M', 30, 5, 0)], flags=_lib.CELL_SKIP, **GEO)
    assert lib.tfnas_cell_plan(C.byref(p)) == EINVAL


@pytest.mark.parametrize('gp,nskip', [(1, 1), (1, 2), (3, 1), (3, 2), (7, 1)])
@pytest.mark.parametrize('need_w', (0, 1))
def test_workspace_equals_the_skipless_descriptors_field_by_field(lib, gp, nskip, need_w):
    from tfnas_amd import _lib
    for comp in (_kinds.EIGHT[:gp], [('M', 22 + 4 * i, 3 + 2 * (i % 2), 8 * (i % 2)) for i in range(gp)]):
        d = _skip.skip_desc(comp + [S] * nskip, act=1, **GEO)
        d.flags |= _lib.CELL_K7
        d.need_wgrad = need_w
        assert lib.tfnas_cell_plan(C.byref(d)) == 0
        e = _kinds.mixed_desc(comp, act=1, **GEO)            # flags & ~TFNAS_CELL_SKIP, G = G'
        e.flags |= _lib.CELL_K7
        e.need_wgrad = need_w
        assert lib.tfnas_cell_plan(C.byref(e)) == 0
        a, b = _skip.ws_fields(_ws(lib, d)), _skip.ws_fields(_ws(lib, e))
        assert a == b
        Po = 2 * 7 * 9
        assert a['Pr'] == gp * Po * 8 and a['stats'] == 4 * d.M + 2 * gp * 8 and a['off_resdot'] == 2 * gp * 8


def test_the_bit_without_a_skip_group_changes_nothing(lib):
    from tfnas_amd import _lib
    for cands in (_kinds.THREE, _kinds.EIGHT, [M, ('M', 30, 5, 8)], [F], [N]):
        a = _kinds.mixed_desc(cands, act=1, **GEO)
        a.flags |= _lib.CELL_K7
        b = _kinds.mixed_desc(cands, act=1, **GEO)
        b.flags |= _lib.CELL_K7 | _lib.CELL_SKIP
        assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
        b.flags &= ~_lib.CELL_SKIP
        assert bytes(a) == bytes(b)                          # the plan wrote the same words
        b.flags |= _lib.CELL_SKIP
        assert _skip.ws_fields(_ws(lib, a)) == _skip.ws_fields(_ws(lib, b))
        for fn in (lib.tfnas_cell_route, lib.tfnas_efree_supported, lib.tfnas_fx_supported):
            assert fn(C.byref(a)) == fn(C.byref(b))
    # the bit itself asks for a residual cell, skip group or not
    b = _kinds.mixed_desc(_kinds.THREE, 2, 7, 9, 8, 12, stride=2, act=1)
    assert lib.tfnas_cell_plan(C.byref(b)) == 0
    b.flags |= _lib.CELL_SKIP
    assert lib.tfnas_cell_plan(C.byref(b)) == EINVAL


def test_refusals(lib):
    from tfnas_amd import _lib
    KS = _lib.CELL_KINDS | _lib.CELL_SKIP
    ok = lambda cands=_skip.MNFS, **kw: _skip.skip_desc(cands, **dict(GEO, **kw))      # noqa: E731
    assert lib.tfnas_cell_plan(C.byref(ok())) == 0
    # a skip in a stride-2 cell, in a cell with ic != oc, in a cell that says it has no residual
    assert lib.tfnas_cell_plan(C.byref(ok(stride=2))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(ok(oc=12))) == EINVAL
    d = ok()
    d.has_res = 0
    assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    # a skip before a computing group; an all-skip cell
    for cands in ([M, S, N], [S, M], [M, S, F, S]):
        assert lib.tfnas_cell_plan(C.byref(ok(cands))) == EINVAL
    for n in (1, 2, 8):
        d = ok([M] + [S] * (n - 1)) if n > 1 else ok([M, S])
        d.g[0].mc, d.g[0].k, d.g[0].se, d.g[0].kind = 0, 0, 0, _lib.GROUP_SKIP
        if n == 1:
            d.G = 1
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    # a skip group with a width, a kernel size, an SE width or any pointer
    for field, val in (('mc', 8), ('k', 3), ('se', 4)):
        d = ok()
        setattr(d.g[3], field, val)
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    for field in _lib._W_FIELDS + _lib._G_FIELDS:
        d = ok()
        setattr(d.g[3], field, 256)
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL, field
    # either one-block bit beside it; an undefined bit
    for bit in (_lib.CELL_NOEXPAND, _lib.CELL_FUSED, 0x4000):
        assert lib.tfnas_cell_plan(C.byref(ok(flags=KS | bit))) == EINVAL
    # the other opt-in bits apply as before
    assert lib.tfnas_cell_plan(C.byref(ok(_skip.EIGHT_S, flags=KS))) == EINVAL               # k = 7 without its bit
    assert lib.tfnas_cell_plan(C.byref(ok(_skip.EIGHT_S, flags=KS | _lib.CELL_K7))) == 0
    assert lib.tfnas_cell_plan(C.byref(ok(act=2, flags=KS))) == EINVAL                       # relu6 without its bit
    assert lib.tfnas_cell_plan(C.byref(ok(act=2, flags=KS | _lib.CELL_ACTS))) == 0
    # stem and head mode refuse the bit
    stem = _kinds.mixed_desc([('M', 32, 3, 8)], 2, 0, 0, 27, 16, mode=_lib.MODE_STEM)
    stem.Hi = stem.Wi = 32
    for flags, want in ((KS, EINVAL), (_lib.CELL_SKIP, EINVAL), (0, 0)):
        stem.flags = flags
        assert lib.tfnas_cell_plan(C.byref(stem)) == want
    head = _kinds.mixed_desc([('M', 320, 3, 0)], 2, 7, 7, 320, 4, mode=_lib.MODE_HEAD)
    for flags, want in ((KS, EINVAL), (_lib.CELL_SKIP, EINVAL), (0, 0)):
        head.flags = flags
        assert lib.tfnas_cell_plan(C.byref(head)) == want
    head.flags = _lib.CELL_SKIP
    assert lib.tfnas_head_fwd(C.byref(head), ONE, ONE, ONE, ONE, ONE, None) == EINVAL
    # the entry points re-check a descriptor changed after its plan, before any pointer is looked at
    changes = [lambda d: setattr(d.g[3], 'mc', 8), lambda d: setattr(d.g[3], 'w_proj', 256), lambda d: setattr(d, 'has_res', 0),
               lambda d: setattr(d.g[2], 'kind', 3), lambda d: setattr(d, 'flags', d.flags & ~_lib.CELL_SKIP),
               lambda d: setattr(d, 'flags', d.flags & ~_lib.CELL_KINDS), lambda d: setattr(d, 'stride', 2)]
    for change in changes:
        for launch in (_fwd, _bwd):
            d = ok()
            assert lib.tfnas_cell_plan(C.byref(d)) == 0
            change(d)
            assert launch(lib, d) == EINVAL
    d = ok()
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d.g[1].kind, d.g[2].kind = 3, 3                                  # [M, S, S, S]-looking words with widths: a skip with mc != 0
    assert _fwd(lib, d) == EINVAL
    # the affine entry points refuse the bit
    bn = _lib.TfnasBnAffine()
    d = ok([M, S])
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    for G in (2, 1):
        d.G = G
        assert lib.tfnas_mbconv_fwd(C.byref(d), C.byref(bn), None, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None) == EINVAL
        assert lib.tfnas_mbconv_bwd(C.byref(d), C.byref(bn), None, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, ONE, ONE, ONE, ONE,
                                    ONE, None, None, None) == EINVAL


def _plain_desc(N, H, W, ic, oc, mids, ks, ses, skip):
    cands = [('M', m, k, se) for m, k, se in zip(mids, ks, ses)] + ([S] if skip else [])
    if skip:
        return _skip.skip_desc(cands, N, H, W, ic, oc, act=1)
    return _kinds.mixed_desc(cands, N, H, W, ic, oc, act=1, flags=0)


def test_route_queries_give_up_the_fused_and_e_free_routes_with_a_skip(lib):
    from tfnas_amd import _lib
    # frozen weights; the 14 x 14, ic = oc = 80, N = 8 cell of tests/test_act_abi.py and a 56 x 56, ic = oc = 24, N = 2 cell
    late = dict(N=8, H=14, W=14, ic=80, oc=80, mids=(240, 480), ks=(3, 3), ses=(0, 80))
    early = dict(N=2, H=56, W=56, ic=24, oc=24, mids=(72, 144), ks=(3, 5), ses=(0, 24))
    for geo, fx, efree in ((late, 1, 1), (early, 0, 1)):
        a, b = _plain_desc(skip=False, **geo), _plain_desc(skip=True, **geo)
        assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
        assert lib.tfnas_fx_supported(C.byref(a)) == fx and lib.tfnas_efree_supported(C.byref(a)) == efree
        assert lib.tfnas_cell_route(C.byref(a)) == _lib.ROUTE_TAKEN_VALID | (_lib.ROUTE_TAKEN_FX if fx else 0)
        assert lib.tfnas_fx_supported(C.byref(b)) == 0 and lib.tfnas_efree_supported(C.byref(b)) == 0
        assert lib.tfnas_cell_route(C.byref(b)) == _lib.ROUTE_TAKEN_VALID
        assert _fwd(lib, b, None) == ENULL                       # E == NULL: the plain groups of a skip cell materialise E
        # ... and the workspace is the plain cell's own
        assert _skip.ws_fields(_ws(lib, a)) == _skip.ws_fields(_ws(lib, b))


@pytest.mark.gpu          # (tfnas_path_create makes streams and events: it needs a device; nothing is launched)
def test_path_level_refuses_the_bit(lib):
    from tfnas_amd import _lib
    ctx = C.c_void_p(None)
    assert lib.tfnas_path_create(C.byref(ctx)) == 0
    try:
        beta = C.c_void_p(256)
        plain = [('M', 22 + 4 * i, 3, 0) for i in range(7)]
        for src, want in ((_kinds.mixed_desc(plain + [('M', 50, 3, 0)], 2, 9, 13, 16, 16, flags=0), 0),
                          (_skip.skip_desc(plain + [S], 2, 9, 13, 16, 16), EINVAL)):
            pd = _lib.TfnasPathDesc()
            pd.ncell, pd.nstage, pd.soft, pd.need_dx0 = 1, 1, 1, 1
            pd.stage[0].ncell, pd.stage[0].start_res, pd.stage[0].betas = 1, 0, beta
            C.memmove(C.byref(pd.cell[0]), C.byref(src), C.sizeof(src))
            ws = _lib.TfnasPathWs()
            assert lib.tfnas_path_plan(ctx, C.byref(pd), C.byref(ws)) == want
    finally:
        lib.tfnas_path_destroy(ctx)


# ------------------------------------------------------------------------------------------------ Python side (host only)
def _blocks(cands, ic=8, oc=8, stride=1, act='swish'):
    from tfnas_amd.layers import FusedMBConvBlock, IdentityLayer, MBInvertedResBlock
    out = []
    for c in cands:
        if c[0] == 'M':
            out.append(MBInvertedResBlock(ic, c[1], c[3], oc, c[2], stride, act_func=act))
        elif c[0] == 'N':
            out.append(MBInvertedResBlock(ic, ic, c[2], oc, c[1], stride, act_func=act))
        elif c[0] == 'F':
            out.append(FusedMBConvBlock(ic, c[1], c[2], oc, 3, stride, act_func=act))
        else:
            out.append(IdentityLayer(ic, oc))
    return out


def test_identity_layer_is_the_references():
    from tfnas_amd.layers import IdentityLayer
    m = IdentityLayer(24, 24)
    x = torch.randn(2, 24, 5, 5)
    assert m(x) is x and not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    assert m.name == 'IdentityLayer' and (m.in_channels, m.out_channels) == (24, 24)
    assert m.config == {'name': 'IdentityLayer', 'in_channels': 24, 'out_channels': 24, 'use_bn': False, 'affine': False,
                        'act_func': None, 'ops_order': 'weight_bn_act'}
    assert list(m.config) == ['name', 'in_channels', 'out_channels', 'use_bn', 'affine', 'act_func', 'ops_order']
    assert m.hip_params() == [] and m.set_se_style(('relu', 'h-sigmoid')) is None


def test_cellplan_flags_kinds_and_params(lib):
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan
    blocks = _blocks(_skip.EIGHT_SS)
    for kw in (dict(), dict(mixed_kinds=False)):                 # without the keyword: refused like any non-plain block
        with pytest.raises(NotImplementedError):
            CellPlan(8, 8, 1, 'swish', blocks, **kw)
        with pytest.raises(NotImplementedError):
            CellPlan(8, 8, 1, 'swish', _blocks([M, S]), **kw)
    plan = CellPlan(8, 8, 1, 'swish', blocks, mixed_kinds=True)
    d, ws = plan.desc(2, 7, 9)
    assert d.flags & _lib.CELL_KINDS and d.flags & _lib.CELL_SKIP and d.G == 8
    assert [d.g[g].kind for g in range(8)] == [0, 2, 1, 0, 2, 1, 3, 3]
    assert [(d.g[g].mc, d.g[g].k, d.g[g].se, d.g[g].mcp) for g in (6, 7)] == [(0, 0, 0, 0)] * 2
    want = [p for b in blocks[:6] for p in b.hip_params()]
    assert len(plan.params()) == len(want) and all(a is b for a, b in zip(plan.params(), want))
    plan.bind(d, plan.params(), plan.params())                   # (pointers only: nothing is launched)
    for g in (6, 7):
        assert all(getattr(d.g[g], f) is None for f in _lib._W_FIELDS + _lib._G_FIELDS)
    assert lib.tfnas_cell_route(C.byref(d)) == _lib.ROUTE_TAKEN_VALID
    # all-plain computing blocks, and one alone, still make a KINDS | SKIP descriptor
    for cands in ([('M', 22, 3, 0), ('M', 30, 5, 8), S], [M, S], [M, S, S]):
        p = CellPlan(8, 8, 1, 'swish', _blocks(cands), mixed_kinds=True)
        dd = p.desc(2, 7, 9)[0]
        assert dd.flags & _lib.CELL_KINDS and dd.flags & _lib.CELL_SKIP and not dd.flags & (_lib.CELL_FUSED | _lib.CELL_NOEXPAND)
        assert p.kind is _lib.MBCONV
    # all identity; a skip before a computing block; a non-residual cell
    with pytest.raises(ValueError):
        CellPlan(8, 8, 1, 'swish', _blocks([S, S]), mixed_kinds=True)
    with pytest.raises(ValueError):
        CellPlan(8, 8, 1, 'swish', _blocks([S]), mixed_kinds=True)
    with pytest.raises(ValueError):
        CellPlan(8, 8, 1, 'swish', _blocks([M, S, N]), mixed_kinds=True)
    with pytest.raises(ValueError):
        CellPlan(8, 12, 1, 'swish', _blocks([M, S], oc=12), mixed_kinds=True)
    with pytest.raises(ValueError):
        CellPlan(8, 8, 2, 'swish', _blocks([M, S], stride=2), mixed_kinds=True)


def _mc(ic):
    return dict(enumerate([3 * ic, 6 * ic] * 4))


def test_registry_name_and_the_three_refusals_of_mixedop(lib):
    from tfnas_amd import model_search as ms, geometry as g
    from tfnas_amd.layers import IdentityLayer
    assert ms.SKIP == g.SKIP == 'skip' and ms.SKIP not in ms.OPS and ms.SKIP not in g.PRIMITIVE_SPECS
    new = ['FMB_k3_e3', 'FMB_k3_e6', 'FMB_k3_e3_se', 'FMB_k3_e6_se', 'DS_k3', 'DS_k5', 'DS_k3_se', 'DS_k5_se',
           'MBI_k7_e3', 'MBI_k7_e6', 'MBI_k7_e3_se', 'MBI_k7_e6_se']
    assert sorted(ms.OPS) == sorted(ms.PRIMITIVES + new)
    names = ms.PRIMITIVES[:7] + ['skip']
    assert ms.check_primitives(names) == names
    with pytest.raises(ValueError, match='unknown primitive'):
        ms.check_primitives(ms.PRIMITIVES[:7] + ['skipp'])
    op = ms.MixedOP(16, 16, 1, False, 'swish', 8, _mc(16), _skip.SkipLut(), primitives=names)
    assert isinstance(op.m_ops[7], IdentityLayer) and not any(k.startswith('m_ops.7.') for k in op.state_dict())
    assert any(k.startswith('m_ops.6.') for k in op.state_dict()) and op.log_alphas.shape == (8,)
    lats = op.get_lookup_latency(14)
    assert len(lats) == 8 and lats[-1] == 0 and all(v > 0 for v in lats[:7])
    # the widths are ignored for the skip: a table without entry 7 works
    mc7 = {i: v for i, v in _mc(16).items() if i != 7}
    ms.MixedOP(16, 16, 1, False, 'swish', 8, mc7, {}, primitives=names)
    for kw, why in ((dict(stride=2), 'residual'), (dict(oc=24), 'residual')):
        with pytest.raises(ValueError, match=why):
            ms.MixedOP(16, kw.get('oc', 16), kw.get('stride', 1), False, 'swish', 8, _mc(16), {}, primitives=names)
    with pytest.raises(ValueError, match='after every other'):
        ms.MixedOP(16, 16, 1, False, 'swish', 8, _mc(16), {}, primitives=['skip'] + ms.PRIMITIVES[:7])
    with pytest.raises(ValueError, match='at least one'):
        ms.MixedOP(16, 16, 1, False, 'swish', 8, _mc(16), {}, primitives=['skip'] * 8)
    # the sampled forward of a skip is the input tensor itself, without a launch (CPU tensors never reach the library)
    x = torch.randn(2, 16, 5, 5)
    op._pre = 7
    y, lat = op(x, True, 'random')
    assert y is x and lat == 0 and op.last_idx == 7


def test_residual_cells_and_networks_message(lib):
    from tfnas_amd import model_search as ms, geometry as g
    res = list(g.residual_cells())
    assert res == [(st, b) for st, b, ic, oc, s, act, size in g.iter_cells() if ic == oc and s == 1]
    assert len(res) == 12 and ('stage1', 'block1') not in res and ('stage4', 'block1') not in res and ('stage6', 'block1') not in res
    names = ms.PRIMITIVES[:7] + ['skip']
    mc = g.initial_mc_num_dddict()
    with pytest.raises(ValueError, match=r'stage1 block1.*\{stage: \{block: list\}\}'):      # one list for every cell cannot work
        ms.Network(10, mc, _skip.SkipLut(), primitives=names)
    with pytest.raises(ValueError, match='stage3 block1'):
        ms.Network(10, mc, _skip.SkipLut(), primitives={'stage3': {'block1': names}})
    prim = {}
    for st, b in g.residual_cells():
        prim.setdefault(st, {})[b] = names
    net = ms.Network(10, mc, _skip.SkipLut(), primitives=prim)
    assert net.plain_candidates() is False
    kinds = [c.m_ops[7].name for c in net.cells()]
    assert kinds.count('IdentityLayer') == 12
    assert not any('.m_ops.7.' in k for k in net.stage3.block2.state_dict(prefix='stage3.block2.'))
    assert any(k.startswith('stage3.block1.m_ops.7.') for k in net.state_dict())


def test_epoch_boundary_names_the_skip(lib):
    from tfnas_amd import epoch, model_search as ms, geometry as g
    mc = g.initial_mc_num_dddict()
    net = ms.Network(10, mc, _skip.SkipLut(), primitives={'stage2': {'block2': ms.PRIMITIVES[:7] + ['skip']}})
    with pytest.raises(NotImplementedError, match=r"stage2\.block2 holds 'skip' as candidate 7"):
        epoch.require_default_primitives('slice_weights_from_max', model=net)
    with pytest.raises(NotImplementedError, match="'skip'"):
        epoch.require_default_primitives('slice_weights_from_max', primitives=ms.PRIMITIVES[:7] + ['skip'])
