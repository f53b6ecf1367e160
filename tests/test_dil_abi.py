"""CPU-side checks of dilated depthwise groups in the C ABI (include/tfnas_hip.h: TfnasGroup.dil, read only from a descriptor
that carries TFNAS_CELL_DILATION), through ctypes as tests/test_k7_abi.py does, and of the Python layers above it: the plan
accepts (k, dil) = (3, 2) and (5, 2) at both strides from a caller that set the bit; without the bit the word is not read and
nothing changes; with the bit an undilated descriptor plans, sizes and routes identically (the 18 cells at B = 128); every refusal
of the header; a dilated cell takes the materialised route where its undilated twin is E-free or fused; the entry points re-check
a descriptor changed after its plan; HipModes.apply sets the bit for dilated descriptors only; the registry, the config export
and NetworkCfg, the latency key and the epoch boundary."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _desc(N=2, H=9, W=11, ic=24, oc=24, stride=1, mids=(32, 53), ks=(3, 5), dils=(2, 2), ses=(0, 24), need_wgrad=0, act=1,
          flags=None, mode=0, kinds=None):
    from tfnas_amd import _lib
    d = _lib.TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, H, W, ic, oc, stride, act, len(mids), mode
    d.has_res = int(mode == 0 and ic == oc and stride == 1)
    d.eps = 1e-5
    d.need_wgrad = need_wgrad
    for g, (m, k, dl, s) in enumerate(zip(mids, ks, dils, ses)):
        d.g[g].mc, d.g[g].k, d.g[g].dil, d.g[g].se = m, k, dl, s
        if kinds is not None:
            d.g[g].kind = kinds[g]
    d.flags = (_lib.CELL_DILATION | (_lib.CELL_K7 if 7 in ks else 0) | _lib.act_flags(act)) if flags is None else flags
    return d


def _ws(lib, d):
    from tfnas_amd import _lib
    ws = _lib.TfnasCellWs()
    assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == 0
    return {f: getattr(ws, f) for f, _ in ws._fields_}


def _planned(d):
    return ((d.M, d.SE, d.Ho, d.Wo), [(d.g[g].off, d.g[g].mcp, d.g[g].se_off) for g in range(d.G)])


def _queries(lib, d):
    return tuple(fn(C.byref(d)) for fn in (lib.tfnas_cell_route, lib.tfnas_efree_supported, lib.tfnas_fx_supported))


def test_header_and_mirror_agree_and_the_abi_version_stays(lib):
    from tfnas_amd import _lib
    src = open(HEADER).read()
    m = re.search(r'#define TFNAS_CELL_DILATION (0x[0-9a-fA-F]+)', src)
    assert m and int(m.group(1), 16) == _lib.CELL_DILATION == 0x8000
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src) and lib.tfnas_abi_version() == 4
    assert not re.search(r'#define TFNAS_\w+ 0x4000\b', src)                              # (stays undefined)
    assert re.search(r'int32_t k;\s*/\* depthwise kernel size: 3 or 5; 7 with TFNAS_CELL_K7', src)
    # the field took the padding word: same position, same struct sizes
    body = re.search(r'typedef struct TfnasGroup \{(.*?)\} TfnasGroup;', src, re.S).group(1)
    words = re.findall(r'int32_t (\w+);', body)
    assert words == [n for n, t in _lib.TfnasGroup._fields_ if t is C.c_int32] and words[-1] == 'dil' and 'pad1' not in words
    assert lib.tfnas_sizeof(0) == C.sizeof(_lib.TfnasGroup) == 8 * 4 + 14 * 8
    assert lib.tfnas_sizeof(1) == C.sizeof(_lib.TfnasCellDesc)
    assert 'TFNAS_CELL_DILATION' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


@pytest.mark.parametrize('stride', [1, 2])
def test_plan_accepts_both_pairs_with_the_bit(lib, stride):
    for ks, dils in (((3, 5), (2, 2)), ((5, 3), (2, 1)), ((3, 3), (1, 2)), ((7, 5), (0, 2))):
        d = _desc(ks=ks, dils=dils, stride=stride, oc=24 if stride == 1 else 40)
        assert lib.tfnas_cell_plan(C.byref(d)) == 0, (ks, dils)
        assert (d.Ho, d.Wo) == ((9 - 1) // stride + 1, (11 - 1) // stride + 1)           # padding dil * (k / 2): the size of every k
    for act in (0, 1, 2, 3):                                                               # all four activations
        assert lib.tfnas_cell_plan(C.byref(_desc(act=act, stride=stride, oc=24 if stride == 1 else 40, need_wgrad=1))) == 0


def test_without_the_bit_the_word_is_not_read(lib):
    """a non-zero dil -- legal or not -- in a descriptor without the bit changes nothing: planned words, workspace, route"""
    from tfnas_amd import _lib
    geo = dict(N=128, H=14, W=14, ic=112, oc=112, mids=(336, 672, 336), ks=(3, 5, 5), ses=(0, 0, 112))
    base = _desc(dils=(0, 0, 0), flags=0, **geo)
    assert lib.tfnas_cell_plan(C.byref(base)) == 0
    for dils in ((2, 2, 2), (1, 0, 2), (7, -3, 1 << 30)):
        d = _desc(dils=dils, flags=0, **geo)
        assert lib.tfnas_cell_plan(C.byref(d)) == 0, dils
        assert _planned(d) == _planned(base) and _ws(lib, d) == _ws(lib, base) and _queries(lib, d) == _queries(lib, base)
    assert lib.tfnas_fx_supported(C.byref(base)) == 1
    # ... and the descriptor is refused exactly as before where it was: k = 7 without TFNAS_CELL_K7, bit 0x4000
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3, 7), dils=(2, 2), flags=0))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(0, 0), flags=0x4000))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(0, 0), flags=0x4000 | _lib.CELL_DILATION))) == EINVAL


def test_with_the_bit_an_undilated_descriptor_is_what_it_was_on_the_18_cells(lib):
    """the 18 cells of the search space at B = 128, all eight candidates, frozen weights and with weight gradients: planned words,
    tfnas_cell_ws field by field, tfnas_cell_route, tfnas_efree_supported, tfnas_fx_supported"""
    from tfnas_amd import _lib, geometry as g
    n = 0
    for stage, block, ic, oc, stride, act, size in g.iter_cells():
        for need_wgrad in (0, 1):
            geo = dict(N=128, H=size, W=size, ic=ic, oc=oc, stride=stride, mids=(3 * ic, 6 * ic) * 4, ks=(3, 3, 5, 5) * 2,
                       ses=(0,) * 4 + (ic, 2 * ic) * 2, act=_lib.ACT[act], need_wgrad=need_wgrad)
            a = _desc(dils=(0,) * 8, flags=0, **geo)
            for dils in ((0,) * 8, (1,) * 8, (0, 1) * 4):
                b = _desc(dils=dils, **geo)
                assert b.flags == _lib.CELL_DILATION
                assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
                assert _planned(a) == _planned(b), (stage, block)
                assert _ws(lib, a) == _ws(lib, b), (stage, block)
                assert _queries(lib, a) == _queries(lib, b), (stage, block)
            n += 1
    assert n == 36


def test_dilation_changes_neither_planned_words_nor_workspace(lib):
    for stride in (1, 2):
        for need_wgrad in (0, 1):
            geo = dict(N=4, H=14, W=14, ic=40, oc=40 if stride == 1 else 80, stride=stride, mids=(120, 240, 131),
                       ks=(3, 5, 5), ses=(0, 40, 80), need_wgrad=need_wgrad)
            dd, du = _desc(dils=(2, 2, 1), **geo), _desc(dils=(0, 0, 0), **geo)
            assert lib.tfnas_cell_plan(C.byref(dd)) == 0 and lib.tfnas_cell_plan(C.byref(du)) == 0
            assert _planned(dd) == _planned(du) and _ws(lib, dd) == _ws(lib, du)


def test_refusals(lib):
    from tfnas_amd import _lib
    ok = _desc()
    assert lib.tfnas_cell_plan(C.byref(ok)) == 0
    for bad in (3, 4, -1, 1 << 20):                                                        # dil outside {0, 1, 2}
        assert lib.tfnas_cell_plan(C.byref(_desc(dils=(bad, 1)))) == EINVAL
        assert lib.tfnas_cell_plan(C.byref(_desc(dils=(2, bad)))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3, 7), dils=(1, 2)))) == EINVAL          # k == 7 with dil == 2
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3, 7), dils=(2, 1)))) == 0
    K = _lib.CELL_KINDS | _lib.CELL_DILATION
    M, N_, F_, S = 0, 1, 2, _lib.GROUP_SKIP
    kinds_geo = dict(ic=24, oc=24, mids=(32, 24, 40), ks=(3, 5, 3), ses=(0, 0, 0))
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(2, 2, 0), flags=K, kinds=(M, N_, F_), **kinds_geo))) == 0
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(0, 0, 2), flags=K, kinds=(M, N_, F_), **kinds_geo))) == EINVAL   # a dilated FUSED group
    skip_geo = dict(ic=24, oc=24, mids=(32, 0), ks=(3, 0), ses=(0, 0))
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(2, 0), flags=K | _lib.CELL_SKIP, kinds=(M, S), **skip_geo))) == 0
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(2, 2), flags=K | _lib.CELL_SKIP, kinds=(M, S), **skip_geo))) == EINVAL   # a dilated SKIP group
    one = dict(ic=24, oc=24, mids=(40,), ks=(3,), ses=(0,))
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(0,), flags=_lib.CELL_FUSED | _lib.CELL_DILATION, **one))) == 0
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(2,), flags=_lib.CELL_FUSED | _lib.CELL_DILATION, **one))) == EINVAL      # a dilated FUSED cell
    noexp = dict(ic=24, oc=24, mids=(24,), ks=(5,), ses=(24,))
    assert lib.tfnas_cell_plan(C.byref(_desc(dils=(2,), flags=_lib.CELL_NOEXPAND | _lib.CELL_DILATION, **noexp))) == 0      # expand-free: allowed
    stem = dict(ic=27, oc=16, mids=(32,), ks=(3,), ses=(8,), act=0, mode=_lib.MODE_STEM)
    for dil, want in ((0, 0), (2, EINVAL)):                                                # stem and head mode
        d = _desc(dils=(dil,), **stem)
        d.Hi, d.Wi = 18, 26
        assert lib.tfnas_cell_plan(C.byref(d)) == want
        h = _desc(ic=320, oc=320, mids=(1280,), ks=(3,), ses=(0,), dils=(dil,), mode=_lib.MODE_HEAD)
        assert lib.tfnas_cell_plan(C.byref(h)) == want


def test_dilated_cells_take_the_materialised_route(lib):
    from tfnas_amd import _lib
    # the geometries where the undilated cell is E-free / fused (frozen weights): stride-2 ic 16 at 112 x 112, ic 112 at 14 x 14
    for geo in (dict(N=8, H=112, W=112, ic=16, oc=24, stride=2, mids=(48, 96), ses=(0, 16)),
                dict(N=8, H=14, W=14, ic=112, oc=112, stride=1, mids=(336, 672), ses=(0, 0))):
        du = _desc(ks=(3, 5), dils=(1, 0), **geo)
        assert lib.tfnas_cell_plan(C.byref(du)) == 0 and lib.tfnas_efree_supported(C.byref(du)) == 1
        for ks, dils in (((3, 5), (2, 0)), ((3, 5), (0, 2)), ((5, 5), (2, 2))):
            dd = _desc(ks=ks, dils=dils, **geo)
            assert lib.tfnas_cell_plan(C.byref(dd)) == 0
            assert _queries(lib, dd) == (_lib.ROUTE_TAKEN_VALID, 0, 0), (ks, dils)
            for route in (_lib.ROUTE_DW['direct'], _lib.ROUTE_DW['lds'], _lib.ROUTE_DW['tiled'], _lib.ROUTE_DWWG_OFF):
                dd.route = route
                assert _queries(lib, dd) == (_lib.ROUTE_TAKEN_VALID, 0, 0)


def test_entry_points_recheck_a_descriptor_changed_after_its_plan(lib):
    """every entry point runs the checks of the plan again, before any pointer is looked at: a planned descriptor whose dilation
    words were made illegal afterwards is refused.  A descriptor whose BIT was dropped after the plan is, by the rule that dil is
    not read without it, the undilated descriptor: it answers every query as its undilated twin does (nothing of a dilated
    plan survives in the planned words, so there is nothing left to refuse it by)."""
    from tfnas_amd import _lib
    one = C.c_void_p(16)

    def fwd(d):
        return lib.tfnas_mixedop_fwd(C.byref(d), one, None, one, one, one, one, one, one, one, None)

    def bwd(d):
        return lib.tfnas_mixedop_bwd(C.byref(d), one, None, one, one, one, one, one, one, one, one, one, one, one, one, one, None, None)
    bn = _lib.TfnasBnAffine()

    def afwd(d):
        return lib.tfnas_mbconv_fwd(C.byref(d), C.byref(bn), None, one, one, one, one, one, one, one, one, None)

    def abwd(d):
        return lib.tfnas_mbconv_bwd(C.byref(d), C.byref(bn), None, one, one, one, one, one, one, one, one, one, one, one, one,
                                    one, one, one, None)
    for entry in (fwd, bwd, afwd, abwd):
        for change in ('dil3', 'k7', 'fused', 'stem'):
            d = _desc(mids=(53,), ks=(5,), dils=(2,), ses=(24,))
            assert lib.tfnas_cell_plan(C.byref(d)) == 0
            if change == 'dil3':
                d.g[0].dil = 3
            elif change == 'k7':
                d.g[0].k, d.flags = 7, d.flags | _lib.CELL_K7
            elif change == 'fused':
                d.flags |= _lib.CELL_FUSED
            else:
                d.mode = _lib.MODE_STEM
            assert entry(d) == EINVAL, (entry.__name__, change)
    d, u = _desc(N=8, H=14, W=14, ic=112, oc=112, mids=(336,), ks=(5,), dils=(2,), ses=(0,)), None
    assert lib.tfnas_cell_plan(C.byref(d)) == 0 and lib.tfnas_fx_supported(C.byref(d)) == 0
    d.flags &= ~_lib.CELL_DILATION
    u = _desc(N=8, H=14, W=14, ic=112, oc=112, mids=(336,), ks=(5,), dils=(0,), ses=(0,), flags=0)
    assert lib.tfnas_cell_plan(C.byref(u)) == 0
    assert _queries(lib, d) == _queries(lib, u) and _planned(d) == _planned(u) and lib.tfnas_fx_supported(C.byref(d)) == 1


def test_python_mirror_sets_the_bit_for_dilated_descriptors_only():
    from tfnas_amd import _lib, functions as F
    for dils, want in (((0, 0), 0), ((1, 1), 0), ((0, 2), _lib.CELL_DILATION), ((2, 2), _lib.CELL_DILATION)):
        d = _desc(dils=dils, flags=0)
        F.HipModes().apply(d)
        assert d.flags == want, dils
        F.HipModes(lazy_join=True).apply(d)
        assert d.flags == want | _lib.CELL_LAZY_JOIN
    d = _desc(ks=(7, 3), dils=(0, 2), flags=0, act=3)
    F.HipModes().apply(d)
    assert d.flags == _lib.CELL_K7 | _lib.CELL_ACTS | _lib.CELL_DILATION
    assert _lib.describe_block(_lib.MBCONV, 2, 9, 9, 16, 48, 0, 16, 3, 1, 0).flags == 0
    db = _lib.describe_block(_lib.NOEXPAND, 2, 9, 9, 16, 16, 0, 16, 5, 1, 0, 2)
    assert db.flags == _lib.CELL_NOEXPAND | _lib.CELL_DILATION and db.g[0].dil == 2


def test_cell_plan_writes_the_word_and_keeps_it_zero_for_undilated_groups(lib):
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan
    from tfnas_amd.layers import MBInvertedResBlock
    blocks = [MBInvertedResBlock(16, 40, 8, 24, 3, 2, dilation=2), MBInvertedResBlock(16, 52, 0, 24, 5, 2),
              MBInvertedResBlock(16, 44, 0, 24, 5, 2, dilation=2)]
    d, _ = CellPlan(16, 24, 2, 'relu', blocks).desc(2, 9, 13)
    assert [d.g[g].dil for g in range(3)] == [2, 0, 2] and d.flags & _lib.CELL_DILATION
    d, _ = CellPlan(16, 24, 2, 'relu', blocks[1:2]).desc(2, 9, 13)
    assert d.g[0].dil == 0 and not d.flags & _lib.CELL_DILATION
    d, _ = CellPlan(16, 16, 1, 'swish', [MBInvertedResBlock(16, 16, 16, 16, 5, 1, dilation=2)]).desc(2, 9, 13)
    assert d.flags & _lib.CELL_NOEXPAND and d.flags & _lib.CELL_DILATION and d.g[0].dil == 2


def test_block_argument():
    import torch
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock
    plain, dil = MBInvertedResBlock(16, 48, 8, 24, 5, 2, affine=True), MBInvertedResBlock(16, 48, 8, 24, 5, 2, affine=True, dilation=2)
    assert plain.dilation == 1 and dil.dilation == 2
    c = dil.depth_conv.conv
    assert (tuple(c.weight.shape), c.padding, c.dilation, c.stride, c.groups, c.bias) == ((48, 1, 5, 5), (4, 4), (2, 2), (2, 2), 48, None)
    assert plain.depth_conv.conv.padding == (2, 2) and plain.depth_conv.conv.dilation == (1, 1)
    assert list(plain.state_dict()) == list(dil.state_dict())
    assert [tuple(v.shape) for v in plain.state_dict().values()] == [tuple(v.shape) for v in dil.state_dict().values()]
    assert [type(m) for m in plain.modules()] == [type(m) for m in dil.modules()]
    y = c(torch.zeros(1, 48, 9, 13))
    assert tuple(y.shape[2:]) == (5, 7)                                                    # (H - 1) / stride + 1
    for bad in (0, 3, 4, True, 2.0, None):
        with pytest.raises(ValueError):
            MBInvertedResBlock(16, 48, 8, 24, 3, 1, dilation=bad)
    with pytest.raises(ValueError, match='7'):
        MBInvertedResBlock(16, 48, 8, 24, 7, 1, dilation=2)
    with pytest.raises(TypeError):
        MBInvertedResBlock(16, 48, 8, 24, 3, 1, False, 'relu', None, 'sigmoid', 2)         # keyword-only
    with pytest.raises(TypeError):
        FusedMBConvBlock(16, 48, 8, 24, 3, 1, dilation=2)


def test_registry_and_primitives(lib):
    from tfnas_amd import _lib, model_search as ms, geometry as g
    new = ['MBI_k3d2_e3', 'MBI_k3d2_e6', 'MBI_k5d2_e3', 'MBI_k5d2_e6', 'MBI_k3d2_e3_se', 'MBI_k3d2_e6_se', 'MBI_k5d2_e3_se',
           'MBI_k5d2_e6_se', 'DS_k3d2', 'DS_k5d2', 'DS_k3d2_se', 'DS_k5d2_se']
    assert sorted(ms.DILATED_OPS) == sorted(new) == sorted(g.PRIMITIVE_DILATION) and not set(new) & set(ms.OPS)
    old = ['FMB_k3_e3', 'FMB_k3_e6', 'FMB_k3_e3_se', 'FMB_k3_e6_se', 'DS_k3', 'DS_k5', 'DS_k3_se', 'DS_k5_se',
           'MBI_k7_e3', 'MBI_k7_e6', 'MBI_k7_e3_se', 'MBI_k7_e6_se']
    assert sorted(ms.OPS) == sorted(ms.PRIMITIVES + old)                                   # OPS is what it was
    want = {'MBI_k3d2_e3': (_lib.MBCONV, 3, 48, 0), 'MBI_k3d2_e6_se': (_lib.MBCONV, 3, 48, 32), 'MBI_k5d2_e3_se': (_lib.MBCONV, 5, 48, 16),
            'MBI_k5d2_e6': (_lib.MBCONV, 5, 48, 0), 'DS_k3d2': (_lib.NOEXPAND, 3, 16, 0), 'DS_k5d2_se': (_lib.NOEXPAND, 5, 16, 16)}
    for name, (kind, k, mid, se) in want.items():
        b = ms.DILATED_OPS[name](16, 48, 24, 2, False, 'swish')
        assert (b.kind, b.kernel_size, b.mid_channels, b.se_channels, b.stride, b.out_channels, b.dilation) == (kind, k, mid, se, 2, 24, 2)
        layer, mc, se_, k_ = g.primitive_block(name, 16, 48)                                # still four words
        assert (layer, mc, se_, k_) == ('MBInvertedResBlock', mid, se, k) and g.primitive_dilation(name) == 2
    for name in list(ms.OPS) + [g.SKIP]:
        assert g.primitive_dilation(name) == 1
    with pytest.raises(ValueError):
        g.primitive_dilation('MBI_k3d3_e3')
    mc = dict(enumerate([48, 96, 48, 96, 48, 96, 48, 96]))
    names = ['MBI_k3_e3', 'MBI_k3d2_e6', 'MBI_k5d2_e3', 'MBI_k5_e6', 'MBI_k3d2_e3_se', 'MBI_k3_e6_se', 'MBI_k5_e3_se', 'MBI_k5d2_e6_se']
    assert ms.check_primitives(names) == names
    op = ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {}, primitives=names)
    assert [b.dilation for b in op.m_ops] == [1, 2, 2, 1, 2, 1, 1, 2] and all(b.kind is _lib.MBCONV for b in op.m_ops)
    d, _ = op._plan(tuple(range(8))).desc(2, 9, 13)
    assert [d.g[i].dil for i in range(8)] == [0, 2, 2, 0, 2, 0, 0, 2] and d.flags == _lib.CELL_DILATION
    default = ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {})
    assert list(default.state_dict()) == list(op.state_dict())
    assert default._plan(tuple(range(8))).desc(2, 9, 13)[0].flags == 0
    ds = ms.MixedOP(16, 16, 1, False, 'swish', 8, mc, {}, primitives=names[:7] + ['DS_k3d2'])
    assert ds.m_ops[7].kind is _lib.NOEXPAND and ds._plan(tuple(range(8))).group_kinds is not None
    with pytest.raises(ValueError, match='DS_k3d2.*MBI_k3d2_e3'):
        ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {}, primitives=names[:7] + ['MBI_k7d2_e3'])


def test_network_of_dilated_mbi_candidates_is_plain_and_one_with_a_dilated_ds_is_not(lib):
    from tfnas_amd import model_search as ms, geometry as g
    mcs = g.initial_mc_num_dddict()
    names = ['MBI_k3_e3', 'MBI_k3d2_e6', 'MBI_k5d2_e3', 'MBI_k5_e6', 'MBI_k3d2_e3_se', 'MBI_k3_e6_se', 'MBI_k5_e3_se', 'MBI_k5d2_e6_se']
    ref = ms.Network(10, mcs, {})
    net = ms.Network(10, mcs, {}, primitives=names)
    assert net.plain_candidates() and list(net.state_dict()) == list(ref.state_dict())
    assert all([b.dilation for b in c.m_ops] == [1, 2, 2, 1, 2, 1, 1, 2] for c in net.cells())
    one = ms.Network(10, mcs, {}, primitives={'stage3': {'block2': names[:7] + ['DS_k3d2']}})
    assert not one.plain_candidates()


def test_config_export_and_networkcfg_round_trip(lib):
    from collections import OrderedDict
    from tfnas_amd import geometry as g, model_eval as me, parsing
    mcs = g.initial_mc_num_dddict()
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 2)) for i, (st, bl) in enumerate(mcs.items()))
    default = parsing.derived_config(arch, mcs, 20)
    assert not any('dilation' in c for k, v in default.items() if k.startswith('stage') for c in v)
    assert 'dilation' not in default['second_stem']
    assert me.NetworkCfg(20, default).config == default
    names = ['MBI_k3d2_e3', 'MBI_k3_e6', 'MBI_k5d2_e3', 'DS_k5d2', 'MBI_k3d2_e3_se', 'MBI_k3_e6_se', 'DS_k3d2_se', 'MBI_k5d2_e6_se']
    cfg = parsing.derived_config(arch, mcs, 20, primitives=names)
    got = [(c['kernel_size'], c.get('dilation'), c['mid_channels'] > c['in_channels']) for k, v in sorted(cfg.items())
           if k.startswith('stage') for c in v]
    want = []
    for i, st in enumerate(mcs):
        for j in range(min(2, len(mcs[st]))):
            n = names[(i * 3 + j) % 8]
            want.append((g.primitive_block(n, 16, 48)[3], 2 if g.primitive_dilation(n) == 2 else None, not n.startswith('DS')))
    assert got == want and any(w[1] == 2 for w in want) and any(w[1] is None for w in want)
    net = me.NetworkCfg(20, cfg)
    assert net.config == cfg                                                               # reads the key back, writes it back
    blocks = [b for st in net._stages() for b in st]
    assert [b.dilation for b in blocks] == [w[1] or 1 for w in want]
    derived = me.Network(20, arch, mcs, primitives=names)
    assert derived.config == cfg and list(derived.state_dict()) == list(net.state_dict())
    # the counters do not depend on the key
    plain_cfg = {k: ([{kk: vv for kk, vv in c.items() if kk != 'dilation'} for c in v] if k.startswith('stage') else v) for k, v in cfg.items()}
    assert parsing.count_macs_in_M(cfg, 64) == parsing.count_macs_in_M(plain_cfg, 64)
    assert parsing.count_params_in_MB(cfg) == parsing.count_params_in_MB(plain_cfg)
    for bad in (dict(cfg, second_stem=dict(cfg['second_stem'], dilation=2)),):
        with pytest.raises(NotImplementedError):
            me.NetworkCfg(20, bad)
    bad = {k: ([dict(c) for c in v] if k.startswith('stage') else v) for k, v in cfg.items()}
    bad['stage2'][0]['dilation'] = 3
    with pytest.raises(ValueError):
        me.NetworkCfg(20, bad)


def test_lut_key_text():
    from tfnas_amd import geometry as g, model_search as ms, model_eval as me
    assert g.lut_key(14, 80, 0, 80, 3, 1, 'swish') == 'MBInvertedResBlock_14_80_0_80_k3_s1_swish'
    assert g.lut_key(14, 80, 0, 80, 3, 1, 'swish', 2) == 'MBInvertedResBlock_14_80_0_80_k3d2_s1_swish'
    assert g.lut_key(56, 24, 24, 24, 5, 2, 'relu', dilation=2) == 'MBInvertedResBlock_56_24_24_24_k5d2_s2_relu'
    assert g.make_lat_lookup_key_dddict()['stage1']['block1'][2] == 'MBInvertedResBlock_112_16_0_24_k5_s2_relu'

    class Lut(dict):
        def __missing__(self, key):
            self.asked.append(key)
            return {m: 1.0 for m in range(1, 2000)}
    lut = Lut(base=0.0)
    lut.asked = []
    names = ['MBI_k3_e3', 'MBI_k3d2_e6', 'MBI_k5d2_e3', 'MBI_k5_e6', 'MBI_k3d2_e3_se', 'MBI_k3_e6_se', 'MBI_k5_e3_se', 'DS_k5d2_se']
    op = ms.MixedOP(16, 16, 1, False, 'relu', 8, dict(enumerate([48, 96] * 4)), lut, primitives=names)
    assert op.get_lookup_latency(28) == [1.0] * 8
    assert lut.asked == ['MBInvertedResBlock_28_16_%d_16_%s_s1_relu' % (se, kt) for se, kt in
                         ((0, 'k3'), (0, 'k3d2'), (0, 'k5d2'), (0, 'k5'), (16, 'k3d2'), (32, 'k3'), (16, 'k5'), (16, 'k5d2'))]
    import _dil
    import torch
    lut.asked = []
    net = me.NetworkCfg(20, _dil.dil_network_config(20), lut)
    net.get_lookup_latency(torch.zeros(1, 3, 64, 64))
    assert [k.split('_')[5] for k in lut.asked][-3:-1] == ['k5d2', 'k3d2'] and sum('d2' in k for k in lut.asked) == 2


def test_shipped_tables_hold_no_dilated_key():
    from tfnas_amd import load_lat_lookup
    assert not any('d2_' in k for k in load_lat_lookup('gpu') if k != 'base')


def test_epoch_boundary_names_the_primitive_it_refuses():
    from tfnas_amd import epoch, geometry as g
    names = list(g.PRIMITIVES)
    names[2] = 'MBI_k5d2_e3'
    with pytest.raises(NotImplementedError, match=r"search_epoch.*'MBI_k5d2_e3' as candidate 2"):
        epoch.require_default_primitives('search_epoch', names)
    with pytest.raises(NotImplementedError, match=r"stage3\.block2 holds 'DS_k3d2'"):
        epoch.require_default_primitives('run_search', {'stage3': {'block2': names[:2] + ['DS_k3d2'] + names[3:]}})


def test_measurer_describes_a_dilated_block(lib):
    from tfnas_amd import _lib, lut_builder
    d, ws, kind, mc, woff, nw, boff = lut_builder.Measurer._describe(24, 72, 0, 24, 5, 1, 'relu', 28, 28, 4, 'MBInvertedResBlock', 2)
    assert d.g[0].dil == 2 and d.flags & _lib.CELL_DILATION and kind is _lib.MBCONV
    d1 = lut_builder.Measurer._describe(24, 72, 0, 24, 5, 1, 'relu', 28, 28, 4, 'MBInvertedResBlock')[0]
    assert d1.g[0].dil == 0 and d1.flags == 0
    with pytest.raises(NotImplementedError):
        lut_builder.Measurer._describe(24, 72, 0, 24, 3, 1, 'relu', 28, 28, 4, 'FusedMBConvBlock', 2)
