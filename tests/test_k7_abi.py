"""CPU-side checks of depthwise kernel size 7 in the C ABI (include/tfnas_hip.h: TfnasGroup.k is 3, 5 or -- in a descriptor that
carries TFNAS_CELL_K7 -- 7), through ctypes as tests/test_accum_abi.py does: the plan accepts 7 from a caller that set the bit,
refuses it from one that did not (as it always has: tests/test_capi_symbols.py) and still refuses every other size; the bit changes
nothing for 3 x 3 / 5 x 5 cells; nothing in the workspace depends on the
kernel size, a cell with a 7 x 7 group takes the materialised route (neither E-free nor the fused per-image route), and the
route of 3 x 3 / 5 x 5 cells is what it was.  The depthwise weight-gradient partial row (sum of mc * k * k) must fit the
partials region: the elasticity bound does, a descriptor that does not is refused with TFNAS_ERANGE."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL, ERANGE = -1, -3


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _desc(N=2, H=9, W=11, ic=24, oc=24, stride=1, mids=(32, 53), ks=(3, 7), ses=(0, 24), need_wgrad=0, k7=True):
    from tfnas_amd import _lib
    d = _lib.TfnasCellDesc()
    d.flags = _lib.CELL_K7 if k7 else 0
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G = N, H, W, ic, oc, stride, 1, len(mids)
    d.has_res = int(ic == oc and stride == 1)
    d.eps = 1e-5
    d.need_wgrad = need_wgrad
    for g, (m, k, s) in enumerate(zip(mids, ks, ses)):
        d.g[g].mc, d.g[g].k, d.g[g].se = m, k, s
    return d


def _ws(lib, d):
    from tfnas_amd import _lib
    ws = _lib.TfnasCellWs()
    assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == 0
    return {f: getattr(ws, f) for f, _ in ws._fields_}


def test_header_documents_three_kernel_sizes_and_keeps_the_abi_version():
    from tfnas_amd import _lib
    src = open(HEADER).read()
    assert re.search(r'int32_t k;\s*/\* depthwise kernel size: 3 or 5; 7 with TFNAS_CELL_K7', src)
    m = re.search(r'#define TFNAS_CELL_K7 (0x[0-9a-fA-F]+)', src)
    assert m and int(m.group(1), 16) == _lib.CELL_K7 == 0x80
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src)
    assert ERANGE == -int(re.search(r'#define TFNAS_ERANGE \(?-(\d+)', src).group(1))


def test_plan_accepts_kernel_size_7(lib):
    for ks in ((3, 7), (7, 7), (7, 5)):
        for stride in (1, 2):
            d = _desc(ks=ks, stride=stride, oc=24 if stride == 1 else 40)
            assert lib.tfnas_cell_plan(C.byref(d)) == 0, (ks, stride)
            assert (d.Ho, d.Wo) == ((9 - 1) // stride + 1, (11 - 1) // stride + 1)         # pad = k / 2: the size of k = 3 / 5
    d = _desc(mids=(72,), ks=(7,), ses=(0,), need_wgrad=1)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0


def test_k7_is_opt_in_and_the_bit_changes_nothing_else(lib):
    """without TFNAS_CELL_K7 a 7 x 7 group is refused as before the bit existed, by the plan and -- should the bit be dropped
    after it -- by the entry points; with the bit a 3 x 3 / 5 x 5 descriptor plans, sizes and routes exactly as without it"""
    from tfnas_amd import _lib
    for ks in ((3, 7), (7, 5)):
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=ks, k7=False))) == EINVAL
        d = _desc(ks=ks, k7=False)
        d.flags = _lib.CELL_LAZY_JOIN | _lib.CELL_ACCUM_WGRAD
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    d = _desc()
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d.flags = 0                                      # (a descriptor changed after its plan: refused before any pointer is looked at)
    one = C.c_void_p(16)
    assert lib.tfnas_mixedop_fwd(C.byref(d), one, None, one, one, one, one, one, one, one, None) == EINVAL
    geo = dict(N=128, H=14, W=14, ic=112, oc=112, mids=(336, 672, 336), ks=(3, 5, 5), ses=(0, 0, 112))
    a, b = _desc(k7=False, **geo), _desc(k7=True, **geo)
    assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
    assert (a.M, a.SE, a.Ho, a.Wo) == (b.M, b.SE, b.Ho, b.Wo) and _ws(lib, a) == _ws(lib, b)
    for fn in (lib.tfnas_efree_supported, lib.tfnas_fx_supported, lib.tfnas_cell_route):
        assert fn(C.byref(a)) == fn(C.byref(b))
    assert lib.tfnas_fx_supported(C.byref(b)) == 1


def test_python_mirror_sets_the_bit_for_k7_descriptors_only():
    from tfnas_amd import _lib, functions as F
    for ks, want in (((3, 5), 0), ((3, 7), _lib.CELL_K7)):
        d = _desc(ks=ks, k7=False)
        F.HipModes().apply(d)
        assert d.flags == want
        F.HipModes(lazy_join=True).apply(d)
        assert d.flags == want | _lib.CELL_LAZY_JOIN


@pytest.mark.parametrize('k', [0, 1, 4, 6, 9])
def test_plan_still_refuses_every_other_kernel_size(lib, k):
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3, k)))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(mids=(48,), ks=(k,), ses=(0,)))) == EINVAL


@pytest.mark.parametrize('need_wgrad', [0, 1])
@pytest.mark.parametrize('stride', [1, 2])
def test_workspace_does_not_depend_on_the_kernel_size(lib, stride, need_wgrad):
    geo = dict(N=4, H=14, W=14, ic=40, oc=40 if stride == 1 else 80, stride=stride, mids=(120, 240, 131), ses=(0, 40, 80),
               need_wgrad=need_wgrad)
    d7, d5 = _desc(ks=(3, 7, 7), **geo), _desc(ks=(3, 5, 5), **geo)
    assert lib.tfnas_cell_plan(C.byref(d7)) == 0 and lib.tfnas_cell_plan(C.byref(d5)) == 0
    assert (d7.M, d7.SE, d7.Ho, d7.Wo) == (d5.M, d5.SE, d5.Ho, d5.Wo)
    assert [(d7.g[g].off, d7.g[g].mcp, d7.g[g].se_off) for g in range(3)] == [(d5.g[g].off, d5.g[g].mcp, d5.g[g].se_off) for g in range(3)]
    assert _ws(lib, d7) == _ws(lib, d5)


def test_k7_cells_take_the_materialised_route(lib):
    from tfnas_amd import _lib
    # the geometries where the 3 x 3 / 5 x 5 cell is E-free / fused (frozen weights): stride-2 ic 16 at 112 x 112, ic 112 at 14 x 14
    for geo in (dict(N=8, H=112, W=112, ic=16, oc=24, stride=2, mids=(48, 96), ses=(0, 16)),
                dict(N=8, H=14, W=14, ic=112, oc=112, stride=1, mids=(336, 672), ses=(0, 0))):
        d5 = _desc(ks=(3, 5), k7=False, **geo)
        assert lib.tfnas_cell_plan(C.byref(d5)) == 0
        assert lib.tfnas_efree_supported(C.byref(d5)) == 1
        for ks in ((3, 7), (7, 5), (7, 7)):
            d7 = _desc(ks=ks, **geo)
            assert lib.tfnas_cell_plan(C.byref(d7)) == 0
            assert lib.tfnas_efree_supported(C.byref(d7)) == 0
            assert lib.tfnas_fx_supported(C.byref(d7)) == 0
            assert lib.tfnas_cell_route(C.byref(d7)) == _lib.ROUTE_TAKEN_VALID


def test_route_of_k3_k5_cells_is_unchanged(lib):
    """the 18 cells of the search space at B = 128, all eight candidates, frozen weights: fused per-image route on the stride-1
    14 x 14 / 7 x 7 cells with 64 <= ic <= 192 and nowhere else (the table of tests/test_capi_symbols.py)"""
    from tfnas_amd import _lib, geometry as g
    got = []
    for stage, block, ic, oc, stride, act, size in g.iter_cells():
        d = _desc(N=128, H=size, W=size, ic=ic, oc=oc, stride=stride, mids=(3 * ic, 6 * ic) * 4, ks=(3, 3, 5, 5) * 2,
                  ses=(0,) * 4 + (4 * (ic // 4),) * 4, k7=False)
        assert lib.tfnas_cell_plan(C.byref(d)) == 0
        got.append((lib.tfnas_fx_supported(C.byref(d)), lib.tfnas_cell_route(C.byref(d))))
    fx = [int(6 <= i <= 16 and i != 13 or i == 17) for i in range(18)]
    assert [f for f, _ in got] == fx
    assert [r for _, r in got] == [_lib.ROUTE_TAKEN_VALID | (_lib.ROUTE_TAKEN_FX if f else 0) for f in fx]


def test_weight_gradient_partial_row_bound(lib):
    """eight 7 x 7 groups of 1536 channels (the elasticity bound of the widest cell) plan; a row that cannot fit the partials
    region once (sum of mc * k * k above 4 Mi - 1024 floats) is refused by the plan and by the workspace query"""
    from tfnas_amd import _lib
    geo = dict(N=2, H=7, W=7, ic=192, oc=192, stride=1, ses=(0,) * 8, need_wgrad=1)
    d = _desc(mids=(1536,) * 8, ks=(7,) * 8, **geo)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    _ws(lib, d)
    per_group = ((4 << 20) - 1024) // (8 * 49) + 4
    d = _desc(mids=(per_group,) * 8, ks=(7,) * 8, **geo)
    assert lib.tfnas_cell_plan(C.byref(d)) == ERANGE
    ok = _desc(mids=(per_group - 8,) * 8, ks=(7,) * 8, **geo)
    assert lib.tfnas_cell_plan(C.byref(ok)) == 0
    ok.g[7].mc = 4 * per_group                       # (a descriptor changed after its plan)
    assert lib.tfnas_cell_ws(C.byref(ok), C.byref(_lib.TfnasCellWs())) == ERANGE
