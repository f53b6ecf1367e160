"""CPU-side checks of TFNAS_CELL_NOEXPAND in the C ABI (include/tfnas_hip.h: a block without expand convolution, G = 1,
mc == ic, no expand pointers), through ctypes as tests/test_k7_abi.py does: the constant; the plan accepts such a descriptor
from a caller that set the bit and refuses every malformed one (two groups, mc != ic, an expand pointer, stem / head mode, the
path level); without the bit nothing changes -- 0x200 on an ordinary descriptor is the only thing that was refused before and
is read now; the workspace reports E = 0 and the minimum dxp; neither the E-free nor the fused per-image route is offered; the
Python mirror sets the bit for single-block plans of a block whose inverted_bottleneck is None, and only for those."""
import ctypes as C
import os
import re

import pytest

import _noexp

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


def _fields(st):
    return {f: getattr(st, f) for f, _ in st._fields_}


def test_header_defines_the_flag_and_keeps_the_abi_version():
    from tfnas_amd import _lib
    src = open(HEADER).read()
    m = re.search(r'#define TFNAS_CELL_NOEXPAND (0x[0-9a-fA-F]+)', src)
    assert m and int(m.group(1), 16) == _lib.CELL_NOEXPAND == 0x200
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src)
    assert 'deliberately out of scope' in src           # (a mixed cell with some expand-free candidates)


@pytest.mark.parametrize('k,act,stride,se,ic', [(3, 0, 1, 0, 16), (5, 1, 2, 8, 20), (7, 2, 1, 24, 72), (3, 3, 2, 0, 4)])
def test_plan_accepts_an_expand_free_block(lib, k, act, stride, se, ic):
    d = _noexp.cell_desc(3, 9, 13, ic, ic if stride == 1 else 24, k, stride, act, se, need_wgrad=1)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    assert (d.g[0].mcp, d.g[0].off, d.M % 32, d.SE) == (ic, 0, 0, se) and d.M >= ic
    ws = _noexp.ws_of(lib, d)
    assert ws.E == 0 and ws.dxp == 4
    assert ws.D == 3 * d.Ho * d.Wo * d.M and ws.dx == 3 * 9 * 13 * ic
    assert lib.tfnas_efree_supported(C.byref(d)) == 0 and lib.tfnas_fx_supported(C.byref(d)) == 0
    assert lib.tfnas_cell_route(C.byref(d)) == 1        # TFNAS_ROUTE_TAKEN_VALID only


def test_late_cell_geometry_takes_neither_short_route(lib):
    """14 x 14, 112 channels, frozen weights: with an expand convolution this geometry runs the fused per-image route"""
    from tfnas_amd import _lib
    geo = dict(N=128, H=14, W=14, ic=112, oc=112)
    a = _noexp.cell_desc(mc=336, flags=0, **geo)
    b = _noexp.cell_desc(**geo)
    assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
    assert lib.tfnas_fx_supported(C.byref(a)) == 1 and lib.tfnas_cell_route(C.byref(a)) == 3
    for route in (0, _lib.ROUTE_DW['direct'], _lib.ROUTE_XG_ALL, _lib.ROUTE_GRAM2):
        b.route = route
        assert lib.tfnas_fx_supported(C.byref(b)) == 0 and lib.tfnas_efree_supported(C.byref(b)) == 0
        assert lib.tfnas_cell_route(C.byref(b)) == 1
    e = _noexp.cell_desc(N=8, H=28, W=28, ic=16, oc=24, stride=2)     # (an E-free geometry: ic 16, stride 2)
    assert lib.tfnas_cell_plan(C.byref(e)) == 0 and lib.tfnas_efree_supported(C.byref(e)) == 0


def test_refusals(lib):
    from tfnas_amd import _lib
    ok = dict(N=2, H=9, W=13, ic=16, oc=16)
    assert lib.tfnas_cell_plan(C.byref(_noexp.cell_desc(**ok))) == 0
    assert lib.tfnas_cell_plan(C.byref(_noexp.cell_desc(G=2, **ok))) == EINVAL                 # two groups
    for mc in (8, 24, 17):
        assert lib.tfnas_cell_plan(C.byref(_noexp.cell_desc(mc=mc, **ok))) == EINVAL           # mc != ic
    for field in ('w_expand', 'g_expand'):                                                     # an expand pointer
        d = _noexp.cell_desc(**ok)
        setattr(d.g[0], field, 256)
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    stem = _noexp.cell_desc(2, 0, 0, 27, 16, mc=32, mode=_lib.MODE_STEM, se=8)
    stem.Hi = stem.Wi = 32
    assert lib.tfnas_cell_plan(C.byref(stem)) == EINVAL
    stem.flags = 0
    assert lib.tfnas_cell_plan(C.byref(stem)) == 0                                             # (the same stem without the bit)
    head = _noexp.cell_desc(2, 7, 7, 320, 4, mc=320, mode=_lib.MODE_HEAD)
    assert lib.tfnas_cell_plan(C.byref(head)) == EINVAL
    head.flags = 0
    assert lib.tfnas_cell_plan(C.byref(head)) == 0
    # a descriptor changed after its plan is refused by the entry points before any pointer is looked at
    one = C.c_void_p(16)
    d = _noexp.cell_desc(**ok)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d.g[0].mc = 24
    assert lib.tfnas_mixedop_fwd(C.byref(d), one, None, None, one, one, one, one, one, one, None) == EINVAL
    head.flags = _lib.CELL_NOEXPAND
    assert lib.tfnas_head_fwd(C.byref(head), one, one, one, one, one, None) == EINVAL
    # affine form: BatchNorm site 0 does not exist
    d = _noexp.cell_desc(**ok)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    for field in ('weight', 'bias', 'g_weight', 'g_bias', 'running_mean', 'running_var'):
        bn = _lib.TfnasBnAffine()
        getattr(bn, field)[0] = 256
        assert lib.tfnas_mbconv_fwd(C.byref(d), C.byref(bn), None, one, None, one, one, one, one, one, one, None) == EINVAL
    # without the bit E stays a required pointer
    plain = _noexp.cell_desc(mc=48, flags=0, need_wgrad=1, **ok)
    assert lib.tfnas_cell_plan(C.byref(plain)) == 0
    assert lib.tfnas_mixedop_fwd(C.byref(plain), one, None, None, one, one, one, one, one, one, None) == -2    # TFNAS_ENULL


@pytest.mark.gpu          # (tfnas_path_create makes streams and events: it needs a device; nothing is launched)
def test_path_level_refuses_a_cell_with_the_bit(lib):
    from tfnas_amd import _lib
    ctx = C.c_void_p(None)
    assert lib.tfnas_path_create(C.byref(ctx)) == 0
    try:
        beta = C.c_void_p(256)
        for flags, want in ((0, 0), (_lib.CELL_NOEXPAND, EINVAL)):
            pd = _lib.TfnasPathDesc()
            pd.ncell, pd.nstage, pd.soft, pd.need_dx0 = 1, 1, 0, 1
            pd.stage[0].ncell, pd.stage[0].start_res, pd.stage[0].betas = 1, 0, beta
            src = _noexp.cell_desc(2, 9, 13, 16, 16, flags=flags, mc=16 if flags else 48)
            C.memmove(C.byref(pd.cell[0]), C.byref(src), C.sizeof(src))
            ws = _lib.TfnasPathWs()
            assert lib.tfnas_path_plan(ctx, C.byref(pd), C.byref(ws)) == want
    finally:
        lib.tfnas_path_destroy(ctx)


# descriptors that planned before the bit existed: (kwargs of _noexp.cell_desc with flags given, G)
_OLD = [
    dict(N=2, H=9, W=13, ic=16, oc=16, mc=48, k=3, act=0, se=0),
    dict(N=2, H=9, W=13, ic=16, oc=24, mc=53, k=5, act=1, se=16, stride=2),
    dict(N=128, H=14, W=14, ic=112, oc=112, mc=336, k=5, act=1, se=112),
    dict(N=4, H=28, W=28, ic=40, oc=40, mc=120, k=3, act=1, se=0, G=8),
    dict(N=2, H=9, W=13, ic=16, oc=16, mc=16, k=3, act=0, se=0),          # mc == ic WITH an expand convolution: stays legal
    dict(N=2, H=9, W=13, ic=24, oc=24, mc=8, k=3, act=0, se=0),           # ... and so does mc < ic
]


@pytest.mark.parametrize('kw', _OLD, ids=lambda kw: '%dx%d_ic%d_mc%d_G%d' % (kw['H'], kw['W'], kw['ic'], kw['mc'], kw.get('G', 1)))
@pytest.mark.parametrize('need_wgrad', [0, 1])
def test_descriptors_without_the_bit_plan_as_before(lib, kw, need_wgrad):
    """the bit-free descriptor is untouched by the feature: it plans, and every [plan] field, workspace size and route query
    equals that of the same descriptor with the other additive bits set (which never moved them); the one thing that changed is
    that 0x200 on it is now READ -- and refused, as it was when it was undefined, because the descriptor has an expand convolution"""
    from tfnas_amd import _lib
    a = _noexp.cell_desc(flags=0, need_wgrad=need_wgrad, **kw)
    b = _noexp.cell_desc(flags=_lib.CELL_K7 | _lib.CELL_ACTS | _lib.CELL_ACCUM_WGRAD, need_wgrad=need_wgrad, **kw)
    assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
    fa, fb = _fields(a), _fields(b)
    for f in ('Ho', 'Wo', 'M', 'SE'):
        assert fa[f] == fb[f]
    for g in range(a.G):
        assert (a.g[g].mcp, a.g[g].off, a.g[g].se_off) == (b.g[g].mcp, b.g[g].off, b.g[g].se_off)
    wa, wb = _fields(_noexp.ws_of(lib, a)), _fields(_noexp.ws_of(lib, b))
    assert wa == wb
    P = kw['N'] * kw['H'] * kw['W']
    assert wa['E'] == P * a.M and wa['dEh'] == P * a.M and wa['dx'] == P * kw['ic']
    for fn in (lib.tfnas_efree_supported, lib.tfnas_fx_supported, lib.tfnas_cell_route):
        assert fn(C.byref(a)) == fn(C.byref(b))
    c = _noexp.cell_desc(flags=_lib.CELL_NOEXPAND, need_wgrad=need_wgrad, **kw)
    c.g[0].w_expand = 256
    assert lib.tfnas_cell_plan(C.byref(c)) == EINVAL


def test_workspace_of_the_expand_free_block_differs_only_where_documented(lib):
    from tfnas_amd import _lib
    geo = dict(N=2, H=9, W=13, ic=16, oc=16, k=5, se=8, need_wgrad=1)
    a = _noexp.cell_desc(flags=0, mc=16, **geo)
    b = _noexp.cell_desc(**geo)
    assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
    wa, wb = _fields(_noexp.ws_of(lib, a)), _fields(_noexp.ws_of(lib, b))
    assert wb['E'] == 0 and wb['dxp'] == 4 and wb['dEh'] == wa['dEh']
    assert {f for f in wa if wa[f] != wb[f]} <= {'E', 'dxp'}


def test_python_mirror_sets_the_bit_for_expand_free_single_block_plans_only():
    from tfnas_amd import _lib, functions as F
    from tfnas_amd.layers import MBInvertedResBlock
    free = MBInvertedResBlock(16, 16, 8, 24, 3, 2)
    free8 = MBInvertedResBlock(16, 8, 0, 16, 5, 1)
    full = MBInvertedResBlock(16, 48, 8, 24, 3, 2)
    assert free.inverted_bottleneck is None and free8.inverted_bottleneck is None and free8.mid_channels == 16
    assert len(free.hip_params()) == 6 and len(free8.hip_params()) == 2 and len(full.hip_params()) == 7
    # (the descriptor a CellPlan fills from its blocks: mc = the block's normalised mid_channels)
    for blocks, mode, want in (([free], _lib.MODE_CELL, _lib.CELL_NOEXPAND), ([free8], _lib.MODE_CELL, _lib.CELL_NOEXPAND),
                               ([full], _lib.MODE_CELL, 0), ([free, free], _lib.MODE_CELL, 0), ([full, free], _lib.MODE_CELL, 0),
                               ([free], _lib.MODE_STEM, 0), ([free], _lib.MODE_HEAD, 0)):
        d = _noexp.cell_desc(2, 9, 13, 16, 24, stride=2, flags=0, mode=mode, G=len(blocks))
        for g, b in enumerate(blocks):
            d.g[g].mc = b.mid_channels
        F.HipModes().apply(d)
        assert d.flags == want, (mode, want)
        F.HipModes(lazy_join=True).apply(d)
        assert d.flags == want | _lib.CELL_LAZY_JOIN
    # the plan of such a block binds no expand pointer, and the library plans its descriptor (on the CPU: no launch)
    plan = F.CellPlan(16, 24, 2, 'relu', [free])
    d, ws = plan.desc(2, 9, 13)
    assert d.flags & _lib.CELL_NOEXPAND and ws.E == 0 and d.g[0].mc == 16
    params = free.hip_params()
    plan.bind(d, params, params)
    assert not d.g[0].w_expand and not d.g[0].g_expand
    assert d.g[0].w_dw == params[0].data_ptr() and d.g[0].b_se_e == params[5].data_ptr() == d.g[0].gb_se_e
    affine = MBInvertedResBlock(16, 16, 0, 16, 3, 1, affine=True)
    assert len(affine.bn_modules()) == 2 and len(MBInvertedResBlock(16, 32, 0, 16, 3, 1, affine=True).bn_modules()) == 3


def test_network_cfg_builds_counts_and_round_trips_on_the_host():
    """a model.config whose stage1 opens with mid_channels == in_channels (and one that says mid < in) builds; parameter names
    carry no inverted_bottleneck for that block; count_macs_in_M follows the hand formula; ``config`` round-trips"""
    import copy
    from tfnas_amd import model_eval as me, parsing
    cfg = _noexp.noexp_network_config(20)
    m = me.NetworkCfg(20, cfg, None, 0.0, 0.2)
    names = [k for k, _ in m.stage1[0].named_parameters()]
    assert m.stage1[0].inverted_bottleneck is None and not any('inverted_bottleneck' in k for k in names)
    assert any('inverted_bottleneck' in k for k, _ in m.stage1[1].named_parameters())
    assert m.config == cfg and me.NetworkCfg(20, m.config).config == cfg
    for size in (64, 224):
        assert abs(parsing.count_macs_in_M(cfg, size) - _noexp.hand_macs_in_M(cfg, size)) < 1e-9
    low = copy.deepcopy(cfg)
    low['stage1'][0]['mid_channels'] = 8                       # mid < in: the same block, recorded back as mid == in
    assert me.NetworkCfg(20, low).config == cfg
    assert abs(parsing.count_macs_in_M(low, 64) - parsing.count_macs_in_M(cfg, 64)) < 1e-9
