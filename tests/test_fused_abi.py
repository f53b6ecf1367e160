"""CPU-side checks of TFNAS_CELL_FUSED in the C ABI (include/tfnas_hip.h: one Fused-MBConv block -- G = 1, k = 3, the dense OIHW
weight in w_expand, no depthwise pointer), through ctypes as tests/test_noexp_abi.py does: the constant; the plan accepts such a
descriptor (ragged widths, both strides, four activations) and refuses every malformed one (two groups, k != 3, a depthwise
pointer, the bit together with TFNAS_CELL_NOEXPAND, stem / head mode, the path level); a width whose weight-gradient partial row
does not fit is TFNAS_ERANGE; the workspace reports E = 0; neither short route is
offered; without the bit nothing changes; the Python module, its plan and the host side of NetworkCfg / parsing."""
import ctypes as C
import os
import re

import pytest

import _fused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL, ENULL, ERANGE = -1, -2, -3


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
    m = re.search(r'#define TFNAS_CELL_FUSED (0x[0-9a-fA-F]+)', src)
    assert m and int(m.group(1), 16) == _lib.CELL_FUSED == 0x400
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src)
    assert re.search(r'#define TFNAS_ERANGE \(?(-3)\)?', src)


@pytest.mark.parametrize('act,stride,se,ic,mc', [(0, 1, 0, 16, 40), (1, 2, 8, 20, 22), (2, 1, 24, 72, 72), (3, 2, 0, 4, 1),
                                                 (0, 1, 8, 24, 24), (1, 1, 0, 80, 240)])
def test_plan_accepts_a_fused_block(lib, act, stride, se, ic, mc):
    d = _fused.cell_desc(3, 9, 13, ic, ic if stride == 1 else 24, mc, stride, act, se, need_wgrad=1)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0            # (TFNAS_EINVAL before the bit existed)
    assert (d.g[0].mcp, d.g[0].off, d.M % 32, d.SE) == ((mc + 3) & ~3, 0, 0, se) and d.M >= mc
    assert (d.Ho, d.Wo) == ((9 - 1) // stride + 1, (13 - 1) // stride + 1)
    ws = _fused.ws_of(lib, d)
    assert ws.E == 0 and ws.dxp == 4
    assert ws.D == 3 * d.Ho * d.Wo * d.M and ws.dx == 3 * 9 * 13 * ic and ws.dEh == 3 * 9 * 13 * d.M
    assert lib.tfnas_efree_supported(C.byref(d)) == 0 and lib.tfnas_fx_supported(C.byref(d)) == 0
    assert lib.tfnas_cell_route(C.byref(d)) == 1           # TFNAS_ROUTE_TAKEN_VALID only


def test_late_cell_geometry_takes_neither_short_route(lib):
    from tfnas_amd import _lib
    geo = dict(N=128, H=14, W=14, ic=112, oc=112, mc=336)
    a = _fused.cell_desc(flags=0, **geo)
    b = _fused.cell_desc(**geo)
    assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
    assert lib.tfnas_fx_supported(C.byref(a)) == 1 and lib.tfnas_cell_route(C.byref(a)) == 3
    for route in (0, _lib.ROUTE_DW['direct'], _lib.ROUTE_XG_ALL, _lib.ROUTE_GRAM2):
        b.route = route
        assert lib.tfnas_fx_supported(C.byref(b)) == 0 and lib.tfnas_efree_supported(C.byref(b)) == 0
        assert lib.tfnas_cell_route(C.byref(b)) == 1
    e = _fused.cell_desc(N=8, H=28, W=28, ic=16, oc=24, mc=48, stride=2)      # (an E-free geometry: ic 16, stride 2)
    assert lib.tfnas_cell_plan(C.byref(e)) == 0 and lib.tfnas_efree_supported(C.byref(e)) == 0


def test_refusals(lib):
    from tfnas_amd import _lib
    ok = dict(N=2, H=9, W=13, ic=16, oc=16, mc=40)
    assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(**ok))) == 0
    assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(G=2, **ok))) == EINVAL                 # two groups
    for k in (5, 7):                                                                           # k != 3
        assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(k=k, flags=_lib.CELL_FUSED | _lib.CELL_K7, **ok))) == EINVAL
    for field in ('w_dw', 'g_dw'):                                                             # a depthwise pointer
        d = _fused.cell_desc(**ok)
        setattr(d.g[0], field, 256)
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    for mc in (16, 40):                                                                        # with TFNAS_CELL_NOEXPAND
        d = _fused.cell_desc(**dict(ok, mc=mc, flags=_lib.CELL_FUSED | _lib.CELL_NOEXPAND))
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(**dict(ok, ic=18)))) == EINVAL         # ic no multiple of 4
    assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(se=6, **ok))) == EINVAL                # se no multiple of 4
    assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(**dict(ok, mc=0)))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(act=2, flags=_lib.CELL_FUSED, **ok))) == EINVAL   # relu6 without its bit
    stem = _fused.cell_desc(2, 0, 0, 27, 16, 32, mode=_lib.MODE_STEM, se=8)
    stem.Hi = stem.Wi = 32
    assert lib.tfnas_cell_plan(C.byref(stem)) == EINVAL
    stem.flags = 0
    assert lib.tfnas_cell_plan(C.byref(stem)) == 0                                             # (the same stem without the bit)
    head = _fused.cell_desc(2, 7, 7, 320, 4, 320, mode=_lib.MODE_HEAD)
    assert lib.tfnas_cell_plan(C.byref(head)) == EINVAL
    head.flags = 0
    assert lib.tfnas_cell_plan(C.byref(head)) == 0
    # a descriptor changed after its plan is refused by the entry points before any pointer is looked at
    one = C.c_void_p(16)
    d = _fused.cell_desc(**ok)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d.g[0].k = 5
    assert lib.tfnas_mixedop_fwd(C.byref(d), one, None, None, one, one, one, one, one, one, None) == EINVAL
    d.g[0].k, d.g[0].w_dw = 3, 256
    assert lib.tfnas_mixedop_bwd(C.byref(d), one, None, None, one, one, one, one, one, one, one, one, one, one, None, None, None,
                                 None) == EINVAL
    head.flags = _lib.CELL_FUSED
    assert lib.tfnas_head_fwd(C.byref(head), one, one, one, one, one, None) == EINVAL
    # affine form: BatchNorm site 0 does not exist
    d = _fused.cell_desc(**ok)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    for field in ('weight', 'bias', 'g_weight', 'g_bias', 'running_mean', 'running_var'):
        bn = _lib.TfnasBnAffine()
        getattr(bn, field)[0] = 256
        assert lib.tfnas_mbconv_fwd(C.byref(d), C.byref(bn), None, one, None, one, one, one, one, one, one, None) == EINVAL
        assert lib.tfnas_mbconv_bwd(C.byref(d), C.byref(bn), None, one, None, one, one, one, one, one, None, one, one, one, one,
                                    one, None, None, None) == EINVAL


def test_weight_gradient_row_that_does_not_fit_is_erange(lib):
    from tfnas_amd import _lib
    part = int(lib.tfnas_sizeof(7)) - int(lib.tfnas_sizeof(8))            # floats of the partial-row region

    def fits(ic, mc):
        """the documented rule: the partial row 9 ic mc, and the repacked weight 9 ic mcp (rounded up to 64 floats) next to 128
        statistics rows of 2 M floats -- M = mcp rounded up to 32, plus 32 where that is a multiple of 512"""
        mcp = (mc + 3) // 4 * 4
        M = (mcp + 31) // 32 * 32
        M += 32 if M % 512 == 0 else 0
        return 9 * ic * mc <= part and (9 * ic * mcp + 63) // 64 * 64 + 128 * 2 * M <= part

    for ic in (1024, 4):
        geo = dict(N=1, H=4, W=4, ic=ic, oc=16)
        last = max(mc for mc in range(4, part // (9 * ic) + 8, 4) if fits(ic, mc))
        assert fits(ic, last) and not fits(ic, last + 1)
        assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(mc=last, **geo))) == 0
        d = _fused.cell_desc(mc=last + 1, **geo)
        assert lib.tfnas_cell_plan(C.byref(d)) == ERANGE
        ws = _lib.TfnasCellWs()
        assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == ERANGE
    # the widest block of the supernet fits (7 x 7, 192 -> 1536); the depthwise limit -- 9 mc floats in one partial row -- is
    # the weaker one for every ic >= 4, so a fused cell is bounded by its own rows alone
    assert lib.tfnas_cell_plan(C.byref(_fused.cell_desc(2, 7, 7, 192, 320, 1536, 1, 1, 384))) == 0


@pytest.mark.gpu          # (tfnas_path_create makes streams and events: it needs a device; nothing is launched)
def test_path_level_refuses_a_cell_with_the_bit(lib):
    from tfnas_amd import _lib
    ctx = C.c_void_p(None)
    assert lib.tfnas_path_create(C.byref(ctx)) == 0
    try:
        beta = C.c_void_p(256)
        for flags, want in ((0, 0), (_lib.CELL_FUSED, EINVAL)):
            pd = _lib.TfnasPathDesc()
            pd.ncell, pd.nstage, pd.soft, pd.need_dx0 = 1, 1, 0, 1
            pd.stage[0].ncell, pd.stage[0].start_res, pd.stage[0].betas = 1, 0, beta
            src = _fused.cell_desc(2, 9, 13, 16, 16, 48, flags=flags)
            C.memmove(C.byref(pd.cell[0]), C.byref(src), C.sizeof(src))
            ws = _lib.TfnasPathWs()
            assert lib.tfnas_path_plan(ctx, C.byref(pd), C.byref(ws)) == want
    finally:
        lib.tfnas_path_destroy(ctx)


# descriptors that planned before the bit existed: [plan] fields, workspace sizes and route answers as the library gave them
# before TFNAS_CELL_FUSED was added
_OLD = [
    (dict(N=2, H=9, W=13, ic=16, oc=16, mc=48, k=3, act=0, se=0), 0,
     dict(Ho=9, Wo=13, M=64, SE=0, mcp=48, E=14976, D=14976, dEh=14976, dxp=4, dx=3744, bsmall=640, efree=1, fx=0, route=1)),
    (dict(N=2, H=9, W=13, ic=16, oc=24, mc=53, k=5, act=1, se=16, stride=2), 0,
     dict(Ho=5, Wo=7, M=64, SE=16, mcp=56, E=14976, D=4480, dEh=14976, dxp=4, dx=3744, bsmall=672, efree=1, fx=0, route=1)),
    (dict(N=128, H=14, W=14, ic=112, oc=112, mc=336, k=5, act=1, se=112), 0,
     dict(Ho=14, Wo=14, M=352, SE=112, mcp=336, E=8830976, D=8830976, dEh=8830976, dxp=14049280, dx=2809856, bsmall=150912,
          efree=1, fx=1, route=3)),
    (dict(N=4, H=28, W=28, ic=40, oc=40, mc=120, k=3, act=1, se=0, G=8), 0,
     dict(Ho=28, Wo=28, M=1056, SE=0, mcp=120, E=3311616, D=3311616, dEh=3311616, dxp=2007040, dx=125440, bsmall=16896,
          efree=1, fx=0, route=1)),
    (dict(N=2, H=9, W=13, ic=16, oc=16, mc=16, k=3, act=0, se=0), 0x200,
     dict(Ho=9, Wo=13, M=32, SE=0, mcp=16, E=0, D=7488, dEh=7488, dxp=4, dx=3744, bsmall=320, efree=0, fx=0, route=1)),
]


@pytest.mark.parametrize('kw,flags,want', _OLD, ids=lambda v: None)
def test_descriptors_without_the_bit_plan_as_before(lib, kw, flags, want):
    d = _fused.cell_desc(flags=flags, **kw)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    ws = _fused.ws_of(lib, d)
    got = dict(Ho=d.Ho, Wo=d.Wo, M=d.M, SE=d.SE, mcp=d.g[0].mcp, E=ws.E, D=ws.D, dEh=ws.dEh, dxp=ws.dxp, dx=ws.dx, bsmall=ws.bsmall,
               efree=lib.tfnas_efree_supported(C.byref(d)), fx=lib.tfnas_fx_supported(C.byref(d)),
               route=lib.tfnas_cell_route(C.byref(d)))
    assert got == want
    # ... and the other additive bits still do not move any of it
    from tfnas_amd import _lib
    b = _fused.cell_desc(flags=flags | _lib.CELL_K7 | _lib.CELL_ACTS | _lib.CELL_ACCUM_WGRAD, **kw)
    assert lib.tfnas_cell_plan(C.byref(b)) == 0 and _fields(_fused.ws_of(lib, b)) == _fields(ws)
    # the fused bit on a descriptor with a depthwise pointer is refused, as every unknown bit was
    c = _fused.cell_desc(flags=flags | _lib.CELL_FUSED, **kw)
    c.g[0].w_dw = 256
    assert lib.tfnas_cell_plan(C.byref(c)) == EINVAL


def test_workspace_of_the_fused_block_differs_only_where_documented(lib):
    geo = dict(N=2, H=9, W=13, ic=16, oc=16, mc=40, se=8, need_wgrad=1)
    a = _fused.cell_desc(flags=0, **geo)
    b = _fused.cell_desc(**geo)
    assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
    wa, wb = _fields(_fused.ws_of(lib, a)), _fields(_fused.ws_of(lib, b))
    assert wb['E'] == 0 and wb['dxp'] == 4 and wb['dEh'] == wa['dEh']
    assert {f for f in wa if wa[f] != wb[f]} <= {'E', 'dxp'}


def test_module_plan_and_python_mirror():
    from tfnas_amd import _lib, functions as F
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock
    blk = FusedMBConvBlock(16, 40, 8, 24, 3, 2, act_func='h-swish')
    same = FusedMBConvBlock(16, 16, 0, 16, 3, 1)                         # mid == in stays a dense convolution
    assert blk.name == 'FusedMBConvBlock' and not blk.has_residual and same.has_residual and blk.drop_connect_rate == 0.0
    assert [k for k, _ in blk.named_parameters()] == [
        'fused_conv.conv.weight', 'squeeze_excite.conv_reduce.weight', 'squeeze_excite.conv_reduce.bias',
        'squeeze_excite.conv_expand.weight', 'squeeze_excite.conv_expand.bias', 'point_linear.conv.weight']
    assert blk.fused_conv.conv.weight.shape == (40, 16, 3, 3) and len(blk.hip_params()) == 6 and len(same.hip_params()) == 2
    aff = FusedMBConvBlock(16, 40, 0, 16, 3, 1, affine=True)
    assert len(aff.bn_modules()) == 2 and 'fused_conv.bn.running_mean' in dict(aff.named_buffers())
    with pytest.raises(NotImplementedError):
        FusedMBConvBlock(16, 40, 0, 16, 5, 1)
    with pytest.raises(RuntimeError):
        blk(__import__('torch').zeros(1, 16, 4, 4))                     # the hot path has no CPU implementation
    for b, want in ((blk, _lib.CELL_FUSED | _lib.CELL_ACTS), (same, _lib.CELL_FUSED)):
        plan = F.CellPlan(b.in_channels, b.out_channels, b.stride, b.act_func, [b])
        d, ws = plan.desc(2, 9, 13)
        assert d.flags == want and ws.E == 0 and d.g[0].mc == b.mid_channels and d.g[0].k == 3
        ps = b.hip_params()
        plan.bind(d, ps, ps)
        assert d.g[0].w_expand == ps[0].data_ptr() == d.g[0].g_expand and d.g[0].w_proj == ps[1].data_ptr()
        assert not d.g[0].w_dw and not d.g[0].g_dw
        if b.se_channels:
            assert d.g[0].b_se_e == ps[5].data_ptr() == d.g[0].gb_se_e
    # an MBConv plan never gets the bit; a fused block is no candidate of a multi-candidate launch
    mb = MBInvertedResBlock(16, 48, 8, 24, 3, 2)
    d, _ = F.CellPlan(16, 24, 2, 'relu', [mb]).desc(2, 9, 13)
    assert not d.flags & _lib.CELL_FUSED
    with pytest.raises(NotImplementedError):
        F.CellPlan(16, 24, 2, 'relu', [mb, FusedMBConvBlock(16, 40, 8, 24, 3, 2)])


def test_network_cfg_builds_counts_and_round_trips_on_the_host():
    import copy
    from tfnas_amd import model_eval as me, parsing
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock
    cfg = _fused.fused_network_config(20)
    m = me.NetworkCfg(20, cfg, None, 0.0, 0.2)
    assert [type(b) for b in m.stage1] == [FusedMBConvBlock, FusedMBConvBlock] and type(m.stage2[0]) is MBInvertedResBlock
    assert type(m.second_stem) is MBInvertedResBlock
    assert m.stage1[1].has_residual and m.stage1[1].mid_channels == 50 and m.stage1[1].drop_connect_rate > 0
    assert m.config == cfg and me.NetworkCfg(20, m.config).config == cfg
    for size in (64, 224):
        macs, params = _fused.hand_counts(cfg, size)
        assert abs(parsing.count_macs_in_M(cfg, size) - macs) < 1e-9
        assert abs(parsing.count_params_in_MB(cfg) - params) < 1e-12
    assert abs(parsing.count_params_in_MB(cfg) - sum(p.numel() for p in m.parameters()) / 1e6) < 1e-12
    lut = {'base': 1.0}
    size = 32
    for st in m._stages():
        for b in st:
            key = '{}_{}_{}_{}_{}_k{}_s{}_{}'.format(b.name, size, b.in_channels, b.se_channels, b.out_channels, b.kernel_size,
                                                     b.stride, b.act_func)
            lut.setdefault(key, {})[b.mid_channels] = 0.5
            size = (size - 1) // b.stride + 1
    assert sum(k.startswith('FusedMBConvBlock_') for k in lut) == 2
    m.lat_lookup = lut
    nblk = sum(len(st) for st in m._stages())
    assert abs(m.get_lookup_latency(__import__('torch').zeros(1, 3, 64, 64)) - (1.0 + 0.5 * nblk)) < 1e-9
    bad = copy.deepcopy(cfg)
    bad['second_stem']['name'] = 'FusedMBConvBlock'                    # second_stem stays an MBConv
    with pytest.raises(NotImplementedError):
        me.NetworkCfg(20, bad)
    bad = copy.deepcopy(cfg)
    bad['stage1'][0]['kernel_size'] = 5
    with pytest.raises(NotImplementedError):
        me.NetworkCfg(20, bad)
