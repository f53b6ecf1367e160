"""CPU-side checks of the activations TFNAS_ACT_RELU6 (2) and TFNAS_ACT_HSWISH (3) in the C ABI (include/tfnas_hip.h), through
ctypes as tests/test_k7_abi.py does: they are accepted only from a descriptor that carries TFNAS_CELL_ACTS, by the plan and by the
entry points; the bit changes nothing for ReLU / Swish descriptors (the planned descriptor is the same, byte for byte); every
other activation value is refused with and without it; such a cell takes the materialised route (neither E-free nor the fused
per-image route) where a ReLU / Swish cell would not; stem mode refuses them; the Python mirror sets the bit exactly when needed
and an unknown activation name is a ValueError that names the legal ones."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL = -1
RELU, SWISH, RELU6, HSWISH = 0, 1, 2, 3


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _desc(act, acts_bit, N=2, H=9, W=11, ic=24, oc=24, stride=1, mids=(32, 53), ks=(3, 5), ses=(0, 24), need_wgrad=0, flags=0,
          mode=0):
    from tfnas_amd import _lib
    d = _lib.TfnasCellDesc()
    d.flags = flags | (_lib.CELL_ACTS if acts_bit else 0)
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G = N, H, W, ic, oc, stride, act, len(mids)
    d.mode = mode
    d.has_res = int(mode == 0 and ic == oc and stride == 1)
    d.eps = 1e-5
    d.need_wgrad = need_wgrad
    for g, (m, k, s) in enumerate(zip(mids, ks, ses)):
        d.g[g].mc, d.g[g].k, d.g[g].se = m, k, s
    return d


def _bytes(d, skip=('flags',)):
    """the descriptor's bytes with the named int32 fields zeroed"""
    from tfnas_amd import _lib
    raw = bytearray(C.string_at(C.addressof(d), C.sizeof(d)))
    for f in skip:
        off = getattr(_lib.TfnasCellDesc, f).offset
        raw[off:off + 4] = b'\0\0\0\0'
    return bytes(raw)


def test_header_and_mirror_agree_and_the_abi_version_stays():
    from tfnas_amd import _lib
    src = open(HEADER).read()
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src)
    for name, val in (('RELU', 0), ('SWISH', 1), ('RELU6', 2), ('HSWISH', 3)):
        assert int(re.search(r'#define TFNAS_ACT_%s (\d+)' % name, src).group(1)) == val
    assert _lib.ACT == {'relu': 0, 'swish': 1, 'relu6': 2, 'h-swish': 3}
    bit = int(re.search(r'#define TFNAS_CELL_ACTS (0x[0-9a-fA-F]+)', src).group(1), 16)
    assert bit == _lib.CELL_ACTS and bit >= 0x100 and bit & (bit - 1) == 0
    others = [int(v, 16) for v in re.findall(r'#define TFNAS_CELL_(?!ACTS)\w+ (0x[0-9a-fA-F]+|\d+)', src)]
    assert others and not any(bit & o for o in others)
    assert 'TFNAS_ACT_RELU6 / TFNAS_ACT_HSWISH' in src.split('#define TFNAS_ABI_VERSION')[0]       # the history comment


@pytest.mark.parametrize('act', [RELU6, HSWISH])
def test_new_activations_are_opt_in(lib, act):
    """without TFNAS_CELL_ACTS: refused by the plan (as before the values existed) and -- should the bit be dropped after the
    plan -- by the entry points, before any pointer is looked at; with it they plan, at both strides, with and without weight
    gradients"""
    from tfnas_amd import _lib
    assert lib.tfnas_cell_plan(C.byref(_desc(act, False))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(act, False, flags=_lib.CELL_LAZY_JOIN | _lib.CELL_ACCUM_WGRAD | _lib.CELL_K7))) == EINVAL
    for stride in (1, 2):
        for nw in (0, 1):
            d = _desc(act, True, stride=stride, oc=24 if stride == 1 else 40, need_wgrad=nw)
            assert lib.tfnas_cell_plan(C.byref(d)) == 0, (stride, nw)
            assert (d.Ho, d.Wo) == ((9 - 1) // stride + 1, (11 - 1) // stride + 1)
    d = _desc(act, True, ks=(3, 7), flags=_lib.CELL_K7)         # both additive bits
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d = _desc(act, True)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d.flags = 0
    one = C.c_void_p(16)
    assert lib.tfnas_mixedop_fwd(C.byref(d), one, None, one, one, one, one, one, one, one, None) == EINVAL
    assert lib.tfnas_mixedop_bwd(C.byref(d), one, None, one, one, one, one, one, one, one, one, one, one, one, one, one, None,
                                 None) == EINVAL
    g1 = _desc(act, True, mids=(72,), ks=(3,), ses=(0,))
    assert lib.tfnas_cell_plan(C.byref(g1)) == 0
    g1.flags = 0
    bn = _lib.TfnasBnAffine() if hasattr(_lib, 'TfnasBnAffine') else None
    if bn is not None:
        assert lib.tfnas_mbconv_fwd(C.byref(g1), C.byref(bn), None, one, one, one, one, one, one, one, one, None) == EINVAL


@pytest.mark.parametrize('act', [RELU, SWISH])
def test_the_bit_changes_nothing_for_relu_and_swish(lib, act):
    geo = dict(N=128, H=14, W=14, ic=112, oc=112, mids=(336, 672, 336), ks=(3, 5, 5), ses=(0, 0, 112))
    for extra in (dict(), dict(need_wgrad=1), dict(stride=2, oc=192)):
        kw = dict(geo, **extra)
        a, b = _desc(act, False, **kw), _desc(act, True, **kw)
        assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
        assert a.flags == 0 and b.flags == 0x100
        assert _bytes(a) == _bytes(b)
        from tfnas_amd import _lib
        wa, wb = _lib.TfnasCellWs(), _lib.TfnasCellWs()
        assert lib.tfnas_cell_ws(C.byref(a), C.byref(wa)) == 0 and lib.tfnas_cell_ws(C.byref(b), C.byref(wb)) == 0
        assert bytes(wa) == bytes(wb)
        for fn in (lib.tfnas_efree_supported, lib.tfnas_fx_supported, lib.tfnas_cell_route):
            assert fn(C.byref(a)) == fn(C.byref(b))


@pytest.mark.parametrize('act', [4, -1, 7, 256])
@pytest.mark.parametrize('bit', [False, True])
def test_every_other_activation_value_is_refused(lib, act, bit):
    assert lib.tfnas_cell_plan(C.byref(_desc(act, bit))) == EINVAL
    d = _desc(SWISH, bit)
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d.act = act
    one = C.c_void_p(16)
    assert lib.tfnas_mixedop_fwd(C.byref(d), one, None, one, one, one, one, one, one, one, None) == EINVAL


@pytest.mark.parametrize('bit', [0x2, 0x4, 0x8, 0x10, 0x40, 0x200, 0x400])
def test_undefined_flag_bits_stay_refused(lib, bit):
    assert lib.tfnas_cell_plan(C.byref(_desc(SWISH, False, flags=bit))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(HSWISH, True, flags=bit))) == EINVAL


def test_new_activation_cells_take_the_materialised_route(lib):
    """frozen weights, a 14 x 14 ic = oc = 80 cell (ReLU / Swish: the fused per-image route) and an ic = 16 stride-2 cell (E-free)"""
    from tfnas_amd import _lib
    for geo in (dict(N=8, H=14, W=14, ic=80, oc=80, stride=1, mids=(240, 480), ses=(0, 80)),
                dict(N=8, H=112, W=112, ic=16, oc=24, stride=2, mids=(48, 96), ses=(0, 16))):
        late = geo['ic'] == 80
        for act in (RELU, SWISH):
            for bit in (False, True):
                d = _desc(act, bit, **geo)
                assert lib.tfnas_cell_plan(C.byref(d)) == 0
                assert lib.tfnas_efree_supported(C.byref(d)) == 1
                assert lib.tfnas_fx_supported(C.byref(d)) == int(late)
                assert lib.tfnas_cell_route(C.byref(d)) == _lib.ROUTE_TAKEN_VALID | (_lib.ROUTE_TAKEN_FX if late else 0)
        for act in (RELU6, HSWISH):
            d = _desc(act, True, **geo)
            assert lib.tfnas_cell_plan(C.byref(d)) == 0
            assert lib.tfnas_efree_supported(C.byref(d)) == 0
            assert lib.tfnas_fx_supported(C.byref(d)) == 0
            assert lib.tfnas_cell_route(C.byref(d)) == _lib.ROUTE_TAKEN_VALID
            one = C.c_void_p(16)            # E may not be omitted: ENULL (-2) as for every cell that is not E-free
            assert lib.tfnas_mixedop_fwd(C.byref(d), one, None, None, one, one, one, one, one, one, None) == -2


def test_workspace_does_not_depend_on_the_activation(lib):
    from tfnas_amd import _lib
    geo = dict(N=4, H=14, W=14, ic=40, oc=40, mids=(120, 240, 131), ks=(3, 5, 5), ses=(0, 40, 80), need_wgrad=1)
    sizes = []
    for act in (RELU, SWISH, RELU6, HSWISH):
        d = _desc(act, True, **geo)
        assert lib.tfnas_cell_plan(C.byref(d)) == 0
        ws = _lib.TfnasCellWs()
        assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == 0
        sizes.append((d.M, d.SE, bytes(ws)))
    assert len(set(sizes)) == 1


@pytest.mark.parametrize('act', [RELU6, HSWISH])
def test_stem_mode_refuses_and_head_mode_accepts(lib, act):
    from tfnas_amd import _lib
    stem = lambda a, bit: _desc(a, bit, N=2, H=0, W=0, ic=27, oc=16, mids=(32,), ks=(3,), ses=(8,), mode=_lib.MODE_STEM)  # noqa: E731
    for bit in (False, True):
        d = stem(act, bit)
        d.Hi = d.Wi = 32
        assert lib.tfnas_cell_plan(C.byref(d)) == EINVAL
    d = stem(RELU, True)
    d.Hi = d.Wi = 32
    assert lib.tfnas_cell_plan(C.byref(d)) == 0
    d.act = act                                   # (changed after the plan: the entry point refuses)
    one = C.c_void_p(16)
    assert lib.tfnas_mixedop_fwd(C.byref(d), one, None, one, one, one, one, one, one, one, None) == EINVAL
    head = lambda bit: _desc(act, bit, N=2, H=7, W=7, ic=320, oc=4, mids=(1280,), ks=(3,), ses=(0,), mode=_lib.MODE_HEAD)  # noqa: E731
    assert lib.tfnas_cell_plan(C.byref(head(False))) == EINVAL
    h = head(True)
    assert lib.tfnas_cell_plan(C.byref(h)) == 0
    h.flags = 0
    assert lib.tfnas_head_fwd(C.byref(h), one, one, one, one, one, None) == EINVAL
    assert lib.tfnas_head_bwd(C.byref(h), one, one, one, one, one, one, one, one, one, one, None) == EINVAL


def test_python_mirror_sets_the_bit_exactly_when_needed():
    from tfnas_amd import _lib, functions as F
    for act, want in ((RELU, 0), (SWISH, 0), (RELU6, _lib.CELL_ACTS), (HSWISH, _lib.CELL_ACTS)):
        d = _desc(act, False)
        F.HipModes().apply(d)
        assert d.flags == want
        F.HipModes(lazy_join=True).apply(d)
        assert d.flags == want | _lib.CELL_LAZY_JOIN
        d7 = _desc(act, False, ks=(3, 7))
        F.HipModes().apply(d7)
        assert d7.flags == want | _lib.CELL_K7
        assert _lib.act_flags(act) == want


def test_unknown_activation_names_raise_value_error():
    from tfnas_amd import _lib
    from tfnas_amd.layers import MBInvertedResBlock
    from tfnas_amd.functions import CellPlan
    for bad in ('gelu', 'hswish', 'ReLU6', None):
        with pytest.raises(ValueError) as ei:
            _lib.act_id(bad)
        for name in ('relu', 'relu6', 'swish', 'h-swish'):
            assert repr(name) in str(ei.value)
    with pytest.raises(ValueError):
        MBInvertedResBlock(16, 48, 0, 16, 3, 1, affine=False, act_func='gelu')
    blk = MBInvertedResBlock(16, 48, 0, 16, 3, 1, affine=False, act_func='relu6')
    with pytest.raises(ValueError):
        CellPlan(16, 16, 1, 'h_swish', [blk]).desc(2, 8, 8)


def test_modules_accept_the_reference_spellings(lib):
    """MBInvertedResBlock (both forms), MixedOP, MixedStage, NetworkCfg / config() and the latency key carry the strings; a
    CellPlan of such a block plans with the bit set (no GPU needed for the plan)"""
    from collections import OrderedDict
    from tfnas_amd import _lib, model_eval as me, model_search as ms
    from tfnas_amd.functions import CellPlan
    from tfnas_amd.layers import MBInvertedResBlock
    import _acts
    for act in _acts.NEW_ACTS:
        for affine in (False, True):
            blk = MBInvertedResBlock(24, 72, 24, 24, 5, 1, affine=affine, act_func=act)
            assert blk.act_func == act
            d, ws = CellPlan(24, 24, 1, act, [blk]).desc(2, 10, 12)
            assert d.act == _lib.ACT[act] and d.flags & _lib.CELL_ACTS and ws.E > 0
        mc = OrderedDict((i, 30 + 6 * i) for i in range(8))
        lut = {'MBInvertedResBlock_10_24_%d_24_k%d_s1_%s' % (se, k, act): {m: 0.5 + 0.01 * m for m in mc.values()}
               for se in (0, 24, 48) for k in (3, 5)}
        op = ms.MixedOP(24, 24, 1, False, act, 8, mc, lut)
        assert [b.act_func for b in op.m_ops] == [act] * 8
        assert op.get_lookup_latency(10) == [0.5 + 0.01 * m for m in mc.values()]
    cfg, _, _ = _acts.act_network_config(10)
    cfg['feature_mix_layer']['act_func'] = 'h-swish'
    net = me.NetworkCfg(10, cfg, None, 0.0, 0.0)
    assert net.config == cfg
    acts = [b.act_func for st in net._stages() for b in st]
    assert acts == [_acts.NEW_ACTS[i % 2] for i in range(len(acts))] and net.feature_mix_layer.act_func == 'h-swish'


def test_ragged_head_widths_are_refused(lib):
    """TFNAS_MODE_HEAD moves the [N][mc] rows of pooled / dpooled in quads (k_head_pool, k_head_bwd): a width that is no multiple
    of 4 would store over the next image's row and past the buffer, so the plan and every head entry point refuse it (the entry
    points before any pointer is looked at -- nothing is launched here).  Cell and stem descriptors plan exactly as before."""
    from tfnas_amd import _lib
    head = lambda mc: _desc(SWISH, False, N=2, H=7, W=7, ic=320, oc=4, mids=(mc,), ks=(3,), ses=(0,), mode=_lib.MODE_HEAD)  # noqa: E731
    one = C.c_void_p(16)
    bn = _lib.TfnasBnAffine()
    for mc in (1281, 1282, 1283):
        assert lib.tfnas_cell_plan(C.byref(head(mc))) == EINVAL, mc
        h = head(1280)
        assert lib.tfnas_cell_plan(C.byref(h)) == 0
        h.g[0].mc = mc                                # (changed after the plan: the entry points refuse)
        assert lib.tfnas_head_fwd(C.byref(h), one, one, one, one, one, None) == EINVAL
        assert lib.tfnas_head_bwd(C.byref(h), one, one, one, one, one, one, one, one, one, one, None) == EINVAL
        assert lib.tfnas_head_wgrad(C.byref(h), one, one, one, one, one, None) == EINVAL
        assert lib.tfnas_head_affine_fwd(C.byref(h), C.byref(bn), one, one, one, one, one, None) == EINVAL
        assert lib.tfnas_head_affine_bwd(C.byref(h), C.byref(bn), one, one, one, one, one, one, one, one, one, one, None) == EINVAL
    for mc in (1280, 1284, 192, 4):
        h = head(mc)
        assert lib.tfnas_cell_plan(C.byref(h)) == 0, mc
        assert h.g[0].mcp == mc and h.M >= mc
    # ragged mid widths stay legal everywhere else: a cell (one group, several groups) and the stem plan as they always did
    for mids, ks, ses in (((1281,), (3,), (0,)), ((53, 131), (3, 5), (0, 24))):
        d = _desc(SWISH, False, mids=mids, ks=ks, ses=ses)
        assert lib.tfnas_cell_plan(C.byref(d)) == 0
        assert [d.g[g].mcp for g in range(len(mids))] == [(m + 3) & ~3 for m in mids]
    stem = _desc(RELU, False, N=2, H=0, W=0, ic=27, oc=16, mids=(32,), ks=(3,), ses=(8,), mode=_lib.MODE_STEM)
    stem.Hi = stem.Wi = 32
    assert lib.tfnas_cell_plan(C.byref(stem)) == 0 and (stem.H, stem.W, stem.g[0].mcp) == (16, 16, 32)
