"""CPU-side checks of the squeeze-excite style word (TfnasCellDesc.se_style, TFNAS_CELL_SE_STYLE) in the C ABI
(include/tfnas_hip.h), through ctypes as tests/test_act_abi.py does, and of its way up through the Python layers: the encoding
rules value by value, with and without the flag, at the plan and at the entry points; the workspace and the route word do not
depend on it; CellPlan reads one style per cell; no state_dict key moves; the derived network's config carries the style only
where it is not the default."""
import copy
import ctypes as C
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL = -1
RELU, SWISH, RELU6, HSWISH = 0, 1, 2, 3
HSIG = 0x10


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _desc(style, flags, act=SWISH, mode=0, mids=(32, 53), ks=(3, 5), ses=(8, 24), N=2, H=9, W=11, ic=24, oc=24):
    from tfnas_amd import _lib
    d = _lib.TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, H, W, ic, oc, 1, act, len(mids), mode
    d.has_res, d.eps, d.flags, d.se_style = int(mode == 0 and ic == oc), 1e-5, flags, style
    if mode == 1:                                  # (a well-formed stem: ic 27, the image's extent)
        d.ic, d.Hi, d.Wi, d.has_res = 27, 2 * H, 2 * W, 0
    for g, (m, k, s) in enumerate(zip(mids, ks, ses)):
        d.g[g].mc, d.g[g].k, d.g[g].se = m, k, s
    return d


def test_header_and_mirror_agree_and_no_struct_changes_size(lib):
    from tfnas_amd import _lib
    src = open(HEADER).read()
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src) and lib.tfnas_abi_version() == 4
    bit = int(re.search(r'#define TFNAS_CELL_SE_STYLE (0x[0-9a-fA-F]+)', src).group(1), 16)
    assert bit == _lib.CELL_SE_STYLE == 0x1000
    others = [int(v, 0) for v in re.findall(r'#define TFNAS_CELL_(?!SE_STYLE)\w+ (0x[0-9a-fA-F]+|\d+)', src)]
    assert others and not any(bit & o for o in others)
    assert re.search(r'int32_t se_style;', src) and not re.search(r'int32_t pad_route;', src)
    assert re.search(r'#define TFNAS_SE_HIDDEN\(act\) \(1 \+ \(act\)\)', src) and 'TFNAS_SE_GATE_HSIGMOID' in src
    assert 'TFNAS_CELL_SE_STYLE' in src.split('#define TFNAS_ABI_VERSION')[0]                  # the history comment
    assert C.sizeof(_lib.TfnasCellDesc) == lib.tfnas_sizeof(1) and C.sizeof(_lib.TfnasGroup) == lib.tfnas_sizeof(0)
    # the word sits where the padding sat: between fwd_route and wgrad_stream
    f = _lib.TfnasCellDesc
    assert f.pad_route.offset == f.fwd_route.offset + 4 and f.wgrad_stream.offset == f.pad_route.offset + 4
    d = _lib.TfnasCellDesc()
    d.se_style = 0x11
    assert d.se_style == 0x11 == d.pad_route


# (se_style, flags beside TFNAS_CELL_SE_STYLE, return code without the flag, with it)
ACTS = 0x100
RULES = [
    (0, 0, 0, 0),                                                    # nothing asked: the flag alone changes nothing
    (1 + RELU, 0, EINVAL, 0), (1 + SWISH, 0, EINVAL, 0),             # each defined hidden activation
    (1 + RELU6, ACTS, EINVAL, 0), (1 + HSWISH, ACTS, EINVAL, 0),
    (1 + RELU6, 0, EINVAL, EINVAL), (1 + HSWISH, 0, EINVAL, EINVAL),   # ... ReLU6 / hard-swish need TFNAS_CELL_ACTS as well
    (HSIG, 0, EINVAL, 0), (HSIG | (1 + RELU), 0, EINVAL, 0), (HSIG | (1 + HSWISH), ACTS, EINVAL, 0),   # the defined gate
    (5, ACTS, EINVAL, EINVAL), (0xf, ACTS, EINVAL, EINVAL),          # undefined hidden values
    (0x20, 0, EINVAL, EINVAL), (0xf0, 0, EINVAL, EINVAL), (0x21, 0, EINVAL, EINVAL),   # undefined gates
    (0x100, 0, EINVAL, EINVAL), (0x111, 0, EINVAL, EINVAL), (1 << 30, 0, EINVAL, EINVAL), (-1, ACTS, EINVAL, EINVAL),   # high bits
]


@pytest.mark.parametrize('style,extra,without,with_', RULES, ids=lambda v: hex(v) if isinstance(v, int) else None)
def test_encoding_rules_at_the_plan_and_at_the_entry_points(lib, style, extra, without, with_):
    from tfnas_amd import _lib
    one = C.c_void_p(16)
    for flag, want in ((0, without), (_lib.CELL_SE_STYLE, with_)):
        d = _desc(style, extra | flag)
        assert lib.tfnas_cell_plan(C.byref(d)) == want, (hex(style), flag)
        # the entry points check again (the word may change after the plan): refused before any pointer is looked at
        ok = _desc(0, extra)
        assert lib.tfnas_cell_plan(C.byref(ok)) == 0
        ok.se_style, ok.flags = style, extra | flag
        if want != 0:
            assert lib.tfnas_mixedop_fwd(C.byref(ok), one, None, one, one, one, one, one, one, one, None) == EINVAL
            assert lib.tfnas_mixedop_bwd(C.byref(ok), one, None, one, one, one, one, one, one, one, one, one, one, one, one, one,
                                         None, None) == EINVAL
            g1 = _desc(0, extra, mids=(32,), ks=(3,), ses=(8,))
            assert lib.tfnas_cell_plan(C.byref(g1)) == 0
            g1.se_style, g1.flags = style, extra | flag
            bn = _lib.TfnasBnAffine()
            assert lib.tfnas_mbconv_fwd(C.byref(g1), C.byref(bn), None, one, one, one, one, one, one, one, one, None) == EINVAL
            assert lib.tfnas_mbconv_bwd(C.byref(g1), C.byref(bn), None, one, one, one, one, one, one, one, None, one, one, one,
                                        one, one, one, one, None) == EINVAL


def test_stem_and_head_refuse_a_style(lib):
    from tfnas_amd import _lib
    one = C.c_void_p(16)
    for mode, kw in ((1, dict(mids=(32,), ks=(3,), ses=(8,), oc=16, act=RELU)), (2, dict(mids=(64,), ks=(3,), ses=(0,), oc=4))):
        assert lib.tfnas_cell_plan(C.byref(_desc(0, 0, mode=mode, **kw))) == 0
        assert lib.tfnas_cell_plan(C.byref(_desc(0, _lib.CELL_SE_STYLE, mode=mode, **kw))) == 0        # (the flag alone is fine)
        for style in (1 + RELU, HSIG, HSIG | (1 + RELU)):
            assert lib.tfnas_cell_plan(C.byref(_desc(style, 0, mode=mode, **kw))) == EINVAL
            assert lib.tfnas_cell_plan(C.byref(_desc(style, _lib.CELL_SE_STYLE, mode=mode, **kw))) == EINVAL
    h = _desc(0, _lib.CELL_SE_STYLE, mode=2, mids=(64,), ks=(3,), ses=(0,), oc=4)
    assert lib.tfnas_cell_plan(C.byref(h)) == 0
    h.se_style = HSIG
    assert lib.tfnas_head_fwd(C.byref(h), one, one, one, one, one, None) == EINVAL
    assert lib.tfnas_head_bwd(C.byref(h), one, one, one, one, one, one, one, one, one, one, None) == EINVAL
    s = _desc(0, _lib.CELL_SE_STYLE, mode=1, mids=(32,), ks=(3,), ses=(8,), oc=16, act=RELU)
    assert lib.tfnas_cell_plan(C.byref(s)) == 0
    s.se_style = HSIG
    assert lib.tfnas_mixedop_fwd(C.byref(s), one, None, one, one, one, one, one, one, one, None) == EINVAL


@pytest.mark.parametrize('ses', [(8, 24), (0, 0)], ids=('se', 'no_se'))
def test_workspace_route_and_plan_do_not_depend_on_the_style(lib, ses):
    """tfnas_cell_ws field by field, tfnas_cell_route, the E-free / fused-route queries and every planned word: equal for a styled
    descriptor and its unstyled twin (a styled cell whose groups have no SE is legal)"""
    from tfnas_amd import _lib
    a, b = _desc(0, 0, ses=ses), _desc(HSIG | (1 + RELU), _lib.CELL_SE_STYLE, ses=ses)
    assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
    for need_w in (0, 1):
        a.need_wgrad = b.need_wgrad = need_w
        wa, wb = _lib.TfnasCellWs(), _lib.TfnasCellWs()
        assert lib.tfnas_cell_ws(C.byref(a), C.byref(wa)) == 0 and lib.tfnas_cell_ws(C.byref(b), C.byref(wb)) == 0
        for n, _ in wa._fields_:
            assert getattr(wa, n) == getattr(wb, n), n
        assert lib.tfnas_cell_route(C.byref(a)) == lib.tfnas_cell_route(C.byref(b)) != 0
        assert lib.tfnas_efree_supported(C.byref(a)) == lib.tfnas_efree_supported(C.byref(b))
        assert lib.tfnas_fx_supported(C.byref(a)) == lib.tfnas_fx_supported(C.byref(b))
    raw = []
    for d in (a, b):
        r = bytearray(C.string_at(C.addressof(d), C.sizeof(d)))
        for f in ('flags', 'pad_route'):
            off = getattr(_lib.TfnasCellDesc, f).offset
            r[off:off + 4] = b'\0\0\0\0'
        raw.append(bytes(r))
    assert raw[0] == raw[1]


# ------------------------------------------------------------------------------------------------ Python side (host only)
def test_se_style_id_and_its_error_messages():
    from tfnas_amd import _lib
    assert _lib.se_style_id() == _lib.se_style_id(None, 'sigmoid') == 0
    assert _lib.se_style_id('relu', 'h-sigmoid') == 0x11 and _lib.se_style_id(None, 'h-sigmoid') == 0x10
    assert [_lib.se_style_id(a, 'sigmoid') for a in ('relu', 'swish', 'relu6', 'h-swish')] == [1, 2, 3, 4]
    assert _lib.se_style_flags(0) == 0 and _lib.se_style_flags(0x11) == _lib.CELL_SE_STYLE
    assert _lib.se_style_flags(0x13) == _lib.CELL_SE_STYLE | _lib.CELL_ACTS == _lib.se_style_flags(4)
    with pytest.raises(ValueError) as e:
        _lib.se_style_id('gelu', 'sigmoid')
    assert all(repr(a) in str(e.value) for a in _lib.ACT) and 'None' in str(e.value) and "'gelu'" in str(e.value)
    with pytest.raises(ValueError) as e:
        _lib.se_style_id('relu', 'hard-sigmoid')
    assert "'sigmoid'" in str(e.value) and "'h-sigmoid'" in str(e.value) and "'hard-sigmoid'" in str(e.value)
    for bad in (0, ['relu'], ('relu',)):
        with pytest.raises(ValueError):
            _lib.se_style_id(bad, 'sigmoid')
    with pytest.raises(ValueError):
        _lib.se_style_id('relu', None)


def _block(cls_name='MBInvertedResBlock', se=8, mid=24, act='h-swish', affine=False, **kw):
    from tfnas_amd import layers
    return getattr(layers, cls_name)(8, mid, se, 8, 3, 1, affine=affine, act_func=act, **kw)


def test_blocks_take_the_style_keyword_only_and_keep_their_state_dict():
    import torch
    for cls in ('MBInvertedResBlock', 'FusedMBConvBlock'):
        for affine in (False, True):
            torch.manual_seed(0)
            a = _block(cls, affine=affine)
            torch.manual_seed(0)
            b = _block(cls, affine=affine, se_act='relu', se_gate='h-sigmoid')
            assert (a.se_act, a.se_gate) == (None, 'sigmoid') and (b.se_act, b.se_gate) == ('relu', 'h-sigmoid')
            sa, sb = a.state_dict(), b.state_dict()
            assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
            assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
        with pytest.raises(TypeError):
            from tfnas_amd import layers
            getattr(layers, cls)(8, 24, 8, 8, 3, 1, False, 'h-swish', 'relu')       # positional after act_func: keyword-only
        with pytest.raises(ValueError):
            _block(cls, se_gate='hard')
        with pytest.raises(ValueError):
            _block(cls, se_act='gelu')


def test_cell_plan_reads_one_style_per_cell(lib):
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan
    mn = dict(se_act='relu', se_gate='h-sigmoid')
    plan = CellPlan(8, 8, 1, 'h-swish', [_block(**mn)])
    d, _ = plan.desc(2, 7, 9)
    assert plan.se_style == d.se_style == 0x11 and d.flags & _lib.CELL_SE_STYLE and d.flags & _lib.CELL_ACTS
    d, _ = plan.desc(2, 7, 9)                        # (the cached descriptor keeps it when the model's modes are re-applied)
    assert d.se_style == 0x11 and d.flags & _lib.CELL_SE_STYLE
    plain = CellPlan(8, 8, 1, 'h-swish', [_block()])
    d0, _ = plain.desc(2, 7, 9)
    assert d0.se_style == 0 and not d0.flags & _lib.CELL_SE_STYLE
    # an explicit ReLU6 hidden layer in a ReLU cell brings TFNAS_CELL_ACTS with it
    d6, _ = CellPlan(8, 8, 1, 'relu', [_block(act='relu', se_act='relu6')]).desc(2, 7, 9)
    assert d6.se_style == 3 and d6.flags & _lib.CELL_ACTS and d6.flags & _lib.CELL_SE_STYLE
    # two SE blocks of different styles: one style per cell
    with pytest.raises(ValueError) as e:
        CellPlan(8, 8, 1, 'h-swish', [_block(**mn), _block(mid=32)])
    assert 'style' in str(e.value)
    with pytest.raises(ValueError):
        CellPlan(8, 8, 1, 'h-swish', [_block(**mn), _block('FusedMBConvBlock', se_gate='h-sigmoid')], mixed_kinds=True)
    # blocks without SE never conflict, whatever they say
    mixed = CellPlan(8, 8, 1, 'h-swish', [_block(**mn), _block(se=0, mid=32), _block(se=0, mid=40, se_act='swish'),
                                          _block('FusedMBConvBlock', **mn)], mixed_kinds=True)
    assert mixed.se_style == 0x11 and mixed.desc(2, 7, 9)[0].se_style == 0x11
    none = CellPlan(8, 8, 1, 'h-swish', [_block(se=0, **mn), _block(se=0, mid=32)])
    assert none.se_style == 0 and none.desc(2, 7, 9)[0].se_style == 0


def test_search_modules_take_the_style_and_keep_their_state_dict():
    from tfnas_amd import geometry, model_search as ms
    import _kinds
    lut = _kinds.AnyLut()
    lut['base'] = 0.0
    mc = geometry.initial_mc_num_dddict()
    mn = ('relu', 'h-sigmoid')
    op = ms.MixedOP(24, 24, 1, False, 'swish', 8, mc['stage1']['block2'], lut, se_style=mn)
    assert all((b.se_act, b.se_gate) == mn for b in op.m_ops) and op.se_style == mn
    assert op._plan(tuple(range(8))).se_style == 0x11 and op._plan((0,)).se_style == 0 and op._plan((5,)).se_style == 0x11
    st = ms.MixedStage([16, 24], [24, 24], [2, 1], [False] * 2, ['relu'] * 2, mc['stage1'], lut, 1, se_style={'block2': mn})
    assert st.block1.m_ops[4].se_gate == 'sigmoid' and st.block2.m_ops[4].se_gate == 'h-sigmoid'
    base = ms.Network(10, mc, lut)
    net = ms.Network(10, mc, lut, se_style={n: mn for n in ('stage2', 'stage3', 'stage4', 'stage5', 'stage6')})
    one = ms.Network(10, mc, lut, se_style=mn)
    assert list(base.state_dict()) == list(net.state_dict()) == list(one.state_dict())
    assert all(b.se_gate == 'sigmoid' for c in net.stage1.blocks() for b in c.m_ops)
    assert all((b.se_act, b.se_gate) == mn for s in net.stages()[1:] for c in s.blocks() for b in c.m_ops)
    assert all((b.se_act, b.se_gate) == mn for c in one.cells() for b in c.m_ops)
    assert (one.second_stem.se_act, one.second_stem.se_gate) == (None, 'sigmoid')     # the stems keep the reference's SE
    assert all(b.se_gate == 'sigmoid' for c in base.cells() for b in c.m_ops)
    assert ms.OPS['MBI_k3_e3_se'](8, 24, 8, 1, False, 'relu').se_gate == 'sigmoid'
    for bad in ('relu', ('relu',), ('relu', 'hard')):
        with pytest.raises(ValueError):
            ms.MixedOP(24, 24, 1, False, 'swish', 8, mc['stage1']['block2'], lut, se_style=bad)


def _arch():
    from collections import OrderedDict
    from tfnas_amd import geometry as g
    return OrderedDict((st, OrderedDict((b, (i * 3 + j + 4) % 8) for j, b in enumerate(bl) if j < 2))
                       for i, (st, bl) in enumerate(g.initial_mc_num_dddict().items()))


def test_derived_config_round_trip():
    from tfnas_amd import geometry, model_eval, parsing
    mc, arch = geometry.initial_mc_num_dddict(), _arch()
    mn = ('relu', 'h-sigmoid')
    plain = parsing.derived_config(arch, mc, 20)
    assert parsing.derived_config(arch, mc, 20, se_style=None) == plain
    assert json.dumps(parsing.derived_config(arch, mc, 20, se_style=(None, 'sigmoid'))) == json.dumps(plain)     # byte-equal
    assert not any('se_act' in b or 'se_gate' in b for s in range(1, 7) for b in plain['stage%d' % s])
    style = {'stage%d' % s: mn for s in range(2, 7)}
    cfg = parsing.derived_config(arch, mc, 20, se_style=style)
    assert all('se_act' not in b and 'se_gate' not in b for b in cfg['stage1'])
    assert all(b['se_act'] == 'relu' and b['se_gate'] == 'h-sigmoid' for s in range(2, 7) for b in cfg['stage%d' % s])
    assert 'se_act' not in cfg['second_stem'] and 'se_gate' not in cfg['second_stem']
    half = parsing.derived_config(arch, mc, 20, se_style=(None, 'h-sigmoid'))
    assert all('se_act' not in b and b['se_gate'] == 'h-sigmoid' for b in half['stage3'])
    stripped = copy.deepcopy(cfg)
    for s in range(1, 7):
        for b in stripped['stage%d' % s]:
            b.pop('se_act', None), b.pop('se_gate', None)
    assert stripped == plain
    # NetworkCfg reads the keys and writes them back; Network(se_style=...) builds the same network
    n1 = model_eval.NetworkCfg(20, cfg)
    assert n1.config == cfg and json.loads(json.dumps(n1.config)) == cfg
    assert model_eval.NetworkCfg(20, plain).config == plain
    n2 = model_eval.Network(20, arch, mc, se_style=style)
    assert n2.config == cfg and list(n1.state_dict()) == list(n2.state_dict()) == list(model_eval.Network(20, arch, mc).state_dict())
    assert all((b.se_act, b.se_gate) == mn for b in n2.stage4) and n2.stage1[0].se_gate == 'sigmoid'
    assert model_eval.Network(20, arch, mc).config == plain
    bad = copy.deepcopy(cfg)
    bad['second_stem']['se_gate'] = 'h-sigmoid'       # the stem keeps the reference's SE
    with pytest.raises(NotImplementedError):
        model_eval.NetworkCfg(20, bad)
    bad = copy.deepcopy(cfg)
    bad['stage3'][0]['se_gate'] = 'hard'
    with pytest.raises(ValueError):
        model_eval.NetworkCfg(20, bad)


def test_parse_searched_model_exports_the_models_style():
    from tfnas_amd import geometry, model_search as ms, parsing
    import _kinds
    lut = _kinds.AnyLut()
    lut['base'] = 0.0
    mn = ('relu', 'h-sigmoid')
    net = ms.Network(10, geometry.initial_mc_num_dddict(), lut, se_style={'stage5': mn})
    out = parsing.parse_searched_model(net, num_classes=10)
    assert all(b.get('se_gate') == 'h-sigmoid' and b.get('se_act') == 'relu' for b in out['config']['stage5'])
    assert not any('se_gate' in b for s in (1, 2, 3, 4, 6) for b in out['config']['stage%d' % s])
