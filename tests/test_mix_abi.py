"""CPU-side checks of MixConv groups in the C ABI (include/tfnas_hip.h: a packed TfnasGroup.k, read as such only from a descriptor
that carries TFNAS_CELL_MIXK), through ctypes as tests/test_dil_abi.py does, and of the Python layers above it: the plan accepts
the four legal words at both strides from a caller that set the bit; without the bit a packed word is refused as every k above 7
always was; with the bit an unpacked descriptor plans, sizes and routes identically (the 18 cells at B = 128); every refusal of the
header; the workspace and every planned word are those of the same group with a plain k; the partial-row limit counts the packed
layout; the segment boundaries the plan implies are those of the header's rule (computed here on their own); a packed cell takes
the materialised route where its plain twin is E-free or fused; the entry points re-check a descriptor changed after its plan;
HipModes.apply sets the bit for packed descriptors only; the registry, the config export and NetworkCfg, the latency key."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL, ERANGE = -1, -3
LEGAL = (0x53, 0x73, 0x75, 0x753)


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _desc(N=2, H=9, W=11, ic=24, oc=24, stride=1, mids=(44, 53), ks=(0x53, 0x753), dils=None, ses=(0, 24), need_wgrad=0, act=1,
          flags=None, mode=0, kinds=None):
    from tfnas_amd import _lib
    d = _lib.TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, H, W, ic, oc, stride, act, len(mids), mode
    d.has_res = int(mode == 0 and ic == oc and stride == 1)
    d.eps = 1e-5
    d.need_wgrad = need_wgrad
    for g, (m, k, s) in enumerate(zip(mids, ks, ses)):
        d.g[g].mc, d.g[g].k, d.g[g].se = m, k, s
        if dils is not None:
            d.g[g].dil = dils[g]
        if kinds is not None:
            d.g[g].kind = kinds[g]
    has7 = any(k == 7 or (k > 0xf and 7 in ((k >> 4) & 0xf, (k >> 8) & 0xf)) for k in ks)
    d.flags = (_lib.CELL_MIXK | (_lib.CELL_K7 if has7 else 0) | _lib.act_flags(act)
               | (_lib.CELL_DILATION if dils is not None else 0)) if flags is None else flags
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


def _kmax(k):
    return max(k & 0xf, (k >> 4) & 0xf, (k >> 8) & 0xf)


def test_header_and_mirror_agree_and_the_abi_version_stays(lib):
    from tfnas_amd import _lib
    src = open(HEADER).read()
    m = re.search(r'#define TFNAS_CELL_MIXK (0x[0-9a-fA-F]+)', src)
    assert m and int(m.group(1), 16) == _lib.CELL_MIXK == 0x10000
    assert not re.search(r'#define TFNAS_\w+ 0x4000\b', src)          # (0x4000 stays undefined: refused below)
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src) and lib.tfnas_abi_version() == 4
    body = re.search(r'typedef struct TfnasGroup \{(.*?)\} TfnasGroup;', src, re.S).group(1)
    words = re.findall(r'int32_t (\w+);', body)
    assert words == [n for n, t in _lib.TfnasGroup._fields_ if t is C.c_int32]             # no struct changed
    assert lib.tfnas_sizeof(0) == C.sizeof(_lib.TfnasGroup) == 8 * 4 + 14 * 8
    assert lib.tfnas_sizeof(1) == C.sizeof(_lib.TfnasCellDesc)
    assert 'TFNAS_CELL_MIXK' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert [_lib.mix_k_word(ks) for ks in _lib.MIX_KERNELS] == list(LEGAL)


@pytest.mark.parametrize('stride', [1, 2])
def test_plan_accepts_the_four_words_with_the_bit(lib, stride):
    oc = 24 if stride == 1 else 40
    for k in LEGAL:
        for other in (3, 5, 7, k):
            d = _desc(ks=(k, other), stride=stride, oc=oc)
            assert lib.tfnas_cell_plan(C.byref(d)) == 0, (hex(k), other)
            assert (d.Ho, d.Wo) == ((9 - 1) // stride + 1, (11 - 1) // stride + 1)
    for act in (0, 1, 2, 3):                                                               # all four activations
        assert lib.tfnas_cell_plan(C.byref(_desc(act=act, stride=stride, oc=oc, need_wgrad=1))) == 0
    # a plain k under the bit means what it means without it
    for k in (3, 5, 7):
        a, b = _desc(ks=(k, k), stride=stride, oc=oc), _desc(ks=(k, k), stride=stride, oc=oc, flags=_lib_k7(k))
        assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
        assert _planned(a) == _planned(b) and _ws(lib, a) == _ws(lib, b) and _queries(lib, a) == _queries(lib, b)


def _lib_k7(k):
    from tfnas_amd import _lib
    return _lib.CELL_K7 if k == 7 else 0


def test_without_the_bit_a_packed_word_is_refused(lib):
    from tfnas_amd import _lib
    for k in LEGAL:
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=(k, 3), flags=_lib.CELL_K7))) == EINVAL
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3, k), flags=0))) == EINVAL
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=(k, 3), flags=_lib.CELL_K7 | _lib.CELL_DILATION))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3, 5), flags=0))) == 0
    # ... and 0x4000, the bit between TFNAS_CELL_SKIP and TFNAS_CELL_DILATION, stays undefined and refused, with or without this one
    for ks in ((3, 5), (0x53, 3)):
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=ks, flags=0x4000))) == EINVAL
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=ks, flags=0x4000 | _lib.CELL_MIXK))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 3), flags=_lib.CELL_MIXK))) == 0


def test_with_the_bit_an_unpacked_descriptor_is_what_it_was_on_the_18_cells(lib):
    """the 18 cells of the search space at B = 128, all eight candidates, frozen weights and with weight gradients: planned words,
    tfnas_cell_ws field by field, tfnas_cell_route, tfnas_efree_supported, tfnas_fx_supported"""
    from tfnas_amd import _lib, geometry as g
    n = fx = ef = 0
    for stage, block, ic, oc, stride, act, size in g.iter_cells():
        for need_wgrad in (0, 1):
            geo = dict(N=128, H=size, W=size, ic=ic, oc=oc, stride=stride, mids=(3 * ic, 6 * ic) * 4, ks=(3, 3, 5, 5) * 2,
                       ses=(0,) * 4 + (ic, 2 * ic) * 2, act=_lib.ACT[act], need_wgrad=need_wgrad)
            a, b = _desc(flags=0, **geo), _desc(**geo)
            assert b.flags == _lib.CELL_MIXK
            assert lib.tfnas_cell_plan(C.byref(a)) == 0 and lib.tfnas_cell_plan(C.byref(b)) == 0
            assert _planned(a) == _planned(b), (stage, block)
            assert _ws(lib, a) == _ws(lib, b), (stage, block)
            assert _queries(lib, a) == _queries(lib, b), (stage, block)
            ef += _queries(lib, b)[1]
            fx += _queries(lib, b)[2]
            n += 1
    assert n == 36 and ef > 0 and fx > 0                   # (the bit alone gives up neither route)


def test_packing_changes_neither_planned_words_nor_workspace(lib):
    """tfnas_cell_ws and every planned word (M, SE, off, mcp, se_off) are what they are for the same group with a plain k"""
    for stride in (1, 2):
        for need_wgrad in (0, 1):
            for mids in ((120, 240, 131), (44, 53, 107), (9, 12, 1536)):
                geo = dict(N=4, H=14, W=14, ic=40, oc=40 if stride == 1 else 80, stride=stride, mids=mids, ses=(0, 40, 80),
                           need_wgrad=need_wgrad)
                for ks in ((0x53, 0x753, 0x75), (0x753, 0x73, 0x53)):
                    dp, du = _desc(ks=ks, **geo), _desc(ks=tuple(_kmax(k) for k in ks), **geo)
                    assert lib.tfnas_cell_plan(C.byref(dp)) == 0 and lib.tfnas_cell_plan(C.byref(du)) == 0
                    assert _planned(dp) == _planned(du) and _ws(lib, dp) == _ws(lib, du)
                    assert [dp.g[g].k for g in range(3)] == list(ks)                       # (the plan leaves the word alone)


def test_refusals(lib):
    from tfnas_amd import _lib
    assert lib.tfnas_cell_plan(C.byref(_desc())) == 0
    # any other packed word: descending, repeated, garbage above, a fourth nibble, a nibble that is no kernel size, a zero nibble
    for bad in (0x35, 0x33, 0x55, 0x357, 0x7531, 0x1753, 0x50005, 0x10053, 0x1000 | 0x753, 0x93, 0x51, 0x503, 0x530, 0x13, 0x57,
                0x37, 0x735, 0x775, 0x553, 0x40000053, -0x53, 0x5 | (1 << 20), 9, 1, 4, 0x10):
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=(bad, 3), flags=_lib.CELL_MIXK | _lib.CELL_K7))) == EINVAL, hex(bad)
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, bad), flags=_lib.CELL_MIXK | _lib.CELL_K7))) == EINVAL, hex(bad)
    # a 7 without TFNAS_CELL_K7
    for k in (0x73, 0x75, 0x753):
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=(k, 3), flags=_lib.CELL_MIXK))) == EINVAL
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=(k, 3), flags=_lib.CELL_MIXK | _lib.CELL_K7))) == 0
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 7), flags=_lib.CELL_MIXK))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 5), flags=_lib.CELL_MIXK))) == 0
    # q < n: a segment without a channel quad; q == n is the narrowest legal group
    for mc, k, want in ((8, 0x753, EINVAL), (5, 0x753, EINVAL), (9, 0x753, 0), (12, 0x753, 0), (4, 0x53, EINVAL), (1, 0x75, EINVAL),
                        (5, 0x53, 0), (8, 0x73, 0)):
        d = _desc(ic=4, oc=4, mids=(mc,), ks=(k,), ses=(0,))
        assert lib.tfnas_cell_plan(C.byref(d)) == want, (mc, hex(k))
        if want == 0:
            assert d.g[0].mcp == (mc + 3) // 4 * 4
    # packed + dil == 2 in the same group; beside a dilated group it is fine
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 3), dils=(2, 0)))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3, 0x753), dils=(0, 2)))) == EINVAL
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 3), dils=(0, 2)))) == 0
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 5), dils=(1, 2)))) == 0
    # kinds: a packed FUSED or SKIP group; plain and expand-free groups are allowed
    K = _lib.CELL_KINDS | _lib.CELL_MIXK | _lib.CELL_K7
    M, N_, F_, S = 0, 1, 2, _lib.GROUP_SKIP
    kinds_geo = dict(ic=24, oc=24, mids=(32, 24, 40), ses=(0, 0, 0))
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 0x753, 3), flags=K, kinds=(M, N_, F_), **kinds_geo))) == 0
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3, 5, 0x53), flags=K, kinds=(M, N_, F_), **kinds_geo))) == EINVAL      # a packed FUSED group
    skip_geo = dict(ic=24, oc=24, mids=(32, 0), ses=(0, 0))
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 0), flags=K | _lib.CELL_SKIP, kinds=(M, S), **skip_geo))) == 0
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53, 0x53), flags=K | _lib.CELL_SKIP, kinds=(M, S), **skip_geo))) == EINVAL   # a packed SKIP group
    one = dict(ic=24, oc=24, mids=(40,), ses=(0,))
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(3,), flags=_lib.CELL_FUSED | _lib.CELL_MIXK, **one))) == 0
    assert lib.tfnas_cell_plan(C.byref(_desc(ks=(0x53,), flags=_lib.CELL_FUSED | _lib.CELL_MIXK, **one))) == EINVAL      # a packed FUSED cell
    noexp = dict(ic=24, oc=24, mids=(24,), ses=(24,))
    for k in LEGAL:                                                                        # expand-free: allowed
        assert lib.tfnas_cell_plan(C.byref(_desc(ks=(k,), flags=_lib.CELL_NOEXPAND | _lib.CELL_MIXK | _lib.CELL_K7, **noexp))) == 0
    stem = dict(ic=27, oc=16, mids=(32,), ses=(8,), act=0, mode=_lib.MODE_STEM)
    for k, want in ((3, 0), (0x53, EINVAL)):                                               # stem and head mode
        d = _desc(ks=(k,), **stem)
        d.Hi, d.Wi = 18, 26
        assert lib.tfnas_cell_plan(C.byref(d)) == want
        h = _desc(ic=320, oc=320, mids=(1280,), ks=(k,), ses=(0,), mode=_lib.MODE_HEAD)
        assert lib.tfnas_cell_plan(C.byref(h)) == want


def test_partial_row_limit_counts_the_packed_layout(lib):
    """TFNAS_ERANGE when sum over groups of sum_s mc_s k_s^2 is over the partial-row limit: eight 0x753 groups of 1536 channels
    are 8 * 512 * (9 + 25 + 49) = 339 968 floats and fit, as eight plain 7 x 7 groups (602 112) do; the limit itself is found with
    plain 7 x 7 groups of the widest legal oc-independent width, and packed groups of the same width pass it where their
    k_max twins do not"""
    geo = dict(N=2, H=7, W=7, ic=16, oc=16, need_wgrad=1)

    def rc(mids, ks):
        return lib.tfnas_cell_plan(C.byref(_desc(mids=mids, ks=ks, ses=(0,) * len(mids), **geo)))
    assert rc((1536,) * 8, (0x753,) * 8) == 0 and rc((1536,) * 8, (7,) * 8) == 0
    # find a width at which eight plain 7 x 7 groups no longer fit (doubling), then bisect the limit L in floats
    w = 1536
    while rc((w,) * 8, (7,) * 8) == 0:
        w *= 2
        assert w < (1 << 24)
    assert rc((w,) * 8, (7,) * 8) == ERANGE
    lo, hi = w // 2, w                       # rc(lo) == 0, rc(hi) == ERANGE
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rc((mid,) * 8, (7,) * 8) == 0:
            lo = mid
        else:
            hi = mid
    limit_lo, limit_hi = 8 * lo * 49, 8 * hi * 49          # limit_lo <= L < limit_hi

    def packed_floats(mc, k):
        ks = [(k >> (4 * s)) & 0xf for s in range(3) if (k >> (4 * s)) & 0xf]
        q, n = (mc + 3) // 4, len(ks)
        ends = [min(4 * ((s + 1) * (q // n) + q % n), mc) for s in range(n)]
        return sum((e - b) * kk * kk for b, e, kk in zip([0] + ends[:-1], ends, ks))
    # packed groups of width hi (whose 7 x 7 twins are over the limit) are under it; and widening them crosses it exactly where
    # the packed count does
    assert rc((hi,) * 8, (0x753,) * 8) == 0 and 8 * packed_floats(hi, 0x753) < limit_lo
    for k in (0x753, 0x53, 0x75):
        a, b = hi, hi * 8
        assert rc((a,) * 8, (k,) * 8) == 0 and rc((b,) * 8, (k,) * 8) == ERANGE
        while b - a > 1:
            mid = (a + b) // 2
            if rc((mid,) * 8, (k,) * 8) == 0:
                a = mid
            else:
                b = mid
        assert 8 * packed_floats(a, k) < limit_hi and 8 * packed_floats(b, k) > limit_lo, hex(k)
    from tfnas_amd import _lib
    ws = _lib.TfnasCellWs()
    d = _desc(mids=(hi,) * 8, ks=(7,) * 8, ses=(0,) * 8, **geo)
    assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == ERANGE


def _rule(mc, n):
    """the header's rule, written out on its own: q = mcp / 4 quads; segment s gets q / n, segment 0 the q % n remaining ones too;
    segment s = [4 Q_s, min(4 Q_s+1, mc))"""
    mcp = (mc + 3) & ~3
    q = mcp // 4
    quads = [q // n] * n
    quads[0] += q % n
    bounds, c = [], 0
    for s in range(n):
        lo = c
        c += 4 * quads[s]
        bounds.append((lo, min(c, mc)))
    return bounds


@pytest.mark.parametrize('mc', [9, 12, 44, 53, 107, 1536])
def test_segment_boundaries(lib, mc):
    """the boundaries the plan implies -- what the Python mirror splits its packed weight by, and what the library counts its
    partial row by -- against the rule of the header, computed here independently; e.g. 53 with three segments -> 24 | 16 | 13"""
    from tfnas_amd import _lib
    from tfnas_amd.layers import MixDepthwiseConv2d
    assert [b - a for a, b in _rule(53, 3)] == [24, 16, 13] and [b - a for a, b in _rule(44, 2)] == [24, 20]
    for k in LEGAL:
        ks = [(k >> (4 * s)) & 0xf for s in range(3) if (k >> (4 * s)) & 0xf]
        n = len(ks)
        want = _rule(mc, n)
        assert want[0][0] == 0 and want[-1][1] == mc and all(a[1] == b[0] for a, b in zip(want, want[1:]))
        assert all(lo % 4 == 0 for lo, _ in want) and all(hi > lo for lo, hi in want)      # 16-byte aligned, never empty
        if mc % (4 * n) == 0:                  # MixNet's own _split_channels: equal parts, the remainder to the first
            split = [mc // n] * n
            split[0] += mc - sum(split)
            assert [hi - lo for lo, hi in want] == split
        widths = [hi - lo for lo, hi in want]
        assert _lib.mix_split(mc, n) == widths
        dw = MixDepthwiseConv2d(mc, tuple(ks))
        assert dw.splits == widths and dw.weight.numel() == sum(w * kk * kk for w, kk in zip(widths, ks))
        # the library's count of the same layout: the widest cell of such groups the partial row takes is the one this count says
        d = _desc(ic=4, oc=4, mids=(mc,), ks=(k,), ses=(0,), need_wgrad=1)
        assert lib.tfnas_cell_plan(C.byref(d)) == 0 and d.g[0].mcp == (mc + 3) // 4 * 4


def test_packed_cells_take_the_materialised_route(lib):
    from tfnas_amd import _lib
    # the geometries where the plain cell is E-free / fused (frozen weights): stride-2 ic 16 at 112 x 112, ic 112 at 14 x 14
    for geo in (dict(N=8, H=112, W=112, ic=16, oc=24, stride=2, mids=(48, 96), ses=(0, 16)),
                dict(N=8, H=14, W=14, ic=112, oc=112, stride=1, mids=(336, 672), ses=(0, 0))):
        du = _desc(ks=(3, 5), **geo)
        assert lib.tfnas_cell_plan(C.byref(du)) == 0 and lib.tfnas_efree_supported(C.byref(du)) == 1
        for ks in ((0x53, 5), (3, 0x53), (0x53, 0x53)):
            dd = _desc(ks=ks, **geo)
            assert lib.tfnas_cell_plan(C.byref(dd)) == 0
            assert _queries(lib, dd) == (_lib.ROUTE_TAKEN_VALID, 0, 0), ks
            for route in (_lib.ROUTE_DW['direct'], _lib.ROUTE_DW['lds'], _lib.ROUTE_DW['tiled'], _lib.ROUTE_DWWG_OFF):
                dd.route = route
                assert _queries(lib, dd) == (_lib.ROUTE_TAKEN_VALID, 0, 0)


def test_entry_points_recheck_a_descriptor_changed_after_its_plan(lib):
    """every entry point runs the checks of the plan again, before any pointer is looked at: a planned descriptor whose packed
    word, bits or mode were made illegal afterwards is refused"""
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
        for change in ('word', 'k7', 'dil', 'fused', 'stem', 'narrow'):
            d = _desc(mids=(53,), ks=(0x753,), ses=(24,), dils=(0,))
            assert lib.tfnas_cell_plan(C.byref(d)) == 0
            if change == 'word':
                d.g[0].k = 0x357
            elif change == 'k7':
                d.flags &= ~_lib.CELL_K7
            elif change == 'dil':
                d.g[0].dil = 2
            elif change == 'fused':
                d.flags |= _lib.CELL_FUSED
            elif change == 'stem':
                d.mode = _lib.MODE_STEM
            else:
                d.g[0].mc = 8
            assert entry(d) == EINVAL, (entry.__name__, change)


def test_python_mirror_sets_the_bit_for_packed_descriptors_only():
    from tfnas_amd import _lib, functions as F
    for ks, want in (((3, 5), 0), ((5, 5), 0), ((0x53, 5), _lib.CELL_MIXK), ((3, 0x753), _lib.CELL_MIXK | _lib.CELL_K7),
                     ((0x75, 0x53), _lib.CELL_MIXK | _lib.CELL_K7), ((7, 3), _lib.CELL_K7)):
        d = _desc(ks=ks, flags=0)
        F.HipModes().apply(d)
        assert d.flags == want, ks
        F.HipModes(lazy_join=True).apply(d)
        assert d.flags == want | _lib.CELL_LAZY_JOIN
    assert _lib.describe_block(_lib.MBCONV, 2, 9, 9, 16, 48, 0, 16, 3, 1, 0).flags == 0
    db = _lib.describe_block(_lib.NOEXPAND, 2, 9, 9, 16, 16, 0, 16, 7, 1, 0, 1, (3, 5, 7))
    assert db.flags == _lib.CELL_NOEXPAND | _lib.CELL_MIXK | _lib.CELL_K7 and db.g[0].k == 0x753
    db = _lib.describe_block(_lib.MBCONV, 2, 9, 9, 16, 48, 0, 16, 5, 1, 0, mix_kernels=(3, 5))
    assert db.flags == _lib.CELL_MIXK and db.g[0].k == 0x53
    for bad in ((5, 3), (3, 3), (3,), (3, 5, 7, 9), (3, 9), [3, 5.0], 'k35', 53, None):
        with pytest.raises(ValueError):
            _lib.mix_k_word(bad)


def test_cell_plan_packs_the_word(lib):
    from tfnas_amd import _lib
    from tfnas_amd.functions import CellPlan
    from tfnas_amd.layers import MBInvertedResBlock
    blocks = [MBInvertedResBlock(16, 40, 8, 24, stride=2, mix_kernels=(3, 5)), MBInvertedResBlock(16, 52, 0, 24, 5, 2),
              MBInvertedResBlock(16, 44, 0, 24, 3, 2, mix_kernels=(3, 5, 7))]
    d, _ = CellPlan(16, 24, 2, 'relu', blocks).desc(2, 9, 13)
    assert [d.g[g].k for g in range(3)] == [0x53, 5, 0x753] and d.flags == _lib.CELL_MIXK | _lib.CELL_K7
    d, _ = CellPlan(16, 24, 2, 'relu', blocks[1:2]).desc(2, 9, 13)
    assert d.g[0].k == 5 and d.flags == 0
    d, _ = CellPlan(16, 16, 1, 'swish', [MBInvertedResBlock(16, 16, 16, 16, stride=1, mix_kernels=(3, 5))]).desc(2, 9, 13)
    assert d.flags == _lib.CELL_NOEXPAND | _lib.CELL_MIXK and d.g[0].k == 0x53


def test_block_argument():
    import torch
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock, MixDepthwiseConv2d
    plain = MBInvertedResBlock(16, 53, 8, 24, 7, 2, affine=True)
    mix = MBInvertedResBlock(16, 53, 8, 24, 3, 2, affine=True, mix_kernels=(3, 5, 7))
    assert plain.mix_kernels is None and mix.mix_kernels == (3, 5, 7) and mix.kernel_size == 7 and mix.dilation == 1
    c = mix.depth_conv.conv
    assert isinstance(c, MixDepthwiseConv2d) and isinstance(plain.depth_conv.conv, torch.nn.Conv2d)
    assert tuple(c.weight.shape) == (24 * 9 + 16 * 25 + 13 * 49,) and c.splits == [24, 16, 13] and c.bias is None
    assert [tuple(w.shape) for w in c.segment_weights()] == [(24, 1, 3, 3), (16, 1, 5, 5), (13, 1, 7, 7)]
    assert all(w.data_ptr() == c.weight.data_ptr() + 4 * o for w, o in zip(c.segment_weights(), (0, 216, 616)))     # views
    assert list(plain.state_dict()) == list(mix.state_dict())
    same = [k for k in plain.state_dict() if k != 'depth_conv.conv.weight']
    assert all(plain.state_dict()[k].shape == mix.state_dict()[k].shape for k in same)
    y = c(torch.zeros(1, 53, 9, 13))
    assert tuple(y.shape) == (1, 53, 5, 7)                                                 # (H - 1) / stride + 1
    # a block without mix_kernels is what it was, down to every key and module
    again = MBInvertedResBlock(16, 53, 8, 24, 7, 2, affine=True, mix_kernels=None)
    assert list(again.state_dict()) == list(plain.state_dict()) and [type(m) for m in again.modules()] == [type(m) for m in plain.modules()]
    assert [tuple(v.shape) for v in again.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
    for bad in ((5, 3), (3, 3), (3,), (3, 5, 7, 9), (3, 9), 35, 'k35', (3.0, 5)):
        with pytest.raises(ValueError):
            MBInvertedResBlock(16, 48, 8, 24, 3, 1, mix_kernels=bad)
    with pytest.raises(ValueError, match='dilation'):
        MBInvertedResBlock(16, 48, 8, 24, 5, 1, dilation=2, mix_kernels=(3, 5))
    with pytest.raises(ValueError, match='too few'):
        MBInvertedResBlock(4, 8, 0, 4, mix_kernels=(3, 5, 7))
    with pytest.raises(TypeError):
        MBInvertedResBlock(16, 48, 8, 24, 3, 1, False, 'relu', None, 'sigmoid', 1, (3, 5))      # keyword-only
    with pytest.raises(TypeError):
        FusedMBConvBlock(16, 48, 8, 24, 3, 1, mix_kernels=(3, 5))


def test_registry_and_primitives(lib):
    from tfnas_amd import _lib, model_search as ms, geometry as g
    new = ['MBI_k35_e3', 'MBI_k35_e6', 'MBI_k357_e3', 'MBI_k357_e6', 'MBI_k35_e3_se', 'MBI_k35_e6_se', 'MBI_k357_e3_se',
           'MBI_k357_e6_se', 'DS_k35', 'DS_k357', 'DS_k35_se', 'DS_k357_se']
    assert sorted(ms.MIX_OPS) == sorted(new) == sorted(g.PRIMITIVE_MIX)
    assert not set(new) & set(ms.OPS) and not set(new) & set(ms.DILATED_OPS)
    old = ['FMB_k3_e3', 'FMB_k3_e6', 'FMB_k3_e3_se', 'FMB_k3_e6_se', 'DS_k3', 'DS_k5', 'DS_k3_se', 'DS_k5_se',
           'MBI_k7_e3', 'MBI_k7_e6', 'MBI_k7_e3_se', 'MBI_k7_e6_se']
    assert sorted(ms.OPS) == sorted(ms.PRIMITIVES + old)                                   # OPS is what it was
    assert sorted(ms.DILATED_OPS) == sorted(g.PRIMITIVE_DILATION) and len(ms.DILATED_OPS) == 12      # ... and DILATED_OPS
    want = {'MBI_k35_e3': (_lib.MBCONV, (3, 5), 48, 0), 'MBI_k35_e6_se': (_lib.MBCONV, (3, 5), 48, 32),
            'MBI_k357_e3_se': (_lib.MBCONV, (3, 5, 7), 48, 16), 'MBI_k357_e6': (_lib.MBCONV, (3, 5, 7), 48, 0),
            'DS_k35': (_lib.NOEXPAND, (3, 5), 16, 0), 'DS_k357_se': (_lib.NOEXPAND, (3, 5, 7), 16, 16)}
    for name, (kind, ks, mid, se) in want.items():
        b = ms.MIX_OPS[name](16, 48, 24, 2, False, 'swish')
        assert ms.primitive_factory(name) is ms.MIX_OPS[name]
        assert (b.kind, b.kernel_size, b.mid_channels, b.se_channels, b.stride, b.out_channels, b.mix_kernels) == (
            kind, max(ks), mid, se, 2, 24, ks)
        layer, mc, se_, k_ = g.primitive_block(name, 16, 48)                                # still four words
        assert (layer, mc, se_, k_) == ('MBInvertedResBlock', mid, se, max(ks)) and g.primitive_mix_kernels(name) == ks
        assert g.primitive_dilation(name) == 1
    for name in list(ms.OPS) + list(ms.DILATED_OPS) + [g.SKIP]:
        assert g.primitive_mix_kernels(name) is None
    with pytest.raises(ValueError):
        g.primitive_mix_kernels('MBI_k37_e3')
    mc = dict(enumerate([48, 96, 48, 96, 48, 96, 48, 96]))
    names = ['MBI_k3_e3', 'MBI_k35_e6', 'MBI_k357_e3', 'MBI_k5_e6', 'MBI_k35_e3_se', 'MBI_k3_e6_se', 'MBI_k5_e3_se', 'MBI_k357_e6_se']
    assert ms.check_primitives(names) == names
    op = ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {}, primitives=names)
    assert [b.mix_kernels for b in op.m_ops] == [None, (3, 5), (3, 5, 7), None, (3, 5), None, None, (3, 5, 7)]
    assert all(b.kind is _lib.MBCONV for b in op.m_ops)
    d, _ = op._plan(tuple(range(8))).desc(2, 9, 13)
    assert [d.g[i].k for i in range(8)] == [3, 0x53, 0x753, 5, 0x53, 3, 5, 0x753] and d.flags == _lib.CELL_MIXK | _lib.CELL_K7
    assert op._plan((1,)).desc(2, 9, 13)[0].flags == _lib.CELL_MIXK and op._plan((0,)).desc(2, 9, 13)[0].flags == 0
    default = ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {})
    assert list(default.state_dict()) == list(op.state_dict())
    assert default._plan(tuple(range(8))).desc(2, 9, 13)[0].flags == 0
    ds = ms.MixedOP(16, 16, 1, False, 'swish', 8, mc, {}, primitives=names[:7] + ['DS_k35'])
    assert ds.m_ops[7].kind is _lib.NOEXPAND and ds._plan(tuple(range(8))).group_kinds is not None
    with pytest.raises(ValueError, match='DS_k35.*MBI_k357_e3'):
        ms.MixedOP(16, 24, 2, False, 'swish', 8, mc, {}, primitives=names[:7] + ['MBI_k37_e3'])


def test_network_with_a_mixconv_candidate_is_not_plain(lib):
    from tfnas_amd import model_search as ms, geometry as g
    mcs = g.initial_mc_num_dddict()
    names = list(g.PRIMITIVES)
    names[3] = 'MBI_k35_e6'
    ref = ms.Network(10, mcs, {})
    assert ref.plain_candidates()
    one = ms.Network(10, mcs, {}, primitives={'stage3': {'block2': names}})
    assert not one.plain_candidates() and list(one.state_dict()) == list(ref.state_dict())
    assert one.stage3.block2.m_ops[3].mix_kernels == (3, 5)


def test_config_export_and_networkcfg_round_trip(lib):
    from collections import OrderedDict
    from tfnas_amd import geometry as g, model_eval as me, parsing
    mcs = g.initial_mc_num_dddict()
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 2)) for i, (st, bl) in enumerate(mcs.items()))
    default = parsing.derived_config(arch, mcs, 20)
    assert not any('mix_kernels' in c for k, v in default.items() if k.startswith('stage') for c in v)
    assert 'mix_kernels' not in default['second_stem']
    assert me.NetworkCfg(20, default).config == default
    names = ['MBI_k35_e3', 'MBI_k3_e6', 'MBI_k357_e3', 'DS_k357', 'MBI_k35_e3_se', 'MBI_k3_e6_se', 'DS_k35_se', 'MBI_k357_e6_se']
    cfg = parsing.derived_config(arch, mcs, 20, primitives=names)
    got = [(c['kernel_size'], c.get('mix_kernels'), c['mid_channels'] > c['in_channels']) for k, v in sorted(cfg.items())
           if k.startswith('stage') for c in v]
    want = []
    for i, st in enumerate(mcs):
        for j in range(min(2, len(mcs[st]))):
            n = names[(i * 3 + j) % 8]
            mk = g.primitive_mix_kernels(n)
            want.append((g.primitive_block(n, 16, 48)[3], None if mk is None else list(mk), not n.startswith('DS')))
    assert got == want and any(w[1] == [3, 5] for w in want) and any(w[1] == [3, 5, 7] for w in want) and any(w[1] is None for w in want)
    # the key appears only where mixed: every other entry has exactly the keys of the default config's entries
    keys = set(default['stage1'][0])
    for k, v in cfg.items():
        if k.startswith('stage'):
            for c in v:
                assert set(c) == (keys | {'mix_kernels'} if 'mix_kernels' in c else keys)
    net = me.NetworkCfg(20, cfg)
    assert net.config == cfg                                                               # reads the key back, writes it back
    blocks = [b for st in net._stages() for b in st]
    assert [b.mix_kernels for b in blocks] == [None if w[1] is None else tuple(w[1]) for w in want]
    derived = me.Network(20, arch, mcs, primitives=names)
    assert derived.config == cfg and list(derived.state_dict()) == list(net.state_dict())
    assert [tuple(v.shape) for v in derived.state_dict().values()] == [tuple(v.shape) for v in net.state_dict().values()]
    # the state_dict keys of the network are those of the default one (the unmixed blocks' shapes too)
    assert list(me.NetworkCfg(20, default).state_dict()) == list(me.Network(20, arch, mcs).state_dict())
    # the counters count the segments: fewer depthwise taps than the k_max twin, more than the k_min twin
    hi = {k: ([{kk: vv for kk, vv in c.items() if kk != 'mix_kernels'} for c in v] if k.startswith('stage') else v) for k, v in cfg.items()}
    lo = {k: ([{kk: (min(c.get('mix_kernels', [vv])) if kk == 'kernel_size' else vv) for kk, vv in c.items() if kk != 'mix_kernels'}
               for c in v] if k.startswith('stage') else v) for k, v in cfg.items()}
    assert parsing.count_macs_in_M(lo, 64) < parsing.count_macs_in_M(cfg, 64) < parsing.count_macs_in_M(hi, 64)
    assert parsing.count_params_in_MB(lo) < parsing.count_params_in_MB(cfg) < parsing.count_params_in_MB(hi)
    n_params = sum(p.numel() for p in net.parameters())
    assert abs(parsing.count_params_in_MB(cfg) * 1e6 - n_params) < 0.5
    for bad in (dict(cfg, second_stem=dict(cfg['second_stem'], mix_kernels=[3, 5])),):
        with pytest.raises(NotImplementedError):
            me.NetworkCfg(20, bad)
    bad = {k: ([dict(c) for c in v] if k.startswith('stage') else v) for k, v in cfg.items()}
    bad['stage2'][0]['mix_kernels'] = [5, 3]
    with pytest.raises(ValueError):
        me.NetworkCfg(20, bad)


def test_lut_key_text():
    from tfnas_amd import geometry as g, model_search as ms, model_eval as me
    assert g.lut_key(14, 80, 0, 80, 3, 1, 'swish') == 'MBInvertedResBlock_14_80_0_80_k3_s1_swish'
    assert g.lut_key(14, 80, 0, 80, 5, 1, 'swish', mix_kernels=(3, 5)) == 'MBInvertedResBlock_14_80_0_80_k35_s1_swish'
    assert g.lut_key(56, 24, 24, 24, 7, 2, 'relu', 1, (3, 5, 7)) == 'MBInvertedResBlock_56_24_24_24_k357_s2_relu'
    assert g.kernel_tag(7) == 'k7' and g.kernel_tag(5, 2) == 'k5d2' and g.kernel_tag(7, 1, (5, 7)) == 'k57'

    class Lut(dict):
        def __missing__(self, key):
            self.asked.append(key)
            return {m: 1.0 for m in range(1, 2000)}
    lut = Lut(base=0.0)
    lut.asked = []
    names = ['MBI_k3_e3', 'MBI_k35_e6', 'MBI_k357_e3', 'MBI_k5_e6', 'MBI_k35_e3_se', 'MBI_k3_e6_se', 'MBI_k5_e3_se', 'DS_k357_se']
    op = ms.MixedOP(16, 16, 1, False, 'relu', 8, dict(enumerate([48, 96] * 4)), lut, primitives=names)
    assert op.get_lookup_latency(28) == [1.0] * 8
    assert lut.asked == ['MBInvertedResBlock_28_16_%d_16_%s_s1_relu' % (se, kt) for se, kt in
                         ((0, 'k3'), (0, 'k35'), (0, 'k357'), (0, 'k5'), (16, 'k35'), (32, 'k3'), (16, 'k5'), (16, 'k357'))]
    import _mix
    import torch
    lut.asked = []
    net = me.NetworkCfg(20, _mix.mix_network_config(20), lut)
    net.get_lookup_latency(torch.zeros(1, 3, 64, 64))
    assert [k.split('_')[5] for k in lut.asked][-5:-1] == ['k35', 'k357', 'k357', 'k35']
    assert '{}'.format(_mix.KTag((3, 5, 7))) == '357' and int(_mix.KTag((3, 5))) == 5


def test_shipped_tables_hold_no_mixconv_key():
    from tfnas_amd import load_lat_lookup
    assert not any(re.search(r'_k(35|37|57|357)_', k) for k in load_lat_lookup('gpu') if k != 'base')
    assert 'No MixConv' in open(os.path.join(ROOT, 'README.md')).read() or 'no MixConv' in open(os.path.join(ROOT, 'README.md')).read()


def test_epoch_boundary_names_the_primitive_it_refuses():
    from tfnas_amd import epoch, geometry as g
    names = list(g.PRIMITIVES)
    names[2] = 'MBI_k357_e3'
    with pytest.raises(NotImplementedError, match=r"search_epoch.*'MBI_k357_e3' as candidate 2"):
        epoch.require_default_primitives('search_epoch', names)


def test_measurer_describes_a_mixconv_block(lib):
    from tfnas_amd import _lib, lut_builder
    d, ws, kind, mc, woff, nw, boff = lut_builder.Measurer._describe(24, 72, 0, 24, 5, 1, 'relu', 28, 28, 4, 'MBInvertedResBlock', 1,
                                                                     (3, 5))
    assert d.g[0].k == 0x53 and d.flags == _lib.CELL_MIXK and kind is _lib.MBCONV
    d1 = lut_builder.Measurer._describe(24, 72, 0, 24, 5, 1, 'relu', 28, 28, 4, 'MBInvertedResBlock')[0]
    assert d1.g[0].k == 5 and d1.flags == 0
    with pytest.raises(NotImplementedError):
        lut_builder.Measurer._describe(24, 72, 0, 24, 3, 1, 'relu', 28, 28, 4, 'FusedMBConvBlock', 1, (3, 5))
    import inspect
    assert 'mix_kernels' in inspect.signature(lut_builder.build_latency_lookup).parameters
    assert 'mix_kernels' in inspect.signature(lut_builder.Measurer.measure).parameters
