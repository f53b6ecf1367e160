"""Workspace independence of the plain eight-candidate cell on its default route (what bench.py times), at the C ABI.

Contract: no entry point reads a workspace buffer it has not written in the same call; only the
reserved words of `part` must be zero; nothing past the sizes tfnas_cell_ws reports is touched.  Every case runs the launch pair
on buffers the probe made (tests/_wsprobe.py: guard bands of 4096 elements on both sides, interiors poisoned) and holds it to

  1. run(A) == run(B) in every bit of out, Pr, D / E (valid columns), dx, dwmix and every weight gradient (two poisons that
     differ at every element);
  2. every guard word intact after the forward and after the backward;
  3. run(A) == the same launch through MixedOpFn.apply in every bit (the route tests/test_gpu_cell.py holds to the oracle: equal
     garbage cannot pass), with E == NULL in the one exactly where it is in the other.

No cell kernel uses floating-point atomics; there is no tolerance anywhere in this file.

Kernel families per row, read off the planners (dwconv_kernels.hip: dw_plan_fwd / dw_plan_bwd_data / dw_plan_wgrad, dwd_*_use,
pick_slide, dws_pipe, dwd_plan; fx_kernels.hip: fx_plan, fx_supported; efree_kernels.hip; functions._cell_forward's E-free policy:
stride 2 and ic <= 24 and frozen weights).  There is no query for a family: the table is kept by hand against that code, the
asserts below cover what the ABI can tell (tfnas_cell_route, tfnas_efree_supported).  "rw" = register-window (k_dwd_*), "ring" =
k_dws_*, "tile" = the LDS tile kernels; fwd / bwd / wg = the three depthwise passes (wg only with need_wgrad and only where the
backward pass does not carry the weight gradient itself).

  row                  geometry (N ic oc s act HxW)   mids     families
  tiny_s1_relu_res     2 24 24 1 relu  9x11           CONFIGS  fwd tile, bwd tile (W < 14: no ring); wg rw (W <= 14, even mids);
                                                               SE wave kernels (SE groups' mids % 4 == 0); residual
  tiny_ragged_res      3 40 40 1 swish 8x6            CONFIGS  fwd / bwd / wg tile (W < 14; odd mids: dwd_plan refuses); SE per-image
                                                               or tiled kernels (a mid % 4 != 0); residual
  tiny_1x1_img         5 16 16 1 swish 1x1            CONFIGS  fwd / bwd / wg tile (odd mids), one pixel per image; residual
  tiny_s2_relu         2 16 24 2 relu  12x10          CONFIGS  frozen: E-free (E == NULL), tile kernels recomputing E (stride 2: no
  tiny_s2_swish_odd    2 24 40 2 swish 9x13           CONFIGS  ring; H < 56: no rw forward).  need_wgrad: fwd tile, bwd rw with the
                                                               fused stride-2 weight gradient (dw_plan_bwd_data: k 3 and 5)
  rw_fwd_s2_57x58      1 16 24 2 relu  57x58          even     need_wgrad: fwd rw (dwd_fwd_use: stride 2, H >= 56), bwd rw + fused
                                                               weight gradient.  frozen: E-free tile kernels, ragged tile borders
  rw_s1_6x60           1 16 16 1 relu  6x60           even     fwd / bwd / wg rw at stride 1 (W > 56: no ring either); residual
  ring_17x23           3 24 24 1 swish 17x23          ragged   fwd / bwd ring, TH = 4 rows per block: the last block holds one row;
                                                               prefetch (dws_pipe: W > 20 and M >= 512) in the soft launches
                                                               (M = 864), none in the sampled ones; wg ring (odd mids: no rw)
  ring_pipe_9x44       2 24 24 1 relu  9x44           ragged   fwd / bwd ring with prefetch (W > 40); sampled 3 x 3 with need_wgrad:
                                                               the ring backward carries the weight gradient (W >= 28), no prefetch
  fx_14x14_80          3 80 80 1 swish 14x14          ragged   frozen: fused per-image route, one image per workgroup, dEh as
  fx_10x12_96          3 96 96 1 relu  10x12          ragged   [nslices + 1][P][ic] scratch; E == NULL: recompute form (k_fx_bwd).
  fx_5x9_64            7 64 64 1 swish 5x9            ragged   5x9: two images per workgroup (128 / 45), the fourth group half
                                                               empty.  need_wgrad: materialised route, ring (14x14) / tile kernels
  max_width_7          2 192 192 1 swish 7x7          CONFIGS  K-split project forward, split expand dgrad (dxp); materialised in
                                                               every soft mode (M = 9248: the fused route's planner refuses the
                                                               eight-candidate launch), fwd / bwd tile, wg rw; the frozen sampled
                                                               launch (M = 768) takes the fused per-image route

Route words: every entry of test_gpu_cell.VARIANTS once, on the smallest row (in pixels) whose launches the switch changes
(ROUTE_CASES gives the reason per word), in the soft frozen mode and the sampled need_wgrad mode of candidate 5 (3 x 3 with SE).
TFNAS_CELL_ACCUM_WGRAD is not probed: it reads its destinations by contract."""
import functools

import pytest
import torch

import _hipcheck as hc
import _wsprobe as wp
from test_gpu_cell import CONFIGS, VARIANTS

pytestmark = pytest.mark.gpu

RAGGED = (0, 5, 29, 9, 83, 1, 19, 12)
EVEN = (0, 6, 30, 10, 84, 2, 20, 12)         # (the register-window planner refuses odd mc)
_CFG = {c[0]: c for c in CONFIGS}


def _row(name, N, ic, oc, stride, act, H, W, extra):
    return (name, ic, oc, stride, act, H, W, N, [3 * ic + v for v in extra])


ROWS = [_CFG[n] for n in ('tiny_s1_relu_res', 'tiny_ragged_res', 'tiny_1x1_img', 'tiny_s2_relu', 'tiny_s2_swish_odd')] + [
    _row('rw_fwd_s2_57x58', 1, 16, 24, 2, 'relu', 57, 58, EVEN),
    _row('rw_s1_6x60', 1, 16, 16, 1, 'relu', 6, 60, EVEN),
    _row('ring_17x23', 3, 24, 24, 1, 'swish', 17, 23, RAGGED),
    _row('ring_pipe_9x44', 2, 24, 24, 1, 'relu', 9, 44, RAGGED),
    _row('fx_14x14_80', 3, 80, 80, 1, 'swish', 14, 14, RAGGED),
    _row('fx_10x12_96', 3, 96, 96, 1, 'relu', 10, 12, RAGGED),
    _row('fx_5x9_64', 7, 64, 64, 1, 'swish', 5, 9, RAGGED),
    _CFG['max_width_7'],
]
_ROW = {r[0]: r for r in ROWS}
FX_ROWS = ('fx_14x14_80', 'fx_10x12_96', 'fx_5x9_64')                       # the fused per-image route is meant (frozen modes)
FX_ALSO = {('max_width_7', 'sampled0_frozen')}                               # ... and in this launch (see the table)
EFREE_ROWS = ('tiny_s2_relu', 'tiny_s2_swish_odd', 'rw_fwd_s2_57x58')        # the policy passes E == NULL (frozen modes)
assert all(r[7] * r[5] * r[6] <= 4000 for r in ROWS)                         # a few thousand pixels at most

# route word -> (row, why this is the smallest row the switch acts on)
ROUTE_CASES = {
    'lds_depthwise_only': ('tiny_s2_swish_odd', 'smallest stride-2 row: its register-window backward becomes a tile launch'),
    'register_window_depthwise_everywhere': ('tiny_s1_relu_res', 'smallest row of even mids: all three tile passes become rw'),
    'tiled_depthwise': ('ring_pipe_9x44', 'smallest ring row (on the rw rows it launches what lds_depthwise_only launches)'),
    'se_fused_per_image': ('tiny_s1_relu_res', 'smallest row whose SE groups take the wave kernels by default'),
    'se_lds_gemm': ('tiny_s1_relu_res', 'as se_fused_per_image'),
    'bn2_tables_in_their_own_pass': ('tiny_s1_relu_res', 'smallest row of VARIANTS\' own list for this word'),
    'depthwise_weight_gradient_in_its_own_kernel': ('ring_pipe_9x44', 'the only row whose ring backward carries the weight gradient'),
    'stride2_depthwise_weight_gradient_in_its_own_kernel': ('tiny_s2_swish_odd', 'smallest stride-2 row (fused rw weight gradient)'),
    'weight_gradients_on_the_callers_stream': ('tiny_1x1_img', 'every need_wgrad launch: the smallest row'),
    'expand_weight_gradient_gram_form_everywhere': ('tiny_1x1_img', 'every need_wgrad launch with ic % 4 == 0: the smallest row'),
    'expand_weight_gradient_per_element_from_E': ('tiny_1x1_img', 'acts from 100 MB of E on, beyond any row here: the word alone'),
    'materialised_late_cells': ('fx_5x9_64', 'smallest row of the fused per-image route'),
    'gram_operator_split_k': ('tiny_1x1_img', 'every backward with dx: the smallest row'),
}
assert sorted(ROUTE_CASES) == sorted(VARIANTS)


@functools.lru_cache(maxsize=None)
def _cell(name):
    """(product MixedOP on cuda, x, cotangent, mix weights) of a row: made once, never changed"""
    _, ic, oc, s, act, H, W, N, mids = _ROW[name]
    _, m = hc.make_cell_pair(ic, oc, s, act, mids, seed=len(name))
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, ic, H, W, generator=g)
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=g)
    w = torch.softmax(torch.randn(8, generator=g), 0)
    return m, x, r, w


def _check(name, mode, route=None, efree=None, tamper_b=None):
    """properties 1-3 of one row x mode (route: TFNAS_ROUTE_* bits of the cell's launches); returns the probe and run(A) | run(B)"""
    from tfnas_amd import _lib, functions as F
    m, x, r, w = _cell(name)
    idx, need_wgrad, want_dx = wp.MODES[mode]
    idxs, wmix = (tuple(range(8)), w) if idx is None else ((idx,), None)
    wp.check_seed_pair(wp.SEED_A, wp.SEED_B, 4096)
    F.adopt_modes(m, F.HipModes(route=route))
    try:
        p = wp.WsProbe(m, idxs, x, r, wmix, need_wgrad, want_dx, efree=efree)
        # what the ABI can tell of the family
        fx_meant = ((name in FX_ROWS and not need_wgrad) or (name, mode) in FX_ALSO) and not (route or 0) & _lib.ROUTE_FX_OFF
        assert p.fwd_route == _lib.ROUTE_TAKEN_VALID | (_lib.ROUTE_TAKEN_FX if fx_meant else 0), (p.fwd_route, fx_meant)
        if efree is None:
            assert p.efree == (name in EFREE_ROWS and not need_wgrad), p.efree
        if p.efree:
            assert p.efree_supported == 1
        ra = p.run(wp.SEED_A)
        rb = p.run(wp.SEED_B, tamper=tamper_b)
        if tamper_b is not None:
            return p, ra, rb
        print('%s %s: %d results, %d buffers, E %s, fwd_route %d' % (name, mode, len(ra), len(p.bufs),
                                                                     'NULL' if p.E is None else 'kept', p.fwd_route))
        assert wp.compare(ra, rb) == {}, 'results depend on what the workspace held before'
        if efree is None:
            rm, kept_E = wp.module_run(m, idxs, x, r, wmix, need_wgrad, want_dx)
            assert kept_E == (p.E is not None)
            assert set(rm) == set(ra) - {'Pr', 'E'}, (sorted(rm), sorted(ra))
            assert wp.compare({k: ra[k] for k in rm}, rm) == {}, 'the probe launch differs from MixedOpFn.apply'
        return p, ra, rb
    finally:
        F.adopt_modes(m, F.HipModes())


_CASES = [(r[0], mode) for r in ROWS for mode in wp.MODES]


@pytest.mark.parametrize('name,mode', _CASES, ids=['%s-%s' % c for c in _CASES])
def test_results_do_not_depend_on_the_workspace(name, mode):
    p, ra, _ = _check(name, mode)
    idx, need_wgrad, want_dx = wp.MODES[mode]
    assert ('dx' in ra) == want_dx and ('dwmix' in ra) == (idx is None)
    assert sum(k.startswith('g') for k in ra) == (len(p.w) if need_wgrad else 0)
    assert {'dZ', 'dEh', 'bsmall', 'red', 'part_fwd', 'part_bwd', 'D', 'Pr', 'fsmall', 'stats', 'out'} <= set(p.bufs)
    if not want_dx and not need_wgrad:
        assert p.bufs['dZ'].n == 4 and p.bufs['dEh'].n == 4                   # only d wmix: 4-float dZ / dEh, no dx, no dxp
        assert 'dx' not in p.bufs and 'dxp' not in p.bufs
    assert p.bufs['part_bwd'].n == (2 if need_wgrad else 1) * p.piece


@pytest.mark.parametrize('name', FX_ROWS)
def test_fused_route_recompute_form_without_an_E_buffer(name):
    """frozen soft mode of the fused per-image rows with E == NULL (the policy keeps the buffer for ehat): k_fx_bwd recomputes"""
    p, ra, _ = _check(name, 'soft_frozen', efree=True)
    assert p.E is None and 'E' not in ra and 'E' not in p.bufs


_RCASES = [(v, mode) for v in sorted(ROUTE_CASES) for mode in ('soft_frozen', 'sampled5_wgrad')]


@pytest.mark.parametrize('variant,mode', _RCASES, ids=['%s-%s' % c for c in _RCASES])
def test_route_words_do_not_depend_on_the_workspace(variant, mode):
    from tfnas_amd import functions as F
    _check(ROUTE_CASES[variant][0], mode, route=F.route_bits(**VARIANTS[variant][0]))


def test_probe_sees_a_dependence_when_there_is_one():
    """One mantissa bit of one valid element of the saved D flipped between forward and backward of run(B): dx must differ.  (D is
    data: nothing indexes by it.)"""
    def tamper(p):
        d = p.d
        assert d.g[0].mc > 0
        word = wp.bits(p.D)[d.g[0].off:d.g[0].off + 1]                        # pixel 0, first channel of group 0
        assert word.data_ptr() == p.D.data_ptr() + 4 * d.g[0].off
        word ^= 1 << 22                                                        # the top mantissa bit
    _, ra, rb = _check('tiny_ragged_res', 'soft_frozen', tamper_b=tamper)
    bad = wp.compare(ra, rb)
    assert 'dx' in bad, bad
    assert not {'out', 'Pr', 'D', 'E'} & set(bad), bad                         # (the forward's results were taken before the flip)
