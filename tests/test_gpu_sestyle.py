"""Squeeze-excite styles (TFNAS_CELL_SE_STYLE: TfnasCellDesc.se_style) on raw cells: forward and backward, need_wgrad 0 and 1,
against the float32 CPU restatement of tests/_sestyle.py -- the oracle's blocks with the SE branch's hidden activation and gate
swapped.  Gate: _hipcheck.worst (atol 2e-5 + rtol 1e-4 * max|ref|), no element exempted.

Shapes are the smallest at which the SE kernels can go wrong: 2 x 8 x 7 x 9 at both strides; batch 5 and batch 33 (the batch is
the K dimension of the SE weight gradients, and the bias-gradient kernel walks it in steps of 4 x 8; 33 is also three 16-row tiles
of the wave-level kernels); hidden widths 8 and 12 in ONE launch (two SE groups at different se_off); aligned widths (24, 44: the
wave-level kernels) and a ragged 22 (the per-image and LDS-tiled kernels).  Every style on each of the three TFNAS_ROUTE_SE_*
routes; a plain, an expand-free and a Fused-MBConv one-block cell and the three-kind cell of tests/_kinds.py.
Seeds: _sestyle.case_data -- every float64 pre-activation, the hidden layer's and the gate's included, keeps KINK_TAU from every
kink; asserted here on the CPU restatement alone, before anything is launched.  Under a hard-sigmoid gate the restatement's gate
biases are spread so that all three branches of the gate occur (asserted as well)."""
import pytest
import torch

import _hipcheck as hc
import _kinds
import _sestyle as S

pytestmark = pytest.mark.gpu

ALIGNED = [('M', 24, 3, 8), ('M', 44, 5, 12)]               # two SE groups, se 8 and 12, widths the wave-level kernels take
RAGGED = [('M', 24, 3, 8), ('F', 22, 12), ('N', 5, 0)]      # ... and a ragged one (mc 22): per-image / LDS-tiled kernels
ONE_BLOCK = {'plain': [('M', 22, 5, 8)], 'noexp': [('N', 5, 8)], 'fused': [('F', 22, 8)], 'three': _kinds.THREE}
ROUTES = ('wave', 'fused', 'gemm')

_CACHE = {}


def _case(cands, geom, style):
    """case_data and the restatement's results, computed once and shared (never changed) by the tests that need them"""
    key = (tuple(cands), geom, style)
    if key not in _CACHE:
        act, se_act, se_gate = style
        o, x, r, w, seed = S.case_data(cands, *geom, act, se_act, se_gate)
        if len(cands) == 1:
            w = torch.ones(1)
        _CACHE[key] = (o, x, r, w, _kinds.ref_run(o, x, r, w))
    o, x = _CACHE[key][:2]
    assert S.kink_distance(o, x) >= S.KINK_TAU                   # (CPU restatement alone; nothing has been launched)
    if style[2] == 'h-sigmoid' and any(op.squeeze_excite is not None for op in o.m_ops):
        assert min(S.gate_branches(o, x)) > 0, S.gate_branches(o, x)
    return _CACHE[key]


def _plan(o, route='wave', blocks=None):
    from tfnas_amd.functions import CellPlan, HipModes, route_bits
    blocks = S.hip_blocks_like(o) if blocks is None else blocks
    return CellPlan(o.in_channels, o.out_channels, o.stride, o.act_func, blocks, modes=HipModes(route=route_bits(se=route)),
                    mixed_kinds=True)


def _run(plan, x, r, w, need_wgrad):
    """_kinds.hip_run; a one-block plan runs in the sampled form (wmix == NULL) and reports d wmix = <out, r> as the soft form
    of a one-candidate cell with weight 1 would"""
    if len(plan.blocks) > 1:
        return _kinds.hip_run(plan, x, r, w, need_wgrad)
    from collections import OrderedDict
    from tfnas_amd.functions import MixedOpFn
    params = plan.params()
    for p in params:
        p.requires_grad_(need_wgrad)
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = MixedOpFn.apply(plan, xm, None, *params)
    (y * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = OrderedDict(('g0.' + k, p.grad.clone()) for k, p in plan.blocks[0].named_parameters()) if need_wgrad else None
    return y.detach(), xm.grad, None, grads


def _check(tag, cands, geom, style, route='wave'):
    from tfnas_amd import _lib
    o, x, r, w, ref = _case(cands, geom, style)
    plan = _plan(o, route)
    d = plan.desc(geom[0], geom[3], geom[4])[0]
    has_se = any(c[-1] for c in cands)
    assert d.se_style == (_lib.se_style_id(*style[1:]) if has_se else 0)
    assert bool(d.flags & _lib.CELL_SE_STYLE) == bool(d.se_style) and d.route == _lib.ROUTE_SE[route]
    for need_w in (0, 1):
        got = _run(plan, x, r, w, bool(need_w))
        if got[2] is None:
            got = (got[0], got[1], ref[2], got[3])
        res = _kinds.compare(ref, got)
        print('%s w%d' % (tag, need_w), ' '.join('%s=%.2e/%.2e' % (k, v[0], v[1]) for k, v in res.items()))
        assert (len(res) > 3) == bool(need_w)
        bad = hc.worst(res)
        assert not bad, bad


_ids = lambda st: '%s_%s_%s' % (st[0], st[1] or 'own', st[2])     # noqa: E731


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('style', S.STYLES, ids=_ids)
def test_every_style_on_every_excite_route(style, route):
    """two SE groups (se 8 at se_off 0, se 12 at se_off 8) of aligned widths: route 'wave' runs k_se_nt / k_se_nn, 'fused' the
    per-image pair, 'gemm' the LDS-tiled GEMMs; the weight-gradient modes and the bias gradients run in all three"""
    _check('routes %s %s' % (_ids(style), route), ALIGNED, _kinds.SMALL_SHAPE + (1,), style, route)


@pytest.mark.parametrize('stride', (1, 2))
@pytest.mark.parametrize('kind', sorted(ONE_BLOCK))
def test_every_kind_of_cell(kind, stride):
    _check('%s s%d' % (kind, stride), ONE_BLOCK[kind], _kinds.SMALL_SHAPE + (stride,), S.STYLES[0])


@pytest.mark.parametrize('style', S.STYLES[1:], ids=_ids)
def test_three_kind_cell_in_the_other_styles(style):
    _check('three %s' % _ids(style), _kinds.THREE, _kinds.SMALL_SHAPE + (2,), style)


@pytest.mark.parametrize('batch,cands,route', [(5, RAGGED, 'gemm'), (33, RAGGED, 'gemm'), (33, ALIGNED, 'wave'), (5, RAGGED, 'fused')],
                         ids=('n5_gemm', 'n33_gemm', 'n33_wave', 'n5_fused'))
def test_batch_sizes_of_the_weight_gradient_k_dimension(batch, cands, route):
    _check('batch %d %s' % (batch, route), cands, (batch, 8, 8, 7, 9, 1), S.STYLES[0], route)


# ------------------------------------------------------------------------------------------------ bit for bit
def _all(plan, x, r, w):
    got = _run(plan, x, r, w, True)
    return [got[0].clone(), got[1].clone()] + ([] if got[2] is None else [got[2].clone()]) + [g for g in got[3].values()]


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('act', ('relu', 'swish', 'h-swish'))
def test_defaults_spelled_explicitly_equal_the_unflagged_launch_bitwise(act, route):
    """hidden = the cell's act by id, logistic gate, TFNAS_CELL_SE_STYLE set: the kernels the unflagged descriptor launches"""
    from tfnas_amd import _lib
    o, x, r, w, _ = _case(ALIGNED, _kinds.SMALL_SHAPE + (1,), (act, None, 'sigmoid'))
    blocks = S.hip_blocks_like(o)
    old, new = _plan(o, route, blocks), _plan(o, route, blocks)
    new.se_style = _lib.se_style_id(act, 'sigmoid')
    do, dn = old.desc(2, 7, 9)[0], new.desc(2, 7, 9)[0]
    assert do.se_style == 0 and not do.flags & _lib.CELL_SE_STYLE
    assert dn.se_style == 1 + _lib.ACT[act] and dn.flags & _lib.CELL_SE_STYLE
    a, b = _all(old, x, r, w), _all(new, x, r, w)
    assert len(a) == len(b) > 4 and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize('cands', ([('M', 22, 3, 0)], [('M', 22, 3, 0), ('N', 5, 0), ('F', 22, 0)]), ids=('one', 'three'))
def test_styled_cell_without_se_groups_equals_the_unstyled_launch_bitwise(cands):
    from tfnas_amd import _lib
    o, x, r, w, _ = _case(cands, _kinds.SMALL_SHAPE + (1,), ('h-swish', None, 'sigmoid'))
    blocks = S.hip_blocks_like(o)
    old, new = _plan(o, blocks=blocks), _plan(o, blocks=blocks)
    new.se_style = _lib.se_style_id('relu', 'h-sigmoid')
    do, dn = old.desc(2, 7, 9)[0], new.desc(2, 7, 9)[0]
    assert do.se_style == 0 and dn.se_style == 0x11 and dn.flags & _lib.CELL_SE_STYLE and dn.SE == 0
    a, b = _all(old, x, r, w), _all(new, x, r, w)
    assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))
