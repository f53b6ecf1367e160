"""Weight-gradient accumulation (TFNAS_CELL_ACCUM_WGRAD, g <- g + v): per launch, every weight-gradient store site adds exactly
the value the same launch stores without the bit; on the drop-in path level, .grad follows autograd's semantics over several
backward passes (bit-identical to the per-cell route, which accumulates through autograd)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- per launch
def _modes(accum, **kw):
    """Launch modes for a plan under test: HipModes(**kw), plus the accumulate bit on every descriptor when `accum`."""
    from tfnas_amd import _lib
    from tfnas_amd.functions import HipModes

    class AccumModes(HipModes):
        def apply(self, d):
            HipModes.apply(self, d)
            if accum:
                d.flags |= _lib.CELL_ACCUM_WGRAD
    return AccumModes(**kw)


def _launch(plan, fn_args, targets, accum, r, streams=None, route=None):
    """One forward + backward of a MixedOpFn / StemFn whose backward writes (accum=False) or adds (accum=True) the weight
    gradients into `targets` (plan.grad_targets)."""
    fn, x, wmix, params = fn_args
    saved = plan._modes
    plan.grad_targets, plan.wgrad_streams, plan._modes = targets, streams, _modes(accum, route=route)
    try:
        out = fn.apply(plan, x, wmix, *params)
        (out * r).sum().backward()
        torch.cuda.synchronize()
    finally:
        plan.grad_targets, plan.wgrad_streams, plan._modes = None, None, saved


def _check_sum(gots, g0, v):
    for i, (o, a, b) in enumerate(zip(gots, g0, v)):
        assert torch.equal(o, a + b), (i, float((o - (a + b)).abs().max()))


def _check_accumulates(plan, fn_args, r, streams=None, route=None):
    params = fn_args[3]
    gen = torch.Generator(device='cuda').manual_seed(17)
    v = [torch.full_like(p, float('nan')) for p in params]
    _launch(plan, fn_args, v, False, r, streams, route)                       # bit clear: every element written
    assert all(bool(torch.isfinite(t).all()) for t in v)
    g0 = [torch.randn(p.shape, device='cuda', generator=gen) for p in params]
    out = [t.clone() for t in g0]
    _launch(plan, fn_args, out, True, r, streams, route)
    _check_sum(out, g0, v)
    again = [t.clone() for t in g0]
    _launch(plan, fn_args, again, False, r, streams, route)                   # ... and without it the same launch overwrites
    for a, b in zip(again, v):
        assert torch.equal(a, b)


CELLS = {   # (ic, oc, stride, act, mids, H, W, N)
    'cell0_s2_relu_ic16': (16, 24, 2, 'relu', [48, 96, 48, 96, 48, 96, 48, 96], 56, 56, 4),
    's1_relu_res': (24, 24, 1, 'relu', [72, 144, 72, 144, 72, 144, 72, 144], 28, 28, 4),
    'swish_se_k5': (40, 40, 1, 'swish', [120, 240, 120, 240, 120, 240, 120, 240], 14, 14, 4),
    'late_7x7': (192, 192, 1, 'swish', [576, 1152, 576, 1152, 576, 1152, 576, 1152], 7, 7, 8),
}


def _cell(name, seed=3):
    import _hipcheck as hc
    ic, oc, stride, act, mids, H, W, N = CELLS[name]
    _, m = hc.make_cell_pair(ic, oc, stride, act, mids, seed=seed)
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(N, ic, H, W, device='cuda', generator=gen).contiguous(memory_format=torch.channels_last)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = torch.randn(N, oc, Ho, Wo, device='cuda', generator=gen)
    return m, x, r


def _cell_args(m, x, idxs):
    from tfnas_amd.functions import MixedOpFn
    plan = m._plan(tuple(idxs))
    params = plan.params()
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    wmix = None
    if len(idxs) > 1:
        wmix = torch.softmax(torch.linspace(-1.0, 1.0, 8, device='cuda'), 0)
    return plan, (MixedOpFn, x.requires_grad_(True), wmix, params)


def _routes():
    from tfnas_amd import functions as Fn
    return {
        'policy': Fn.route_bits(),
        'xg_off': Fn.route_bits(xg='0'),
        'xg_all': Fn.route_bits(xg='all'),
        'dwwg_off': Fn.route_bits(dwwg=False, dwwg2=False),
        'dw_direct': Fn.route_bits(dw='direct'),
        'dw_lds': Fn.route_bits(dw='lds'),
        'dw_tiled': Fn.route_bits(dw='tiled'),
        'se_fused': Fn.route_bits(se='fused'),
        'se_gemm': Fn.route_bits(se='gemm'),
        'inline': Fn.route_bits(wgrad_stream=False),
    }


@pytest.mark.parametrize('name', list(CELLS))
@pytest.mark.parametrize('G', [1, 8])
def test_cell_backward_accumulates_every_weight_gradient(name, G):
    m, x, r = _cell(name)
    idxs = [7 if name == 'swish_se_k5' else 3] if G == 1 else list(range(8))    # (7: k5 with SE; 3: k5 without)
    plan, args = _cell_args(m, x, idxs)
    routes = _routes() if G == 1 else {k: v for k, v in _routes().items() if k in ('policy', 'xg_off', 'xg_all', 'dwwg_off')}
    for rname, bits in routes.items():
        try:
            _check_accumulates(plan, args, r, route=bits)
        except AssertionError as e:
            raise AssertionError('%s / G=%d / route %s: %s' % (name, G, rname, e))


def test_cell_backward_accumulates_with_wgrad_stream_forks():
    m, x, r = _cell('s1_relu_res')
    plan, args = _cell_args(m, x, [5])
    streams = [torch.cuda.Stream() for _ in range(3)]
    _check_accumulates(plan, args, r, streams)


def test_stem_backward_accumulates():
    from tfnas_amd import Network, geometry
    from tfnas_amd.functions import StemFn
    from tfnas_amd.latency import load_lat_lookup
    torch.manual_seed(4)
    model = Network(100, geometry.initial_mc_num_dddict(), load_lat_lookup('gpu')).cuda()
    plan = model.stem_plan()
    params = plan.params()
    gen = torch.Generator(device='cuda').manual_seed(9)
    img = torch.randn(2, 3, 64, 48, device='cuda', generator=gen)
    r = torch.randn(2, 16, 32, 24, device='cuda', generator=gen)
    _check_accumulates(plan, (StemFn, img, None, params), r)


def test_mbconv_affine_backward_accumulates_weights_and_batchnorm_parameters():
    from tfnas_amd.functions import adopt_modes
    from tfnas_amd.layers import MBInvertedResBlock
    torch.manual_seed(6)
    blk = MBInvertedResBlock(24, 72, 24, 24, 5, 1, affine=True, act_func='swish').cuda().train()
    gen = torch.Generator(device='cuda').manual_seed(8)
    x = torch.randn(4, 24, 14, 14, device='cuda', generator=gen).contiguous(memory_format=torch.channels_last)
    r = torch.randn(4, 24, 14, 14, device='cuda', generator=gen)
    params = blk.hip_params() + [t for mod in blk.bn_modules() for t in (mod.weight, mod.bias)]

    def run(grads, accum):
        for p, g in zip(params, grads):
            p.grad = g
        adopt_modes(blk, _modes(accum, direct_grads=True))     # (in-place .grad targets: the kernels store into them)
        (blk(x) * r).sum().backward()
        torch.cuda.synchronize()
        return [p.grad for p in params]

    v = run([torch.full_like(p, float('nan')) for p in params], False)
    assert all(bool(torch.isfinite(t).all()) for t in v)
    v = [t.clone() for t in v]
    g0 = [torch.randn(p.shape, device='cuda', generator=gen) for p in params]
    _check_sum(run([t.clone() for t in g0], True), g0, v)


def _head_backward(plan, saved, dpooled, grads, accum, entry, bn_mod=None):
    """tfnas_head_bwd / tfnas_head_wgrad / tfnas_head_affine_bwd on the tensors a HeadFn / HeadAffineFn forward saved, with the
    weight gradient (and, affine, the BatchNorm parameter gradients) stored into `grads`."""
    import ctypes as C
    from tfnas_amd import _lib
    from tfnas_amd._lib import ptr
    from tfnas_amd.functions import _bn_struct, _part, _stream
    lib = _lib.lib()
    xh, E, stats, w = saved[:4]
    N, H, W, _ = xh.shape
    d, ws = plan.desc(N, H, W)
    plan.bind(d, [w], grads[:1])
    if accum:
        d.flags |= _lib.CELL_ACCUM_WGRAD
    dev = xh.device
    dEh = torch.empty(ws.dEh, device=dev)
    cb1 = torch.empty(4 * d.M, device=dev)
    red = torch.empty(2 * d.M, device=dev, dtype=torch.float64)
    dx = torch.empty((N, H, W, plan.ic), device=dev)
    dxp = torch.empty(ws.dxp, device=dev)
    s = _stream(dev)
    data = (ptr(dpooled), ptr(dEh), ptr(cb1), ptr(red), ptr(_part(ws.part, dev)), ptr(dx), ptr(dxp), s)
    try:
        if entry == 'affine':
            bn = _bn_struct([bn_mod], True, grads[1:])
            assert lib.tfnas_head_affine_bwd(C.byref(d), C.byref(bn), ptr(xh), ptr(E), ptr(stats), *data) == 0
        elif entry == 'bwd':
            assert lib.tfnas_head_bwd(C.byref(d), ptr(xh), ptr(E), ptr(stats), *data) == 0
        else:                           # the weight step's split: data gradient first, then the weight gradient alone
            d.need_wgrad = 0
            assert lib.tfnas_head_bwd(C.byref(d), ptr(xh), ptr(E), ptr(stats), *data) == 0
            d.need_wgrad = 1
            assert lib.tfnas_head_wgrad(C.byref(d), ptr(xh), ptr(E), ptr(dEh), ptr(cb1), ptr(_part(ws.part, dev)), s) == 0
        torch.cuda.synchronize()
    finally:
        d.flags &= ~_lib.CELL_ACCUM_WGRAD
        d.need_wgrad = 0


@pytest.mark.parametrize('entry', ['bwd', 'wgrad', 'affine'])
def test_head_backward_accumulates(entry):
    from tfnas_amd import _lib, model_eval
    from tfnas_amd.functions import CellPlan, HeadAffineFn, HeadFn
    from tfnas_amd.layers import ConvLayer
    torch.manual_seed(5)
    affine = entry == 'affine'
    fm = ConvLayer(320, 1280, kernel_size=1, stride=1, affine=affine, act_func='swish').cuda().train()
    plan = CellPlan(320, 4, 1, 'swish', [model_eval._HeadBlock(fm)], mode=_lib.MODE_HEAD)
    gen = torch.Generator(device='cuda').manual_seed(12)
    x = torch.randn(4, 320, 7, 7, device='cuda', generator=gen).contiguous(memory_format=torch.channels_last)
    w = fm.conv.weight
    if affine:
        pooled = HeadAffineFn.apply(plan, x, fm.bn, True, w, fm.bn.weight, fm.bn.bias)
    else:
        pooled = HeadFn.apply(plan, x, w)
    saved = pooled.grad_fn.saved_tensors
    dpooled = torch.randn(pooled.shape, device='cuda', generator=gen)
    params = [w] + ([fm.bn.weight, fm.bn.bias] if affine else [])

    def run(fill, accum):
        grads = [t.clone() for t in fill]
        _head_backward(plan, saved, dpooled, grads, accum, entry, fm.bn if affine else None)
        return grads
    v = run([torch.full_like(p, float('nan')) for p in params], False)
    assert all(bool(torch.isfinite(t).all()) for t in v)
    g0 = [torch.randn(p.shape, device='cuda', generator=gen) for p in params]
    _check_sum(run(g0, True), g0, v)


# --------------------------------------------------------------------------------------------------------- drop-in route
@pytest.fixture(scope='module')
def lut():
    from tfnas_amd.latency import load_lat_lookup
    return load_lat_lookup('gpu')


P1 = [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
P2 = [7, 1, 5, 3, 0, 5, 2, 7, 6, 1, 2, 4, 4, 0, 6, 3, 1, 1]


def _dropin(lut, paths, positions, between=None):
    from tfnas_amd import Network, geometry, model_search
    old = model_search.MODULE_PATHS
    model_search.MODULE_PATHS = paths
    try:
        torch.manual_seed(2)
        m = Network(100, geometry.initial_mc_num_dddict(), lut).cuda()
        m.set_temperature(5.0)
        for p in m.arch_parameters():                         # (train_w_arch: frozen architecture -> the path level)
            p.requires_grad = False
        gen = torch.Generator(device='cuda').manual_seed(5)
        x = torch.randn(4, 3, 224, 224, device='cuda', generator=gen)
        y = torch.randint(0, 100, (4,), device='cuda', generator=gen)
        for k, pos in enumerate(positions):
            logits, _ = m(x, True, 'max_alphas', pos=pos)
            loss = F.cross_entropy(logits, y)
            if k > 0 and between == 'zero_grad_before_backward':
                m.zero_grad()
            loss.backward()
            if k == 0 and between == 'zero_grad_keep':
                m.zero_grad(set_to_none=False)
            if k == 0 and between == 'foreign_grad':
                for p in m.parameters():                      # .grad that is not the arena view: copied in, then summed
                    if p.grad is not None:
                        p.grad = p.grad.clone()
        torch.cuda.synchronize()
        out = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        if paths:
            st = m.__dict__.get('_pstate')
            assert st is not None and 'B' in st.runner._slots          # (the forwards did run on the path level)
            s = st.runner._slots['B']
            lib = st.runner.lib
            assert lib.tfnas_path_set_wgrad_accum(s.ctx, 1 << 18) == -3          # TFNAS_ERANGE: 18 cells
            assert lib.tfnas_path_set_wgrad_accum(s.ctx, 0xffffffff) == -3
            assert lib.tfnas_path_set_wgrad_accum(s.ctx, (1 << 18) - 1) == 0
            assert lib.tfnas_path_set_wgrad_accum(s.ctx, 0) == 0
        m.close()
        return out
    finally:
        model_search.MODULE_PATHS = old


def _assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize('positions,between', [((P1, P1), None), ((P1, P2), None), ((P1, P2), 'foreign_grad')])
def test_dropin_two_backward_passes_accumulate_like_the_per_cell_route(lut, positions, between):
    _assert_same(_dropin(lut, True, positions, between), _dropin(lut, False, positions, between))


def test_dropin_zero_grad_keeps_single_pass_results(lut):
    single = _dropin(lut, True, (P2,))
    kept = _dropin(lut, True, (P1, P2), 'zero_grad_keep')
    _assert_same({k: v for k, v in kept.items() if k in single}, single)
    assert all(float(v.abs().max()) == 0.0 for k, v in kept.items() if k not in single)
    _assert_same(_dropin(lut, True, (P1, P2), 'zero_grad_before_backward'), single)
