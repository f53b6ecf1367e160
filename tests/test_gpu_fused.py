"""Fused-MBConv blocks (TFNAS_CELL_FUSED: a dense 3 x 3 convolution as three implicit GEMMs, csrc/conv_kernels.hip) in the search
form: ``layers.FusedMBConvBlock`` through ``MixedOpFn`` against the float32 CPU restatement of tests/_fused.py (pinned to a
composition of the reference's classes in tests/test_fused_oracle_pin.py): out, dx and every weight gradient.

Shapes are the smallest that reach each way the kernels can go wrong: mid 22 (ragged, mid % 4 != 0), K = 72 ending inside a
16-chunk, odd 7 x 9 images (every border tap, both stride-2 parities), an even width; ic 20 / mid 36 (K = 180: a tap boundary
inside a chunk); 588 rows (four full 128-row tiles and a ragged fifth, the residual gradient in the dgrad store); 14 -> 7 and
7 -> 4 at stride 2.  Raw-ABI cases: accumulation over two backward passes, dx == NULL, need_wgrad = 0, the GEMM modes.
Gate: _hipcheck.worst (atol 2e-5 + rtol 1e-4 * max|ref|), no element exempted; the seeds keep every float64 pre-activation
KINK_TAU from a kink (asserted on the CPU by tests/test_fused_oracle_pin.py)."""
import pytest
import torch

import _fused
import _hipcheck as hc

pytestmark = pytest.mark.gpu


def _report(tag, res):
    print(tag, ' '.join('%s=%.2e/%.2e' % (k, v[0], v[1]) for k, v in res.items()))


@pytest.mark.parametrize('geom', _fused.GEOMS, ids=_fused.geom_id)
def test_search_form_block_matches_the_restatement(geom):
    o, x, r, seed = _fused.case_data(*geom)
    m = _fused.hip_block_like(o)
    res = _fused.compare(o, m, x, r)
    _report(_fused.geom_id(geom), res)
    assert set(res) >= {'out', 'dx', 'g.fused_conv.conv.weight', 'g.point_linear.conv.weight'}
    bad = hc.worst(res)
    assert not bad, bad


def _raw_case(gemm=None, geom=_fused.RAW_GEOM):
    o, x, r, seed = _fused.case_data(*geom, base=300)
    cell = _fused.raw_cell(o, x, gemm=gemm)
    return o, x, r, cell


def _grad_res(got, want):
    return {'g.' + k: hc.err(got[k], want[k]) for k in want}


def test_guard_bands_and_plain_launch():
    o, x, r, cell = _raw_case()
    y, dx, g = _fused.ref_grads(o, x, r)
    out = cell.forward()
    assert cell.guard_ok(cell.D, cell.ws.D)
    rc, dxh, gh = cell.backward(r)
    assert rc == 0 and cell.guard_ok(cell.dx_raw, x.numel())
    res = dict(out=hc.err(out, y), dx=hc.err(dxh, dx), **_grad_res(gh, g))
    _report('raw', res)
    assert not hc.worst(res), hc.worst(res)


def test_accumulation_over_two_backward_passes():
    o, x, r, cell = _raw_case()
    _, _, g1 = _fused.ref_grads(o, x, r)
    _, _, g2 = _fused.ref_grads(o, x, 0.5 * r)
    cell.forward()
    start = [torch.full_like(w, 0.25) for w in cell.w]
    rc, _, acc = cell.backward(r, accum_into=start)
    assert rc == 0
    rc, _, acc = cell.backward(0.5 * r, accum_into=list(acc.values()))
    assert rc == 0
    want = {k: 0.25 + g1[k] + g2[k] for k in g1}
    res = _grad_res(acc, want)
    _report('accum', res)
    assert not hc.worst(res), hc.worst(res)


def test_dx_null_skips_the_data_gradient_and_need_wgrad_0_the_weight_gradients():
    o, x, r, cell = _raw_case()
    _, dx, g = _fused.ref_grads(o, x, r)
    cell.forward()
    rc, dxh, gh = cell.backward(r, want_dx=False)
    assert rc == 0 and dxh is None
    res = _grad_res(gh, g)
    assert not hc.worst(res), hc.worst(res)
    rc, dxh, gh = cell.backward(r, need_wgrad=False)
    assert rc == 0 and gh is None
    res = dict(dx=hc.err(dxh, dx))
    assert not hc.worst(res), hc.worst(res)
    rc, dxh, gh = cell.backward(r, need_wgrad=False, want_dx=False)     # (nothing wanted: returns after the BN_b sums)
    assert rc == 0 and dxh is None and gh is None


def _rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).pow(2).sum().sqrt() / b.pow(2).sum().sqrt())


def test_gemm_modes():
    """fp32 MFMA at the gate of every other test; plain bf16 at the tolerance tests/test_gpu_gemm_modes.py applies to the 1 x 1
    convolutions in that mode: relative L2 error <= 3e-2 against the fp32-MFMA launch of the same block -- on a swish block, as
    there: that bound is a statement about rounding (2^-9 per product), and a 2^-9 perturbation of a pre-activation flips ReLU
    decisions that KINK_TAU = 1e-4 does not protect, each flip an O(1) difference in a gradient element."""
    o, x, r, cell = _raw_case('f32')
    y, dx, g = _fused.ref_grads(o, x, r)
    out0 = cell.forward().clone()
    rc, dx0, g0 = cell.backward(r)
    assert rc == 0
    res = dict(out=hc.err(out0, y), dx=hc.err(dx0, dx), **_grad_res(g0, g))
    _report('f32', res)
    assert not hc.worst(res), hc.worst(res)
    swish = _fused.RAW_GEOM[:8] + ('swish',)
    o, x, r, cell = _raw_case('f32', swish)
    out0 = cell.forward().clone()
    rc, dx0, g0 = cell.backward(r)
    assert rc == 0
    o, x, r, cell = _raw_case('bf16', swish)
    out1 = cell.forward()
    rc, dx1, g1 = cell.backward(r)
    assert rc == 0
    seen = dict(out=_rel_l2(out1, out0), dx=_rel_l2(dx1, dx0), **{'g.' + k: _rel_l2(g1[k], g0[k]) for k in g0})
    print('bf16', seen)
    assert all(v <= 3e-2 for v in seen.values()), seen
    assert seen['out'] > 2e-6 and seen['dx'] > 2e-6        # (the mode is really taken: beyond the split-bf16 level)
