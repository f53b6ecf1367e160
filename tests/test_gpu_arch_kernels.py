"""GPU: the architecture-parameter and sink kernels (csrc/arch_kernels.hip) at the raw C ABI against the float64 restatements of
_smallref.py (pinned to the oracle / torch float64 by test_small_refs.py): tfnas_arch_fwd / bwd over ncell x temperature with every
NULL branch, tfnas_arch_sample under random partial masks at ncell > 1 (the bi-sampling state), tfnas_sink_fwd / bwd from one
float4 up to the size where all 2048 workgroups loop, with every optional output switched off in turn."""
import ctypes as C

import numpy as np
import pytest
import torch

import _smallref as sr

pytestmark = pytest.mark.gpu

EINVAL, ENULL, ERANGE = -1, -2, -3
SENT = -4242.5


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(t, n):
    from tfnas_amd import _lib
    return _lib.raw_array([t[i].data_ptr() for i in range(n)])


# ------------------------------------------------------------------------------------------ tfnas_arch_fwd / bwd
def _arch_inputs(ncell, seed, extreme):
    g = torch.Generator().manual_seed(seed)
    la = torch.log_softmax(torch.randn(ncell, 8, generator=g), -1)
    e = torch.empty(ncell, 8).exponential_(generator=g)
    if extreme:                                   # Exp(1) draws mixed with a tiny and a huge one (gumbel +69 / -3.9)
        for c in range(ncell):
            e[c, (3 * c) % 8] = 1e-30 if c % 2 == 0 else 50.0
            if c % 3 == 0:
                e[c, (3 * c + 5) % 8] = 50.0
    lat = torch.rand(ncell, 8, generator=g) * 2
    dw = torch.randn(ncell, 8, generator=g)
    dcl = torch.randn(ncell, generator=g)
    return la, e, lat, dw, dcl


def _fp32_cpu_error(la, e, lat, dw, dcl, T, w_in, combos):
    """Error of the same formulas in torch fp32 on the CPU against the float64 reference: what fp32 rounding of the scaled logit
    costs on these very inputs (max abs error of w, of cell_lat, and of the gradient per NULL combination)."""
    w32 = ((la + (-e.log())) / T).softmax(-1)
    w_ref, cl_ref = sr.gumbel_ref(la, e, T, lat)
    ew = float(np.abs(sr.d64(w32) - w_ref).max())
    ecl = float(np.abs(sr.d64((w32 * lat).sum(1)) - cl_ref).max())
    eg = []
    for use_dw, use_dcl, use_lat in combos:
        gt = torch.zeros_like(w_in)
        if use_dw:
            gt = gt + dw
        if use_dcl and use_lat:
            gt = gt + dcl[:, None] * lat
        g32 = w_in * (gt - (gt * w_in).sum(1, keepdim=True)) / T
        ref = sr.arch_bwd_ref(w_in, lat if use_lat else None, dw if use_dw else None, dcl if use_dcl else None, T)
        eg.append(float(np.abs(sr.d64(g32) - ref).max()))
    return ew, ecl, eg


BWD_COMBOS = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)]       # (dw, dcell_lat, lat) given / NULL


@pytest.mark.parametrize('T', [5.0, 1.0, 0.1])
@pytest.mark.parametrize('ncell', [1, 18, 32])
def test_arch_fwd_bwd_match_float64(ncell, T):
    """Ordinary noise at T >= 1: the tolerances of test_gpu_arch.py (w 1e-6, cell_lat 1e-5, gradients atol 1e-6 / rtol 1e-4).
    At T = 0.1, or with e mixing Exp(1) draws with 1e-30 and 50, fp32 rounding of the scaled logit dominates: the allowance there is
    those floors plus 4 x the error of the same formula in torch fp32 on the CPU, measured on the same inputs.  Measured (CPU fp32
    against float64, worst over ncell; w / cell_lat / gradients): T = 0.1 ordinary 3.4e-7 / 2.9e-7 / 1.9e-6, T = 0.1 extreme
    3.4e-7 / 2.5e-7 / 2.2e-6, T = 1 extreme 1.2e-7 / 2.3e-7 / 8.2e-8, T = 5 extreme 1.2e-7 / 4.0e-7 / 1.2e-7 -- i.e. the
    allowance grows from 1e-6 to at most 2.4e-6 for w and from 1e-6 to at most 9.9e-6 (+ 1e-4 relative) for the gradients."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    s = _stream()
    worst = {}
    for extreme in (False, True):
        la, e, lat, dw, dcl = _arch_inputs(ncell, 1000 * ncell + int(10 * T) + extreme, extreme)
        w_ref, cl_ref = sr.gumbel_ref(la, e, T, lat)
        w_in = torch.from_numpy(w_ref).float()                      # the backward's input: independent of the GPU forward
        strict = T >= 1.0 and not extreme
        ew, ecl, eg = (0.0, 0.0, [0.0] * len(BWD_COMBOS)) if strict else _fp32_cpu_error(la, e, lat, dw, dcl, T, w_in, BWD_COMBOS)
        print('ncell %d T %g %s: fp32 CPU error w %.2e cell_lat %.2e grads %s' % (
            ncell, T, 'extreme' if extreme else 'ordinary', ew, ecl, ['%.2e' % v for v in eg]))
        LA, E, LAT = la.cuda(), e.cuda(), lat.cuda()
        for use_lat, use_cl in ((1, 1), (0, 0), (1, 0), (0, 1)):
            W = torch.full((ncell + 1, 8), SENT, device='cuda')
            CL = torch.full((ncell + 1,), SENT, device='cuda')
            rc = lib.tfnas_arch_fwd(ncell, _rows(LA, ncell), _lib.ptr(E), _lib.ptr(LAT) if use_lat else None, T, _lib.ptr(W),
                                    _lib.ptr(CL) if use_cl else None, s)
            assert rc == 0
            torch.cuda.synchronize()
            W, CL = W.cpu(), CL.cpu()
            err = float(np.abs(sr.d64(W[:ncell]) - w_ref).max())
            assert err <= 1e-6 + 4 * ew, 'w: %.3e' % err
            worst['w'] = max(worst.get('w', 0.0), err / (1e-6 + 4 * ew))
            assert bool((W[ncell] == SENT).all()) and float(CL[ncell]) == SENT
            if use_cl:
                want = cl_ref if use_lat else np.zeros(ncell)       # no latency table: the expected latency is 0
                err = float(np.abs(sr.d64(CL[:ncell]) - want).max())
                assert err <= 1e-5 + 4 * ecl, 'cell_lat: %.3e' % err
                worst['cell_lat'] = max(worst.get('cell_lat', 0.0), err / (1e-5 + 4 * ecl))
            else:
                assert bool((CL == SENT).all())
        Win, DW, DCL = w_in.cuda(), dw.cuda(), dcl.cuda()
        for (use_dw, use_dcl, use_lat), e32 in zip(BWD_COMBOS, eg):
            DLA = torch.full((ncell + 1, 8), SENT, device='cuda')
            rc = lib.tfnas_arch_bwd(ncell, _lib.ptr(Win), _lib.ptr(LAT) if use_lat else None, _lib.ptr(DW) if use_dw else None,
                                    _lib.ptr(DCL) if use_dcl else None, T, _rows(DLA, ncell), s)
            assert rc == 0
            torch.cuda.synchronize()
            DLA = DLA.cpu()
            ref = sr.arch_bwd_ref(w_in, lat if use_lat else None, dw if use_dw else None, dcl if use_dcl else None, T)
            err = np.abs(sr.d64(DLA[:ncell]) - ref)
            lim = 1e-6 + 1e-4 * np.abs(ref) + 4 * e32
            assert np.all(err <= lim), 'gradient (dw %d dcl %d lat %d): %.3e' % (use_dw, use_dcl, use_lat, float(err.max()))
            worst['grad'] = max(worst.get('grad', 0.0), float((err / lim).max()))
            assert bool((DLA[ncell] == SENT).all())
            if not use_dw and not (use_dcl and use_lat):
                assert bool((DLA[:ncell] == 0).all())
    print('arch_fwd/bwd ncell %d T %g: worst error / allowance %s' % (ncell, T, {k: round(v, 3) for k, v in worst.items()}))


def test_arch_fwd_bwd_refuse_bad_cell_counts():
    from tfnas_amd import _lib
    lib = _lib.lib()
    X = torch.full((33, 8), SENT, device='cuda')
    E = torch.ones(33, 8, device='cuda')
    for ncell in (0, 33):
        assert lib.tfnas_arch_fwd(ncell, _rows(X, 33), _lib.ptr(E), None, 1.0, _lib.ptr(X), None, _stream()) == ERANGE
        assert lib.tfnas_arch_bwd(ncell, _lib.ptr(E), None, None, None, 1.0, _rows(X, 33), _stream()) == ERANGE
    torch.cuda.synchronize()
    assert bool((X == SENT).all())


# ------------------------------------------------------------------------------------------------ tfnas_arch_sample
def _sample(lib, la, mask, e, T, mode):
    from tfnas_amd import _lib
    ncell = la.shape[0]
    LA, M = la.cuda(), mask.to(torch.uint8).cuda()
    E = e.cuda() if e is not None else None
    pos = torch.full((ncell + 1,), -9, dtype=torch.int32, device='cuda')
    rc = lib.tfnas_arch_sample(ncell, _rows(LA, ncell), _lib.ptr(M), _lib.ptr(E), T, mode, _lib.ptr(pos), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    pos = pos.cpu()
    assert int(pos[ncell]) == -9
    return pos[:ncell].numpy()


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_arch_sample_positions_equal_the_reference(mode):
    """66 calls per mode over ncell in {1, 18, 32} and T in {5.0, 0.1}, random masks with 1..8 candidates on per cell: positions equal
    sample_ref exactly.  Mode 0 may leave out a cell whose two largest float64 weights are within 1e-5 relative, at most 1 % of the
    cells (test_small_refs.py: the case list itself leaves out none; its smallest gap is 8.8e-4)."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    cells = left_out = 0
    for k, case in enumerate(c for c in sr.sample_cases() if c['mode'] == mode):
        ref, gap = sr.sample_ref(case['la'], case['mask'], case['e'], case['T'], mode)
        got = _sample(lib, case['la'], case['mask'], None if (mode and k % 2) else case['e'], case['T'], mode)   # e is unused in modes 1 / 2
        keep = gap >= sr.SAMPLE_GAP
        cells += len(ref)
        left_out += int((~keep).sum())
        assert np.array_equal(got[keep], ref[keep]), 'call %d (ncell %d, T %g): %s vs %s' % (k, case['ncell'], case['T'], got, ref)
    assert left_out <= sr.SAMPLE_CAP * cells


def test_arch_sample_ties_give_the_first_position():
    """Exact ties are never left out: all-equal log_alphas (the network's initial state) and a duplicated extreme give the first
    position in modes 1 / 2, as torch's CPU argmin / argmax do in the oracle; all-equal log_alphas in mode 0 follow the noise."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    for la, mask in sr.tie_cases():
        for mode in (1, 2):
            assert np.array_equal(_sample(lib, la, mask, None, 1.0, mode), sr.sample_ref(la, mask, None, 1.0, mode)[0])
    eq, m_eq = sr.tie_cases()[0]
    e = torch.empty(3, 8).exponential_(generator=torch.Generator().manual_seed(8))
    for T in (5.0, 0.1):
        ref, gap = sr.sample_ref(eq, m_eq, e, T, 0)
        assert float(gap.min()) > 1e-3
        assert np.array_equal(_sample(lib, eq, m_eq, e, T, 0), ref)
    # mode 0 with equal log_alphas AND equal noise: the weights are bit-identical whatever the rounding, so the first position wins
    ones = torch.ones(3, 8)
    for T in (5.0, 0.1):
        assert _sample(lib, eq, m_eq, ones, T, 0).tolist() == [0, 0, 0] == sr.sample_ref(eq, m_eq, ones, T, 0)[0].tolist()


def test_arch_sample_refusals():
    from tfnas_amd import _lib
    lib = _lib.lib()
    LA = torch.zeros(33, 8, device='cuda')
    M = torch.ones(33, 8, dtype=torch.uint8, device='cuda')
    pos = torch.full((33,), -9, dtype=torch.int32, device='cuda')
    call = lambda ncell, e, mode: lib.tfnas_arch_sample(ncell, _rows(LA, 33), _lib.ptr(M), _lib.ptr(e), 1.0, mode, _lib.ptr(pos), _stream())
    E = torch.ones(33, 8, device='cuda')
    assert call(4, E, -1) == EINVAL
    assert call(4, E, 3) == EINVAL
    assert call(4, None, 0) == ENULL
    assert call(33, E, 0) == ERANGE
    assert call(0, E, 0) == ERANGE
    torch.cuda.synchronize()
    assert bool((pos == -9).all())


# ------------------------------------------------------------------------------------------------ tfnas_sink_fwd / bwd
BIG = 4 * (2048 * 512 + 3)          # the smallest count at which each of the 2048 workgroups iterates twice and one pass is ragged


def _sink_case(lib, K, count, seed, variant, worst):
    """variant 'full': latency in and out, every output.  'nolat': cell_lat / dlat / dcell_lat NULL, every second dres NULL.
    'nobetas': dbetas and out_lat NULL."""
    from tfnas_amd import _lib
    g = torch.Generator().manual_seed(seed)
    betas = torch.randn(K, generator=g)
    cl = torch.rand(K, generator=g)
    res = [torch.randn(count, generator=g) for _ in range(K)]
    dout = torch.randn(count, generator=g)
    dlat = 1.7
    lat_on = variant != 'nolat'
    r = sr.sink_ref(betas, res, cl if lat_on else None, dout, sr.f32(dlat) if lat_on else None)
    s = _stream()
    R = [t.cuda() for t in res]
    B, CLd = betas.cuda(), cl.cuda()
    out = torch.full((count + 4,), SENT, device='cuda')
    out_lat = torch.full((1,), SENT, device='cuda')
    bw = torch.full((K + 1,), SENT, device='cuda')
    rc = lib.tfnas_sink_fwd(K, _lib.ptr(B), _lib.ptr_array(R), _lib.ptr(CLd) if lat_on else None, count, _lib.ptr(out),
                            None if variant == 'nobetas' else _lib.ptr(out_lat), _lib.ptr(bw), s)
    assert rc == 0
    torch.cuda.synchronize()
    out_c, bw_c = out.cpu(), bw.cpu()
    rmax = max(float(t.abs().max()) for t in res)
    lim = K * 2 * sr.U * rmax
    err = float(np.abs(sr.d64(out_c[:count]) - r['out']).max())
    assert err <= lim, 'out K %d count %d: %.3e > %.3e' % (K, count, err, lim)
    worst['out'] = max(worst.get('out', 0.0), err / lim)
    assert bool((out_c[count:] == SENT).all()) and float(bw_c[K]) == SENT
    assert float(np.abs(sr.d64(bw_c[:K]) - r['bw']).max()) <= 1e-6
    if variant == 'nobetas':
        assert float(out_lat) == SENT
    else:
        assert abs(float(out_lat) - r['out_lat']) <= 1e-6
        if not lat_on:
            assert float(out_lat) == 0.0
    # backward; bw is an input: the float32 of the reference's, independent of the forward above
    bw_in = torch.from_numpy(r['bw']).float()
    BW, DOUT = bw_in.cuda(), dout.cuda()
    DLAT = torch.tensor([dlat], device='cuda')
    skip = [variant == 'nolat' and k % 2 == 1 for k in range(K)]
    dres = [None if skip[k] else torch.full((count + 4,), SENT, device='cuda') for k in range(K)]
    dbetas = torch.full((K + 1,), SENT, device='cuda')
    dcl = torch.full((K + 1,), SENT, device='cuda')
    dots = torch.full((K + 4,), SENT, dtype=torch.float64, device='cuda')          # double[K], as the header says, then sentinels
    rc = lib.tfnas_sink_bwd(K, _lib.ptr(BW), _lib.ptr_array(R), _lib.ptr(CLd) if lat_on else None, _lib.ptr(DOUT),
                            _lib.ptr(DLAT) if lat_on else None, count, _lib.ptr_array(dres),
                            None if variant == 'nobetas' else _lib.ptr(dbetas), _lib.ptr(dcl) if lat_on else None, _lib.ptr(dots), s)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((dots[K:] == SENT).all()), 'tfnas_sink_bwd wrote past double[K] of dot_scratch'
    d64 = sr.d64(dout)
    for k in range(K):
        if skip[k]:
            continue
        got = dres[k].cpu()
        assert bool((got[count:] == SENT).all())
        ref = float(bw_in[k]) * d64
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        err = np.abs(sr.d64(got[:count]) - ref)
        assert np.all(err <= ulp), 'dres[%d]: %.3e' % (k, float((err / ulp).max()))
        worst['dres'] = max(worst.get('dres', 0.0), float((err / ulp).max()))
    if variant == 'nobetas':
        assert bool((dbetas == SENT).all())
    else:
        absdot = max(float(np.sum(np.abs(d64 * sr.d64(t)))) for t in res)
        lim = 2.0 ** -20 * absdot + 1e-4 * np.abs(r['dbetas'])
        err = np.abs(sr.d64(dbetas.cpu()[:K]) - r['dbetas'])
        assert np.all(err <= lim), 'dbetas K %d count %d: %s vs %s' % (K, count, err, lim)
        worst['dbetas'] = max(worst.get('dbetas', 0.0), float((err / lim).max()))
        assert float(dbetas[K]) == SENT
    if lat_on:
        assert float(np.abs(sr.d64(dcl.cpu()[:K]) - r['dcell_lat']).max()) <= 1e-6
        assert float(dcl[K]) == SENT
    else:
        assert bool((dcl == SENT).all())


@pytest.mark.parametrize('count', [4, 4 * 257, BIG])
def test_sink_fwd_bwd_match_float64(count):
    """out within K * 2 * 2^-24 * max|res|; dres[k] within 1 ulp of bw[k] * dout; out_lat / dcell_lat / bw within 1e-6; dbetas within
    2^-20 * max_k sum|dout res_k| + 1e-4 relative; dot_scratch is double[K] followed by sentinels that must survive."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    worst = {}
    for K in ((1, 4) if count == BIG else (1, 2, 3, 4)):
        for variant in (('full', 'nolat') if count == BIG else ('full', 'nolat', 'nobetas')):
            _sink_case(lib, K, count, 7 * K + count % 1000, variant, worst)
    print('sink count %d: worst error / bound %s' % (count, {k: round(v, 3) for k, v in worst.items()}))


def test_sink_refusals():
    from tfnas_amd import _lib
    lib = _lib.lib()
    x = torch.full((16,), SENT, device='cuda')
    d = torch.full((8,), SENT, dtype=torch.float64, device='cuda')
    arr = _lib.ptr_array([x] * 5)
    for K, count, want in ((0, 8, ERANGE), (5, 8, ERANGE), (2, 6, EINVAL), (4, 9, EINVAL)):
        assert lib.tfnas_sink_fwd(K, _lib.ptr(x), arr, None, count, _lib.ptr(x), None, _lib.ptr(x), _stream()) == want
        assert lib.tfnas_sink_bwd(K, _lib.ptr(x), arr, None, _lib.ptr(x), None, count, arr, _lib.ptr(x), None, _lib.ptr(d), _stream()) == want
    torch.cuda.synchronize()
    assert bool((x == SENT).all()) and bool((d == SENT).all())
