"""GPU: the weight-EMA kernels (csrc/opt_kernels.hip: k_opt_sgd_ema, k_ema_lerp) at the raw C ABI.  tfnas_sgd_clip_ema_step must
leave w' / g' / m' / the norm exactly as tfnas_sgd_clip_step does on the same inputs (that step is pinned against float64 by
test_gpu_opt_kernels.py), and its ema' -- like tfnas_ema_lerp's -- is held to the float64 lerp (tests/_emaref.py) of the GPU's own
fp32 w' and the input ema.  Range sets as in test_gpu_opt_kernels.py (restated here); state is an input of every call, nothing is
chained; every float outside the ranges is a canary in all four buffers and must come back as it went in.

Bound per element: 2 * 2^-24 * (|ema'| + alpha |w' - ema|) -- one rounding of the difference and one of the fma, doubled so that a
multiply followed by an add would pass too (_emaref.lerp_bound).  alpha is the double that the C float argument holds.  Each test
prints its worst error as a fraction of the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import _emaref as er
import _smallref as sr

pytestmark = pytest.mark.gpu

EINVAL, ENULL, ERANGE = -1, -2, -3
CHUNK = 8192
ARENA = 100 * 1024
HYPER = [(0.025, 0.9, 1e-5), (0.2, 0.0, 0.0)]
CLIPS = [0.5, 2.0]                                      # x the float64 gradient norm: clipping / not clipping
ALPHAS = [1e-4, 0.1, 1.0, 0.0]
CANARY = -12345.5


def _u64(vals):
    return (C.c_uint64 * len(vals))(*vals)


def _place(lens, order, gaps, start):
    off, pos = [0] * len(lens), start
    for k, i in enumerate(order):
        off[i] = pos
        pos += lens[i] + gaps[k % len(gaps)]
    assert pos <= ARENA
    return off


def _range_set(name):
    if name == 'A':                                     # chunk edges, listed out of offset order, gaps of 4..64 floats
        lens = [4, 8, 8188, 8192, 8196, 16384, 24580]
        off = _place(lens, [5, 0, 3, 6, 1, 4, 2], [4, 64, 8, 36, 12, 60], 16)
    elif name == 'B':                                   # the 64-range cap
        g = torch.Generator().manual_seed(64)
        lens = [4, 260] + [4 * int(v) for v in torch.randint(1, 66, (62,), generator=g)]
        off = _place(lens, [int(i) for i in torch.randperm(64, generator=g)], [4, 64, 8, 36, 12, 60], 40)
    else:                                               # the retrain shape: one range, many workgroups
        lens, off = [3 * CHUNK + 4], [1000]
    return list(zip(off, lens))


def _nblocks(ranges):
    return sum((n + CHUNK - 1) // CHUNK for _, n in ranges)


def _inside(ranges):
    mask = torch.zeros(ARENA, dtype=torch.bool)
    for o, n in ranges:
        mask[o:o + n] = True
    return mask


_cache = {}


def _arenas(rset):
    """w / g / m / ema (CPU, never modified): random inside the ranges of ``rset``, the canary everywhere else."""
    if rset not in _cache:
        gen = torch.Generator().manual_seed(100)
        w, g, m = torch.randn(ARENA, generator=gen), torch.randn(ARENA, generator=gen) * 0.3, torch.randn(ARENA, generator=gen) * 0.1
        e = w + torch.randn(ARENA, generator=gen) * 0.05                 # an average trails its weights closely
        e[::7] = 0.0                                                     # ... a few exact zeros
        mask = _inside(_range_set(rset))
        for t in (w, g, m, e):
            t[~mask] = CANARY
        _cache[rset] = (w, g, m, e)
    return _cache[rset]


def _gnorm(g, ranges):
    return float(np.sqrt(sum(float((g[o:o + n].double() ** 2).sum()) for o, n in ranges)))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(lib, ranges, w, g, m, max_norm, lr, mom, wd, ema=None, alpha=None):
    from tfnas_amd import _lib
    nb = _nblocks(ranges)
    scratch = torch.empty(nb, dtype=torch.float64, device='cuda')
    norm = torch.full((1,), -1.0, device='cuda')
    off, ln = _u64([o for o, _ in ranges]), _u64([n for _, n in ranges])
    if ema is None:
        rc = lib.tfnas_sgd_clip_step(_lib.ptr(w), _lib.ptr(g), _lib.ptr(m), len(ranges), off, None, ln, max_norm, lr, mom, wd, 1.0,
                                     _lib.ptr(scratch), nb, _lib.ptr(norm), _stream())
    else:
        rc = lib.tfnas_sgd_clip_ema_step(_lib.ptr(w), _lib.ptr(g), _lib.ptr(m), len(ranges), off, None, ln, max_norm, lr, mom, wd,
                                         1.0, _lib.ptr(ema), alpha, _lib.ptr(scratch), nb, _lib.ptr(norm), _stream())
    assert rc == 0
    return norm


def _check_lerp(got, e0, target, alpha, mask, worst):
    """ema' from the device against the float64 lerp of (e0, target) inside ``mask``; bit-identical outside."""
    a = sr.f32(alpha)
    ref = er.lerp_ref(e0, target, a)
    lim = er.lerp_bound(ref, target, e0, a)
    got64 = sr.d64(got)
    mk = mask.numpy()
    assert np.all(np.isfinite(got64[mk]))
    err = np.abs(got64 - ref)
    bad = np.nonzero(mk & (err > lim))[0]
    assert bad.size == 0, 'ema[%d] alpha %g: err %.3e > bound %.3e' % (bad[0], alpha, err[bad[0]], lim[bad[0]])
    assert torch.equal(got[~mask], e0[~mask]), 'ema outside the ranges'
    nz = mk & (lim > 0)
    if nz.any():
        worst[alpha] = max(worst.get(alpha, 0.0), float((err[nz] / lim[nz]).max()))


@pytest.mark.parametrize('rset', ['A', 'B', 'C'])
def test_ema_step_is_the_sgd_step_bit_for_bit_plus_the_float64_lerp(rset):
    from tfnas_amd import _lib
    lib = _lib.lib()
    ranges = _range_set(rset)
    mask = _inside(ranges)
    w0, g0, m0, e0 = _arenas(rset)
    n0 = _gnorm(g0, ranges)
    worst = {}
    for lr, mom, wd in HYPER:
        for clip in CLIPS:
            max_norm = clip * n0
            w1, g1, m1 = w0.cuda(), g0.cuda(), m0.cuda()
            n1 = _call(lib, ranges, w1, g1, m1, max_norm, lr, mom, wd)
            torch.cuda.synchronize()
            w1, g1, m1, n1 = w1.cpu(), g1.cpu(), m1.cpu(), n1.cpu()
            assert (float(n1) > max_norm) == (clip < 1.0)                # the two regimes are what they are meant to be
            for t, t0 in ((w1, w0), (g1, g0), (m1, m0)):
                assert torch.equal(t[~mask], t0[~mask])
            assert not torch.equal(w1[mask], w0[mask])
            for alpha in ALPHAS:
                w2, g2, m2, e2 = w0.cuda(), g0.cuda(), m0.cuda(), e0.cuda()
                n2 = _call(lib, ranges, w2, g2, m2, max_norm, lr, mom, wd, e2, alpha)
                torch.cuda.synchronize()
                w2, g2, m2, e2 = w2.cpu(), g2.cpu(), m2.cpu(), e2.cpu()
                assert torch.equal(w2, w1) and torch.equal(g2, g1) and torch.equal(m2, m1) and torch.equal(n2.cpu(), n1)
                if alpha == 0.0:
                    assert torch.equal(e2, e0)                           # bit-identical: fma(0, d, e) = e
                _check_lerp(e2, e0, w2, alpha, mask, worst)
    print('sgd_clip_ema_step %s: worst ema error / bound per alpha %s' % (rset, {k: round(v, 3) for k, v in worst.items()}))
    assert set(worst) >= {1e-4, 0.1, 1.0}


@pytest.mark.parametrize('rset', ['A', 'B', 'C'])
def test_ema_step_gives_identical_bits_twice(rset):
    from tfnas_amd import _lib
    lib = _lib.lib()
    ranges = _range_set(rset)
    w0, g0, m0, e0 = _arenas(rset)
    lr, mom, wd = HYPER[0]
    max_norm = 0.5 * _gnorm(g0, ranges)
    runs = []
    for _ in range(2):
        w, g, m, e = w0.cuda(), g0.cuda(), m0.cuda(), e0.cuda()
        n = _call(lib, ranges, w, g, m, max_norm, lr, mom, wd, e, 0.1)
        torch.cuda.synchronize()
        runs.append((w, g, m, e, n))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][3].cpu(), e0)


@pytest.mark.parametrize('rset', ['A', 'B'])
def test_ema_lerp_alone(rset):
    from tfnas_amd import _lib
    lib = _lib.lib()
    ranges = _range_set(rset)
    mask = _inside(ranges)
    w0, _, _, e0 = _arenas(rset)
    off, ln = _u64([o for o, _ in ranges]), _u64([n for _, n in ranges])
    worst = {}
    for alpha in ALPHAS:
        src, e = w0.cuda(), e0.cuda()
        assert lib.tfnas_ema_lerp(_lib.ptr(e), _lib.ptr(src), len(ranges), off, ln, alpha, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(src.cpu(), w0)                                # src is only read
        e = e.cpu()
        if alpha == 0.0:
            assert torch.equal(e, e0)
        _check_lerp(e, e0, w0, alpha, mask, worst)
    print('ema_lerp %s: worst error / bound per alpha %s' % (rset, {k: round(v, 3) for k, v in worst.items()}))
    assert set(worst) >= {1e-4, 0.1, 1.0}


def test_ema_refusals_touch_nothing():
    from tfnas_amd import _lib
    lib = _lib.lib()
    w0, g0, m0, e0 = _arenas('C')
    n = 2 * CHUNK
    w, g, m, e = w0[:n].cuda(), g0[:n].cuda(), m0[:n].cuda(), e0[:n].cuda()
    scratch = torch.full((8,), -1.0, dtype=torch.float64, device='cuda')
    s = _stream()

    def step(ema=e, alpha=0.1, off=(64, 512, 1024), ln=(64, 128, 512)):
        return lib.tfnas_sgd_clip_ema_step(_lib.ptr(w), _lib.ptr(g), _lib.ptr(m), len(off), _u64(off), None, _u64(ln), 5.0, 0.025,
                                           0.9, 1e-5, 1.0, _lib.ptr(ema), alpha, _lib.ptr(scratch), 8, None, s)

    def lerp(ema=e, src=w, alpha=0.1, off=(64, 512, 1024), ln=(64, 128, 512)):
        return lib.tfnas_ema_lerp(_lib.ptr(ema), _lib.ptr(src), len(off), _u64(off), _u64(ln), alpha, s)

    assert step(ema=None) == ENULL and lerp(ema=None) == ENULL and lerp(src=None) == ENULL
    for bad in (-0.1, 1.5, float('nan')):
        assert step(alpha=bad) == EINVAL and lerp(alpha=bad) == EINVAL
    assert step(ema=w) == EINVAL and step(ema=g) == EINVAL and step(ema=m) == EINVAL and lerp(ema=w) == EINVAL
    assert step(off=(64, 100, 1024)) == EINVAL and lerp(off=(64, 100, 1024)) == EINVAL
    assert step(ln=(64, 126, 512)) == EINVAL and lerp(ln=(64, 0, 512)) == EINVAL
    assert step(off=tuple(4 * i for i in range(65)), ln=(4,) * 65) == ERANGE
    torch.cuda.synchronize()
    assert torch.equal(w.cpu(), w0[:n]) and torch.equal(g.cpu(), g0[:n]) and torch.equal(m.cpu(), m0[:n])
    assert torch.equal(e.cpu(), e0[:n]) and bool((scratch == -1.0).all())
