"""GPU: the fused optimizer kernels (csrc/opt_kernels.hip) at the raw C ABI against the float64 restatements of _smallref.py
(themselves pinned to torch's float64 optimizers by test_small_refs.py): tfnas_sgd_clip_step and tfnas_pack_ranges on range sets
around the 8192-float chunk, with carried momentum, every clip regime, grad_scale != 1 and the packed-message route;
tfnas_arch_adam_project with carried moments at step > 1.  State is an input of every call: no steps are chained.

Bounds.  SGD: element-wise, see _smallref.sgd_bounds (16 * 2^-24 * (|g'| + wd |w| + mom |m|) for m' and g'; 2 * 2^-24 |w'| + lr * that
for w'); the norm within 4 * 2^-24 relative.  Adam: m' / v' within 8 * 2^-24 of the summed magnitudes of their two terms, p' within
2e-6 absolute, the norm within 8 * 2^-24 relative.  Each test prints its worst error as a fraction of the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import _smallref as sr

pytestmark = pytest.mark.gpu

EINVAL, ENULL, ERANGE = -1, -2, -3
CHUNK = 8192
ARENA = 100 * 1024
HYPER = [(0.025, 0.9, 1e-5), (0.2, 0.0, 0.0)]           # the project's (train_search.py) / a plain large step
SCALES = [1.0, 0.5, 1.0 / 3.0]
CLIPS = [0.5, 2.0, 1.0 + 1e-3, 1.0 - 1e-3, 0.0, -1.0]   # x the float64 norm of the scaled gradient; <= 0: clipping off


def _u64(vals):
    return (C.c_uint64 * len(vals))(*vals)


def _place(lens, order, gaps, start):
    """Offsets for ranges of ``lens`` laid out in ``order`` with ``gaps`` floats between them -- returned in the order of
    ``lens``, i.e. not ascending."""
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


_cache = {}


def _arenas():
    """Distinct random w / g / m (CPU, never modified)."""
    if 'arenas' not in _cache:
        g = torch.Generator().manual_seed(100)
        _cache['arenas'] = (torch.randn(ARENA, generator=g), torch.randn(ARENA, generator=g) * 0.3, torch.randn(ARENA, generator=g) * 0.1)
    return _cache['arenas']


def _gnorm(g, ranges):
    return float(np.sqrt(sum(float((g[o:o + n].double() ** 2).sum()) for o, n in ranges)))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _step(lib, w, g, m, ranges, goff, max_norm, lr, mom, wd, gs, want_norm=True, scratch=None):
    """One tfnas_sgd_clip_step on device tensors (in place); scratch: exactly sum ceil(len / 8192) doubles."""
    from tfnas_amd import _lib
    nb = _nblocks(ranges)
    scratch = torch.empty(nb, dtype=torch.float64, device='cuda') if scratch is None else scratch
    norm = torch.full((1,), -1.0, device='cuda') if want_norm else None
    rc = lib.tfnas_sgd_clip_step(_lib.ptr(w), _lib.ptr(g), _lib.ptr(m), len(ranges), _u64([o for o, _ in ranges]),
                                 None if goff is None else _u64(goff), _u64([n for _, n in ranges]), max_norm, lr, mom, wd, gs,
                                 _lib.ptr(scratch), nb, _lib.ptr(norm), _stream())
    return rc, norm


def _check_step(w0, g0, m0, ranges, out, max_norm, lr, mom, wd, gs, worst):
    """(w, g, m, norm) from the device against the float64 reference: element-wise bounds, bit-identical outside the ranges."""
    w, g, m, norm = out
    hp = [sr.f32(v) for v in (max_norm, lr, mom, wd, gs)]
    w_ref, g_ref, m_ref, tot = sr.sgd_clip_ref(w0, g0, m0, ranges, None, *hp)
    bm, bw = sr.sgd_bounds(w0, g_ref, m0, w_ref, ranges, None, hp[1], hp[2], hp[3])
    inside = np.zeros(ARENA, dtype=bool)
    for o, n in ranges:
        inside[o:o + n] = True
    for name, got, ref, lim, old in (('w', w, w_ref, bw, w0), ('m', m, m_ref, bm, m0), ('g', g, g_ref, bm, g0)):
        got = sr.d64(got)
        assert np.all(np.isfinite(got)), name
        err = np.abs(got - ref)
        bad = np.nonzero(err > lim)[0]
        assert bad.size == 0, '%s[%d]: err %.3e > bound %.3e' % (name, bad[0], err[bad[0]], lim[bad[0]])
        assert torch.equal(torch.from_numpy(got[~inside]), old.double()[~torch.from_numpy(inside)]), name + ' outside the ranges'
        nz = lim > 0
        if nz.any():
            worst[name] = max(worst.get(name, 0.0), float((err[nz] / lim[nz]).max()))
    if norm is not None:
        assert abs(float(norm) - tot) <= 4 * sr.U * tot, (float(norm), tot)
        if tot > 0:
            worst['norm'] = max(worst.get('norm', 0.0), float(abs(float(norm) - tot) / (4 * sr.U * tot)))


@pytest.mark.parametrize('rset', ['A', 'B', 'C'])
def test_sgd_clip_step_matches_float64(rset):
    """Every (hyper-parameters, grad_scale, clip regime) on one range set, each a separate call from the same carried state."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    ranges = _range_set(rset)
    w0, g0, m0 = _arenas()
    worst = {}
    for lr, mom, wd in HYPER:
        for gs in SCALES:
            n0 = _gnorm(g0, ranges) * sr.f32(gs)
            for k, clip in enumerate(CLIPS):
                max_norm = clip * n0 if clip > 0 else clip
                w, g, m = w0.cuda(), g0.cuda(), m0.cuda()
                rc, norm = _step(lib, w, g, m, ranges, None, max_norm, lr, mom, wd, gs, want_norm=(k % 3 != 2))   # norm_out NULL too
                assert rc == 0
                torch.cuda.synchronize()
                _check_step(w0, g0, m0, ranges, (w.cpu(), g.cpu(), m.cpu(), None if norm is None else norm.cpu()),
                            max_norm, lr, mom, wd, gs, worst)
    print('sgd_clip_step %s: worst error / bound %s' % (rset, {k: round(v, 3) for k, v in worst.items()}))
    assert set(worst) >= {'w', 'm', 'g', 'norm'}


@pytest.mark.parametrize('rset', ['A', 'B', 'C'])
def test_sgd_clip_step_is_deterministic_and_survives_zero_and_tiny_gradients(rset):
    from tfnas_amd import _lib
    lib = _lib.lib()
    ranges = _range_set(rset)
    w0, g0, m0 = _arenas()
    lr, mom, wd = HYPER[0]
    max_norm = 0.5 * _gnorm(g0, ranges)
    runs = []
    for _ in range(2):
        w, g, m = w0.cuda(), g0.cuda(), m0.cuda()
        rc, norm = _step(lib, w, g, m, ranges, None, max_norm, lr, mom, wd, 1.0)
        assert rc == 0
        torch.cuda.synchronize()
        runs.append((w, g, m, norm))
    for a, b in zip(*runs):
        assert torch.equal(a, b)                         # the header promises determinism
    worst = {}
    for (lr, mom, wd), max_norm in ((HYPER[0], 5.0), (HYPER[1], 5.0), (HYPER[0], 0.0)):
        gz = g0.clone()
        for o, n in ranges:
            gz[o:o + n] = 0
        w, g, m = w0.cuda(), gz.cuda(), m0.cuda()
        rc, norm = _step(lib, w, g, m, ranges, None, max_norm, lr, mom, wd, 0.5)
        assert rc == 0
        torch.cuda.synchronize()
        assert float(norm) == 0.0
        _check_step(w0, gz, m0, ranges, (w.cpu(), g.cpu(), m.cpu(), norm.cpu()), max_norm, lr, mom, wd, 0.5, worst)
    # a small gradient (norm ~ 1e-2), clipped: here the 1e-6 of clip_grad_norm_'s coefficient is 1e-4 of the result
    gt = g0 * 1e-3
    lr, mom, wd = HYPER[1]
    max_norm = 0.5 * _gnorm(gt, ranges)
    w, g, m = w0.cuda(), gt.cuda(), m0.cuda()
    rc, norm = _step(lib, w, g, m, ranges, None, max_norm, lr, mom, wd, 1.0)
    assert rc == 0
    torch.cuda.synchronize()
    _check_step(w0, gt, m0, ranges, (w.cpu(), g.cpu(), m.cpu(), norm.cpu()), max_norm, lr, mom, wd, 1.0, worst)


@pytest.mark.parametrize('rset', ['A', 'B', 'C'])
def test_packed_route_is_bit_identical_to_the_in_place_route(rset):
    """tfnas_pack_ranges into a sentinel-filled message, then the step reading (and clipping) the message through goff."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    ranges = _range_set(rset)
    w0, g0, m0 = _arenas()
    off, lens = [o for o, _ in ranges], [n for _, n in ranges]
    goff, pos = [], 8
    for k, n in enumerate(lens):                         # packed, with a few 4-float holes that must keep their sentinel
        goff.append(pos)
        pos += n + (4 if k % 3 == 0 else 0)
    SENT = -12345.5
    msg = torch.full((pos + 8,), SENT, device='cuda')
    g_dev = g0.cuda()
    assert lib.tfnas_pack_ranges(_lib.ptr(g_dev), _lib.ptr(msg), len(ranges), _u64(off), _u64(goff), _u64(lens), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(g_dev.cpu(), g0)
    packed = msg.cpu()
    hole = torch.ones(len(packed), dtype=torch.bool)
    for q, (o, n) in zip(goff, ranges):
        assert torch.equal(packed[q:q + n], g0[o:o + n])
        hole[q:q + n] = False
    assert bool((packed[hole] == SENT).all())
    for (lr, mom, wd), gs, clip in ((HYPER[0], 0.5, 0.5), (HYPER[1], 1.0 / 3.0, 2.0)):
        max_norm = clip * _gnorm(g0, ranges) * sr.f32(gs)
        w1, g1, m1 = w0.cuda(), g0.cuda(), m0.cuda()
        rc1, n1 = _step(lib, w1, g1, m1, ranges, None, max_norm, lr, mom, wd, gs)
        w2, g2, m2, msg2 = w0.cuda(), g0.cuda(), m0.cuda(), msg.clone()
        rc2, n2 = _step(lib, w2, msg2, m2, ranges, goff, max_norm, lr, mom, wd, gs)
        assert rc1 == 0 and rc2 == 0
        torch.cuda.synchronize()
        assert torch.equal(w1, w2) and torch.equal(m1, m2) and torch.equal(n1, n2)
        # (the step was handed the message as g: the arena's own gradient buffer was not passed and cannot have changed)
        out = msg2.cpu()
        g1 = g1.cpu()
        for q, (o, n) in zip(goff, ranges):
            assert torch.equal(out[q:q + n], g1[o:o + n])    # the clipped gradient is left in the message
        assert bool((out[hole] == SENT).all())
        # the same through the reference: w' / m' of the packed route against float64
        worst = {}
        _check_step(w0, g0, m0, ranges, (w2.cpu(), g1, m2.cpu(), n2.cpu()), max_norm, lr, mom, wd, gs, worst)


def test_sgd_and_pack_refusals_touch_nothing():
    from tfnas_amd import _lib
    lib = _lib.lib()
    w0, g0, m0 = _arenas()
    n = 2 * CHUNK                                                    # (every refused range still lies inside the buffers)
    w, g, m = w0[:n].cuda(), g0[:n].cuda(), m0[:n].cuda()
    dst = torch.full((n,), 3.25, device='cuda')
    scratch = torch.full((8,), -1.0, dtype=torch.float64, device='cuda')
    good = ([64, 512, 1024], [0, 128, 640], [64, 128, 512])          # off, goff, len: disjoint, multiples of 4
    s = _stream()

    def step(off, goff, ln, nr=None, sd=3, ptrs=None, null_off=False, null_len=False):
        p = dict(w=w, g=g, m=m, scratch=scratch)
        p.update(ptrs or {})
        return lib.tfnas_sgd_clip_step(_lib.ptr(p['w']), _lib.ptr(p['g']), _lib.ptr(p['m']), len(off) if nr is None else nr,
                                       None if null_off else _u64(off), None if goff is None else _u64(goff),
                                       None if null_len else _u64(ln), 5.0, 0.025, 0.9, 1e-5, 1.0, _lib.ptr(p['scratch']), sd, None, s)

    def pack(off, doff, ln, nr=None, src=g, to=dst, null=None):
        a = dict(off=_u64(off), doff=_u64(doff), ln=_u64(ln))
        if null:
            a[null] = None
        return lib.tfnas_pack_ranges(_lib.ptr(src), _lib.ptr(to), len(off) if nr is None else nr, a['off'], a['doff'], a['ln'], s)

    def swap(which, i, v):
        t = [list(x) for x in good]
        t[which][i] = v
        return t

    many = ([4 * i for i in range(65)], [4 * i for i in range(65)], [4] * 65)
    cases = [
        (ERANGE, step(*good, nr=0), pack(*good, nr=0)),
        (ERANGE, step(*many), pack(*many)),                                           # the 64-range cap
        (EINVAL, step(*swap(0, 1, 514)), pack(*swap(0, 1, 514))),                     # off not a multiple of 4
        (EINVAL, step(*swap(1, 2, 642)), pack(*swap(1, 2, 642))),                     # goff / doff not a multiple of 4
        (EINVAL, step(*swap(2, 0, 62)), pack(*swap(2, 0, 62))),                       # len not a multiple of 4
        (EINVAL, step(*swap(2, 1, 0)), pack(*swap(2, 1, 0))),                         # len == 0
        (EINVAL, step(*swap(0, 1, 100)), pack(*swap(0, 1, 100))),                     # off ranges overlap: [64,128) and [100,228)
        (EINVAL, step(*swap(0, 2, 576)), pack(*swap(0, 2, 576))),                     # ... by their last 64 floats: [512,640) [576,1088)
        (EINVAL, step(*swap(1, 1, 60)), pack(*swap(1, 1, 60))),                       # goff / doff ranges overlap: [0,64) and [60,188)
        (EINVAL, step([64, 512, 512], None, good[2]), None),                          # the same range twice, goff NULL
        (ERANGE, step(*good, sd=2), None),                                            # scratch one double short
        (ERANGE, step([0], None, [CHUNK + 4], sd=1), None),
        (ENULL, step(*good, ptrs=dict(w=None)), pack(*good, src=None)),
        (ENULL, step(*good, ptrs=dict(g=None)), pack(*good, to=None)),
        (ENULL, step(*good, ptrs=dict(m=None)), pack(*good, null='off')),
        (ENULL, step(*good, ptrs=dict(scratch=None)), pack(*good, null='doff')),
        (ENULL, step(*good, null_off=True), pack(*good, null='ln')),
        (ENULL, step(*good, null_len=True), None),
    ]
    for k, (want, rs, rp) in enumerate(cases):
        assert rs == want, 'step refusal %d: %d, expected %d' % (k, rs, want)
        assert rp is None or rp == want, 'pack refusal %d: %d, expected %d' % (k, rp, want)
    torch.cuda.synchronize()                                                          # clean: nothing was launched
    assert torch.equal(w.cpu(), w0[:n]) and torch.equal(g.cpu(), g0[:n]) and torch.equal(m.cpu(), m0[:n])
    assert bool((dst == 3.25).all()) and bool((scratch == -1.0).all())
    assert step([64, 512, 1024], None, [64, 512, 512]) == 0                           # ranges that only touch are disjoint
    assert pack([64, 512, 1024], [0, 64, 576], [64, 512, 512]) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ tfnas_arch_adam_project
ADAM = dict(lr=0.01, b1=0.5, b2=0.999, eps=1e-8)                     # train_search.py:414-422
LENS = {1: [5], 24: [8] * 18 + [2, 3, 4, 4, 4, 1], 32: [8] * 18 + [2, 3, 4, 4, 4, 1] + [1, 2, 3, 4, 5, 6, 7, 8]}
SENT = -777.125


def _adam_state(n, seed):
    """p (log_softmax rows), g, and carried moments consistent with an Adam history (|m| <~ sqrt(v): the step stays a few lr, as
    in a real run, so that the 2e-6 absolute bound on p' speaks about rounding and not about an amplified ratio); a few elements
    with m = v = g = 0.  Everything lives in sentinel-padded [n + 2][8] buffers; rows >= n are sentinels."""
    lens = LENS[n]
    gen = torch.Generator().manual_seed(seed)
    P, G, M, V = (torch.full((n + 2, 8), SENT) for _ in range(4))
    for i, k in enumerate(lens):
        P[i, :k] = torch.log_softmax(torch.randn(k, generator=gen), -1)
        G[i, :k] = torch.randn(k, generator=gen) * 0.2
        M[i, :k] = torch.randn(k, generator=gen) * 0.1
        V[i, :k] = (M[i, :k] ** 2 + 0.01 * torch.rand(k, generator=gen)) * (0.5 + 1.5 * torch.rand(k, generator=gen))
    for i in range(0, n, 5):
        j = i % lens[i]
        G[i, j] = M[i, j] = V[i, j] = 0.0
    return lens, P, G, M, V


def _adam_call(lib, n, lens, P, G, M, V, max_norm, wd, step, gs, norm, p_ptrs=None, g_ptrs=None, lens_arg=None, n_arg=None):
    from tfnas_amd import _lib
    pp = [P[i].data_ptr() for i in range(n)] if p_ptrs is None else p_ptrs
    gp = [G[i].data_ptr() for i in range(n)] if g_ptrs is None else g_ptrs
    ln = lens if lens_arg is None else lens_arg
    return lib.tfnas_arch_adam_project(n if n_arg is None else n_arg, _lib.raw_array(pp), _lib.raw_array(gp), (C.c_int32 * len(ln))(*ln),
                                       _lib.ptr(M), _lib.ptr(V), max_norm, ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], wd, step,
                                       gs, _lib.ptr(norm), _stream())


@pytest.mark.parametrize('n', [1, 24, 32])
def test_arch_adam_project_matches_float64(n):
    """step in {1, 2, 7, 1000, 100000} x clip active / inactive / disabled x grad_scale {1, 1/3} x wd {5e-4, 0}, carried random
    moments each time."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    worst = {}
    for si, step in enumerate((1, 2, 7, 1000, 100000)):
        lens, P0, G0, M0, V0 = _adam_state(n, 10 * n + si)
        live = torch.zeros(n + 2, 8, dtype=torch.bool)
        for i, k in enumerate(lens):
            live[i, :k] = True
        for clip in (0.5, 2.0, 0.0):
            for gs in (1.0, 1.0 / 3.0):
                for wd in (5e-4, 0.0):
                    n0 = float(G0[live].double().norm()) * sr.f32(gs)
                    max_norm = clip * n0
                    P, G, M, V = P0.cuda(), G0.cuda(), M0.cuda(), V0.cuda()
                    norm = torch.full((1,), -1.0, device='cuda')
                    assert _adam_call(lib, n, lens, P, G, M, V, max_norm, wd, step, gs, norm) == 0
                    torch.cuda.synchronize()
                    P, M, V = P.cpu(), M.cpu(), V.cpu()
                    hp = [sr.f32(v) for v in (max_norm, ADAM['lr'], ADAM['b1'], ADAM['b2'], ADAM['eps'], wd)]
                    p_ref, m_ref, v_ref, tot, terms = sr.adam_project_ref(
                        [P0[i, :k] for i, k in enumerate(lens)], [G0[i, :k] for i, k in enumerate(lens)], M0, V0, *hp, step, sr.f32(gs))
                    for name, got, ref, (ta, tb), old in (('m', M, m_ref, terms[:2], M0), ('v', V, v_ref, terms[2:], V0)):
                        lim = 8 * sr.U * (np.abs(ta) + np.abs(tb))
                        err = np.abs(sr.d64(got) - ref)[live.numpy()]
                        lim = lim[live.numpy()]
                        assert np.all(err <= lim), '%s step %d clip %g gs %g wd %g: worst %.3f of the bound' % (
                            name, step, clip, gs, wd, float((err / np.maximum(lim, 1e-300)).max()))
                        nz = lim > 0
                        worst[name] = max(worst.get(name, 0.0), float((err[nz] / lim[nz]).max()))
                        assert torch.equal(got[~live], old[~live])           # padding and the rows >= n: bit-identical sentinels
                    assert torch.equal(P[~live], P0[~live])
                    for i, k in enumerate(lens):
                        err = float(np.abs(sr.d64(P[i, :k]) - p_ref[i]).max())
                        assert err <= 2e-6, 'p[%d] step %d: %.3e' % (i, step, err)
                        worst['p'] = max(worst.get('p', 0.0), err / 2e-6)
                        assert abs(float(torch.logsumexp(P[i, :k].double(), 0))) <= 1e-5
                        if k == 1:
                            assert float(P[i, 0]) == 0.0                      # a length-1 tensor projects to exactly 0
                    assert abs(float(norm) - tot) <= 8 * sr.U * tot
                    worst['norm'] = max(worst.get('norm', 0.0), float(abs(float(norm) - tot) / (8 * sr.U * tot)))
    print('arch_adam_project n=%d: worst error / bound %s' % (n, {k: round(v, 3) for k, v in worst.items()}))


def test_arch_adam_project_refusals_write_nothing():
    from tfnas_amd import _lib
    lib = _lib.lib()
    n = 24
    lens, P0, G0, M0, V0 = _adam_state(n, 5)
    P, G, M, V = P0.cuda(), G0.cuda(), M0.cuda(), V0.cuda()
    norm = torch.full((1,), -1.0, device='cuda')
    ptrs = [P[i].data_ptr() for i in range(n)]
    gptrs = [G[i].data_ptr() for i in range(n)]
    call = lambda **kw: _adam_call(lib, n, lens, P, G, M, V, 5.0, 5e-4, kw.pop('step', 3), 1.0, norm, **kw)
    big = ptrs + ptrs[:9]
    assert call(n_arg=0) == ERANGE
    assert call(n_arg=33, p_ptrs=big, g_ptrs=big, lens_arg=[8] * 33) == ERANGE
    assert call(lens_arg=lens[:7] + [0] + lens[8:]) == ERANGE
    assert call(lens_arg=lens[:23] + [9]) == ERANGE
    assert call(step=0) == EINVAL
    assert call(p_ptrs=ptrs[:5] + [None] + ptrs[6:]) == ENULL
    assert call(g_ptrs=gptrs[:23] + [None]) == ENULL
    torch.cuda.synchronize()
    assert torch.equal(P.cpu(), P0) and torch.equal(M.cpu(), M0) and torch.equal(V.cpu(), V0) and float(norm) == -1.0
