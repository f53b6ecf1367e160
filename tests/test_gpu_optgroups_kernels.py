"""GPU: tfnas_opt_groups_step (csrc/opt_kernels.hip: k_opt_groups) at the raw C ABI against the float64 restatements and the
element-wise bounds of tests/_optref.py (proved on the CPU by tests/test_optref.py).  The arena is 3 * 8192 + 5 * 64 floats: a
ragged last chunk, group boundaries inside a chunk and exactly on a chunk boundary; zero "gaps" as between arena slots; canaries
behind the end.  State is an input of every call: no steps are chained.  Each test prints its worst error as a fraction of the
bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import _optref as oref
import _smallref as sr

pytestmark = pytest.mark.gpu

EINVAL, ENULL, ERANGE = -1, -2, -3
TOTAL = oref.TOTAL
TAIL = 256                         # canary floats behind every arena
SENT = -4321.5
EMA_ALPHA = 0.01

_cache = {}


def _state():
    if 'state' not in _cache:
        _cache['state'] = oref.make_state(TOTAL, 7)
    return _cache['state']


def _dev(t):
    """The arena on the device with TAIL canary floats behind it; the first TOTAL floats are what the library is handed."""
    buf = torch.full((TOTAL + TAIL,), SENT, device='cuda')
    buf[:TOTAL] = t.cuda()
    return buf


def _desc(kind, nesterov, ng, lr, wd, mom, alpha, eps, max_norm, gs, ema_alpha=0.0):
    from tfnas_amd import _lib
    d = _lib.TfnasOptGroups()
    d.kind, d.flags, d.ngroups = kind, (_lib.OPT_NESTEROV if nesterov else 0), ng
    for k in range(min(ng, 8)):
        d.lr[k], d.wd[k] = lr[k], wd[k]
    d.momentum, d.alpha, d.eps, d.max_norm, d.grad_scale, d.ema_alpha = mom, alpha, eps, max_norm, gs, ema_alpha
    return d


def _call(d, w, g, m, v, ema, gmap, total=TOTAL, scratch='own', nd=None, norm=None):
    from tfnas_amd import _lib
    nb = (total + 8191) // 8192
    scratch = torch.empty(max(nb, 1), dtype=torch.float64, device='cuda') if isinstance(scratch, str) else scratch
    return _lib.lib().tfnas_opt_groups_step(C.byref(d) if d is not None else None, _lib.ptr(w), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v),
                                            _lib.ptr(ema), _lib.ptr(gmap), total, _lib.ptr(scratch), nb if nd is None else nd,
                                            _lib.ptr(norm), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _run(row, gmap_np, ng, clip, gs, with_ema, g0=None, state=None):
    """One call from the shared state; returns (device results on the CPU, reference, bounds)."""
    name, kind, nesterov, mom = row
    w0, gg, m0, v0, e0, gap = state or _state()
    g0 = gg if g0 is None else g0
    n0 = float(g0.double().norm()) * sr.f32(gs)
    max_norm = clip * n0 if n0 > 0 else 5.0
    lr, wd = oref.LR[:ng], oref.WD[:ng]
    d = _desc(kind, nesterov, ng, lr, wd, mom, oref.ALPHA, oref.EPS, max_norm, gs, EMA_ALPHA)
    w, g, m, v, e = _dev(w0), _dev(g0), _dev(m0), (_dev(v0) if kind != oref.SGD else None), (_dev(e0) if with_ema else None)
    norm = torch.full((1,), -1.0, device='cuda')
    rc = _call(d, w, g, m, v, e, torch.from_numpy(gmap_np).cuda(), norm=norm)
    assert rc == 0
    torch.cuda.synchronize()
    got = dict(w=w.cpu(), g=g.cpu(), m=m.cpu(), v=None if v is None else v.cpu(), ema=None if e is None else e.cpu(), norm=float(norm))
    hp = dict(lr=[sr.f32(x) for x in lr], wd=[sr.f32(x) for x in wd], mom=sr.f32(mom), alpha=sr.f32(oref.ALPHA), eps=sr.f32(oref.EPS),
              max_norm=sr.f32(max_norm), grad_scale=sr.f32(gs), nesterov=nesterov)
    vin = v0 if kind != oref.SGD else None
    ein = dict(ema=e0, ema_alpha=sr.f32(EMA_ALPHA)) if with_ema else {}
    ref = oref.groups_ref(kind, w0, g0, m0, vin, gmap_np, **hp, **ein)
    lim = oref.groups_bounds(kind, ref, w0, m0, vin, hp['mom'], hp['alpha'], hp['eps'], nesterov, **ein)
    return got, ref, lim


def _check(got, ref, lim, worst, gap):
    for k in ('w', 'g', 'm', 'v', 'ema'):
        if got[k] is None:
            continue
        full = got[k]
        assert bool((full[TOTAL:] == SENT).all()), k + ': canaries behind the arena'
        val = sr.d64(full[:TOTAL])
        assert np.all(np.isfinite(val)), k
        err = np.abs(val - ref[k])
        bad = np.nonzero(err > lim[k])[0]
        assert bad.size == 0, '%s[%d]: err %.3e > bound %.3e (%d elements)' % (k, bad[0], err[bad[0]], lim[k][bad[0]], bad.size)
        assert np.all(val[gap.numpy()] == 0.0), k + ': the gaps stay zero'
        nz = lim[k] > 0
        if nz.any():
            worst[k] = max(worst.get(k, 0.0), float((err[nz] / lim[k][nz]).max()))
    tot = ref['total']
    assert abs(got['norm'] - tot) <= 4 * sr.U * tot, (got['norm'], tot)
    if tot > 0:
        worst['norm'] = max(worst.get('norm', 0.0), abs(got['norm'] - tot) / (4 * sr.U * tot))


@pytest.mark.parametrize('row', oref.KINDS, ids=lambda r: '%s-%g' % (r[0], r[3]))
def test_groups_step_matches_float64(row):
    """Every map x (clip below / above the norm, grad_scale 1 / 0.5) x with / without the EMA, each a separate call."""
    worst = {}
    gap = _state()[5]
    for mname, (gmap, ng) in oref.maps().items():
        for clip, gs in ((0.5, 1.0), (2.0, 0.5)):
            for with_ema in (False, True):
                got, ref, lim = _run(row, gmap, ng, clip, gs, with_ema)
                _check(got, ref, lim, worst, gap)
    print('opt_groups_step %s mom %g: worst error / bound %s' % (row[0], row[3], {k: round(x, 3) for k, x in worst.items()}))
    assert set(worst) >= {'w', 'g', 'norm', 'ema'}


@pytest.mark.parametrize('row', oref.KINDS, ids=lambda r: '%s-%g' % (r[0], r[3]))
def test_equal_inputs_give_equal_bits_and_a_255_block_is_left_alone(row):
    gmap, ng = oref.maps()['interleaved']
    a, _, _ = _run(row, gmap, ng, 0.5, 1.0, True)
    b, _, _ = _run(row, gmap, ng, 0.5, 1.0, True)
    for k in ('w', 'g', 'm', 'v', 'ema'):
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    assert a['norm'] == b['norm']
    # blocks 5 (inside a chunk), 127 / 128 (either side of a chunk boundary) and the last one switched off: not in the table
    off = gmap.copy()
    blocks = [5, 127, 128, TOTAL // 64 - 1]
    off[blocks] = 255
    w0, g0, m0, v0, e0, gap = _state()
    got, ref, lim = _run(row, off, ng, 0.5, 1.0, True)
    worst = {}
    _check(got, ref, lim, worst, gap)
    for b_ in blocks:
        s = slice(64 * b_, 64 * b_ + 64)
        assert torch.equal(got['w'][s], w0[s]) and torch.equal(got['m'][s], m0[s]) and torch.equal(got['ema'][s], e0[s])
        assert got['v'] is None or torch.equal(got['v'][s], v0[s])
        assert not torch.equal(got['g'][s], g0[s])                               # the gradient is still clipped there
    assert abs(got['norm'] - a['norm']) <= 4 * sr.U * a['norm']                    # ... and still counts in the norm


@pytest.mark.parametrize('row', oref.KINDS, ids=lambda r: '%s-%g' % (r[0], r[3]))
def test_zero_gradients_give_a_finite_result(row):
    gmap, ng = oref.maps()['interleaved']
    w0, g0, m0, v0, e0, gap = _state()
    got, ref, lim = _run(row, gmap, ng, 0.5, 0.5, True, g0=torch.zeros_like(g0))
    assert got['norm'] == 0.0
    _check(got, ref, lim, {}, gap)
    # ... and with an all-zero squared-gradient average as well (the first step of torch's RMSprop): 0 / (sqrt(0) + eps)
    zs = (w0, g0, m0, torch.zeros_like(v0), e0, gap)
    got, ref, lim = _run(row, gmap, ng, 0.5, 0.5, True, g0=torch.zeros_like(g0), state=zs)
    _check(got, ref, lim, {}, gap)


def test_refusals_return_their_code_and_touch_nothing():
    from tfnas_amd import _lib
    w0, g0, m0, v0, e0, _ = _state()
    w, g, m, v, e = _dev(w0), _dev(g0), _dev(m0), _dev(v0), _dev(e0)
    gmap_np, ng = oref.maps()['interleaved']
    gmap = torch.from_numpy(gmap_np).cuda()
    scratch = torch.full((8,), -1.0, dtype=torch.float64, device='cuda')
    norm = torch.full((1,), -1.0, device='cuda')
    nan, inf = float('nan'), float('inf')

    def desc(kind=oref.RMSPROP, nesterov=False, ng=2, lr=oref.LR, wd=oref.WD, mom=0.9, alpha=0.9, eps=1e-3, max_norm=5.0, gs=1.0,
             ema_alpha=0.01, flags=None):
        d = _desc(kind, nesterov, ng, list(lr) + [0.0] * 8, list(wd) + [0.0] * 8, mom, alpha, eps, max_norm, gs, ema_alpha)
        if flags is not None:
            d.flags = flags
        return d

    def call(d='default', total=TOTAL, nd=None, **ptrs):
        p = dict(w=w, g=g, m=m, v=v, ema=e, gmap=gmap, scratch=scratch)
        p.update(ptrs)
        return _call(desc() if isinstance(d, str) else d, p['w'], p['g'], p['m'], p['v'], p['ema'], p['gmap'], total=total,
                     scratch=p['scratch'], nd=nd, norm=norm)

    cases = [
        (ENULL, call(d=None)), (ENULL, call(w=None)), (ENULL, call(g=None)), (ENULL, call(m=None)), (ENULL, call(gmap=None)),
        (ENULL, call(scratch=None)),
        (ENULL, call(v=None)), (ENULL, call(desc(kind=oref.RMSPROP_TF), v=None)),
        (EINVAL, call(total=0)), (EINVAL, call(total=TOTAL - 4)), (EINVAL, call(total=8192 + 32)),
        (ERANGE, call(desc(ng=0))), (ERANGE, call(desc(ng=9))), (ERANGE, call(desc(ng=-1))),
        (EINVAL, call(desc(kind=3))), (EINVAL, call(desc(kind=-1))), (EINVAL, call(desc(flags=2))), (EINVAL, call(desc(flags=3))),
        (EINVAL, call(desc(kind=oref.RMSPROP, nesterov=True))), (EINVAL, call(desc(kind=oref.RMSPROP_TF, nesterov=True))),
        (EINVAL, call(desc(lr=[nan, 0.1]))), (EINVAL, call(desc(lr=[0.1, inf]))), (EINVAL, call(desc(wd=[0.0, nan]))),
        (EINVAL, call(desc(wd=[-inf, 0.0]))), (EINVAL, call(desc(mom=nan))), (EINVAL, call(desc(alpha=nan))),
        (EINVAL, call(desc(eps=inf))), (EINVAL, call(desc(max_norm=nan))), (EINVAL, call(desc(gs=inf))),
        (EINVAL, call(desc(kind=oref.SGD, mom=inf))),
        (EINVAL, call(desc(alpha=-0.1))), (EINVAL, call(desc(alpha=1.5))), (EINVAL, call(desc(kind=oref.RMSPROP_TF, alpha=1.5))),
        (EINVAL, call(desc(eps=0.0))), (EINVAL, call(desc(eps=-1e-3))), (EINVAL, call(desc(kind=oref.RMSPROP_TF, eps=0.0))),
        (EINVAL, call(desc(kind=oref.RMSPROP_TF, eps=-1e-3))),
        (EINVAL, call(desc(kind=oref.SGD, nesterov=True, mom=0.0))), (EINVAL, call(desc(kind=oref.SGD, nesterov=True, mom=-0.5))),
        (EINVAL, call(desc(ema_alpha=1.5))), (EINVAL, call(desc(ema_alpha=-0.1))), (EINVAL, call(desc(ema_alpha=nan))),
        (EINVAL, call(ema=w)), (EINVAL, call(ema=g)), (EINVAL, call(ema=m)), (EINVAL, call(ema=v)),
        (ERANGE, call(nd=3)), (ERANGE, call(nd=0)),
    ]
    for k, (want, rc) in enumerate(cases):
        assert rc == want, 'refusal %d: %d, expected %d' % (k, rc, want)
    torch.cuda.synchronize()                                                      # clean: nothing was launched
    for buf, old in ((w, w0), (g, g0), (m, m0), (v, v0), (e, e0)):
        assert torch.equal(buf[:TOTAL].cpu(), old) and bool((buf[TOTAL:] == SENT).all())
    assert bool((scratch == -1.0).all()) and float(norm) == -1.0 and torch.equal(gmap.cpu(), torch.from_numpy(gmap_np))
    # what is not refused: an ema_alpha outside [0, 1] without an ema, alpha / eps that SGD does not read, exactly enough scratch
    assert call(desc(ema_alpha=7.0), ema=None) == 0
    assert call(desc(kind=oref.SGD, alpha=5.0, eps=-1.0), v=None, ema=None, nd=4) == 0
    torch.cuda.synchronize()
