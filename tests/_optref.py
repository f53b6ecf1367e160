"""Float64 restatements of the three kinds of tfnas_opt_groups_step (csrc/opt_kernels.hip: k_opt_groups; the formulas of the
comment in include/tfnas_hip.h), with the clip of _smallref.clip_coef and the group map applied per 64-float block, and the
element-wise error bounds of the fp32 kernel.  Shared by tests/test_optref.py (which proves the restatements against
torch.optim.SGD / RMSprop and optim.RMSpropTF in float64 and the bounds against a float32 emulation and three wrong formulas) and
by the GPU tests (tests/test_gpu_optgroups_kernels.py, tests/test_gpu_optgroups_retrain.py).

Inputs are widened to float64 as they come in; the callers hand over the hyper-parameters as the C floats the kernel receives
(``_smallref.f32``).

Bounds.  Every fp32 operation contributes a relative error of U = 2^-24 of its own result; the errors are carried through the
formula to first order, absolute values throughout (so a cancellation in g' + wd w or d^2 - v is covered: the bound is absolute).
  g'   8 U |g'|: six roundings (the norm's cast, * grad_scale, + 1e-6, the division, grad_scale * coef, g * that), two spare
  d    E_d = E_g + U wd |w| + U |d|                       (product, sum)
  SGD  E_m = E_d + U mu |m| + U (mu |m| + |d|)            (product, sum)
       plain     E_w = lr E_m + U lr |m'| + U |w'|
       Nesterov  t = d + mu m':  E_t = E_d + mu E_m + U mu |m'| + U (|d| + mu |m'|);  E_w = lr E_t + U lr |t| + U |w'|
  RMSprop (torch)  E_dd = 2 |d| E_d + U d^2;  E_v = (1 - a) E_dd + 2 U (1 - a) d^2 + U a v + U v'   ((1 - a) itself is rounded once)
       s = sqrt(v'): E_s = E_v / (2 s) + U s;  den = s + eps: E_den = E_s + U den;  u = d / den: E_u = E_d / den + |u| E_den / den + U |u|
       mu > 0:  E_m = E_u + U mu |m| + U (mu |m| + |u|);  E_w = lr E_m + U lr |m'| + U |w'|
       mu = 0:  E_w = lr E_u + U lr |u| + U |w'|
  RMSprop (TF)  q = d^2 - v: E_q = E_dd + U |q|;  E_v = (1 - a) E_q + 2 U (1 - a) |q| + U v'
       r = sqrt(v' + eps): E_r = (E_v + U (v' + eps)) / (2 r) + U r;  p = lr d: E_p = lr E_d + U lr |d|
       t = p / r: E_t = E_p / r + |t| E_r / r + U |t|;  E_m = E_t + U mu |m| + U (mu |m| + |t|);  E_w = E_m + U |w'|
  ema  E_e = alpha E_w + _emaref.lerp_bound
Underflow: a product that lands below 2^-126 is rounded to a multiple of TINY = 2^-149 and not to 24 bits, so g' (g * scale),
d^2 and the two products that form v' each carry TINY on top wherever they are not exactly zero (a real network has gradient
elements of 1e-20 and less; the test inputs have none).
Where v' = 0 (the zero gaps between the slots) every term is 0.  No element is excluded from any comparison (share 0)."""
import numpy as np

import _emaref as er
import _smallref as sr

U = sr.U
TINY = 2.0 ** -149        # the smallest positive fp32
SGD, RMSPROP, RMSPROP_TF = 0, 1, 2
BLOCK = 64


def per_element(gmap, table, total):
    """(value of the element's group, live mask): a map byte >= len(table) switches its block off."""
    ids = np.repeat(np.asarray(gmap, dtype=np.int64), BLOCK)[:total]
    live = ids < len(table)
    return np.asarray(table, dtype=np.float64)[np.where(live, ids, 0)], live


def groups_ref(kind, w, g, m, v, gmap, lr, wd, mom, alpha, eps, max_norm, grad_scale, nesterov=False, ema=None, ema_alpha=None,
               wrong=None):
    """One tfnas_opt_groups_step in float64.  lr / wd: per-group lists.  Returns dict(w, g, m, v, ema, total, and the
    intermediates the bounds need).  ``wrong`` evaluates a deliberately wrong formula (tests of the bounds' tightness):
    'eps' -- eps on the other side of the root; 'lookahead' -- Nesterov without its look-ahead; 'rate' -- the TF form with the
    rate outside the momentum."""
    w, g, m = sr.d64(w), sr.d64(g), sr.d64(m)
    v = sr.d64(v) if v is not None else np.zeros_like(w)
    n = len(w)
    lr_e, live = per_element(gmap, lr, n)
    wd_e, _ = per_element(gmap, wd, n)
    total = float(np.sqrt(np.sum(g ** 2))) * grad_scale
    gc = g * grad_scale * sr.clip_coef(total, max_norm)
    d = gc + wd_e * w
    out = dict(g=gc, total=total, d=d, live=live, lr=lr_e, wd=wd_e)
    if kind == SGD:
        m2 = mom * m + d
        step = lr_e * ((d + mom * m2) if (nesterov and wrong != 'lookahead') else m2)
        w2, v2 = w - step, v
    elif kind == RMSPROP:
        v2 = alpha * v + (1.0 - alpha) * d * d
        den = np.sqrt(v2 + eps) if wrong == 'eps' else np.sqrt(v2) + eps
        u = d / den
        out['u'] = u
        if mom > 0:
            m2 = mom * m + u
            w2 = w - lr_e * m2
        else:
            m2 = m
            w2 = w - lr_e * u
    else:
        v2 = v + (1.0 - alpha) * (d * d - v)
        r = np.sqrt(v2) + eps if wrong == 'eps' else np.sqrt(v2 + eps)
        if wrong == 'rate':
            m2 = mom * m + d / r
            w2 = w - lr_e * m2
        else:
            m2 = mom * m + lr_e * d / r
            w2 = w - m2
    w2, m2, v2 = np.where(live, w2, w), np.where(live, m2, m), np.where(live, v2, v)
    out.update(w=w2, m=m2, v=v2)
    if ema is not None:
        e = sr.d64(ema)
        out['ema'] = np.where(live, er.lerp_ref(e, w2, ema_alpha), e)
    return out


def _div(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(b > 0, a / np.where(b > 0, b, 1.0), 0.0)


def groups_bounds(kind, ref, w, m, v, mom, alpha, eps, nesterov=False, ema=None, ema_alpha=None):
    """Element-wise bounds {g, m, v, w, ema} of the fp32 kernel around ``ref`` (a groups_ref result), from the old w / m / v (/ ema);
    zero where the block is switched off (m, v, w, ema: those must be bit-identical there)."""
    w, m = np.abs(sr.d64(w)), np.abs(sr.d64(m))
    v = np.abs(sr.d64(v)) if v is not None else np.zeros_like(w)
    lr, wd, live = ref['lr'], ref['wd'], ref['live']
    d, w2, m2, v2 = np.abs(ref['d']), np.abs(ref['w']), np.abs(ref['m']), np.abs(ref['v'])
    nzg = ref['g'] != 0
    Eg = 8 * U * np.abs(ref['g']) + TINY * nzg
    Ed = Eg + U * wd * w + U * d
    Ev = np.zeros_like(w)
    if kind == SGD:
        Em = Ed + U * mom * m + U * (mom * m + d)
        if nesterov:
            t = d + mom * m2
            Ew = lr * (Ed + mom * Em + U * mom * m2 + U * t) + U * lr * t + U * w2
        else:
            Ew = lr * Em + U * lr * m2 + U * w2
    else:
        c = 1.0 - alpha
        nzd = d != 0
        Edd = 2 * d * Ed + U * d * d + TINY * nzd
        if kind == RMSPROP:
            Ev = c * Edd + 2 * U * c * d * d + U * alpha * v + U * v2 + 2 * TINY * nzd
            s = np.sqrt(v2)
            den = s + eps
            Eden = _div(Ev, 2 * s) + U * s + U * den
            u = np.abs(ref['u'])
            Eu = Ed / den + u * Eden / den + U * u
            if mom > 0:
                Em = Eu + U * mom * m + U * (mom * m + u)
                Ew = lr * Em + U * lr * m2 + U * w2
            else:
                Em = np.zeros_like(w)
                Ew = lr * Eu + U * lr * u + U * w2
        else:
            q = np.abs(ref['d'] ** 2 - sr.d64(v))
            Ev = c * (Edd + U * q) + 2 * U * c * q + U * v2 + 2 * TINY * nzd
            r = np.sqrt(v2 + eps)
            Er = (Ev + U * (v2 + eps)) / (2 * r) + U * r
            t = lr * d / r
            Et = (lr * Ed + U * lr * d) / r + t * Er / r + U * t
            Em = Et + U * mom * m + U * (mom * m + t)
            Ew = Em + U * w2
    keeps_m = not (kind == RMSPROP and not mom > 0)
    Em = Em + 2 * TINY * ((ref['m'] != 0) & keeps_m)            # (the same for the products behind m' and w')
    Ew = Ew + 3 * TINY * (ref['w'] != 0)
    out = dict(g=Eg, m=np.where(live, Em, 0.0), v=np.where(live, Ev, 0.0), w=np.where(live, Ew, 0.0))
    if ema is not None:
        out['ema'] = np.where(live, ema_alpha * Ew + er.lerp_bound(ref['ema'], ref['w'], ema, ema_alpha), 0.0)
    return out


def groups_emul32(kind, w, g, m, v, gmap, lr, wd, mom, alpha, eps, max_norm, grad_scale, nesterov=False, ema=None, ema_alpha=None):
    """The kernel's operation order in numpy float32, one rounding per operation (no fused multiply-add; the squared norm in
    float64, as the kernel sums it).  Returns dict(w, g, m, v, ema, total)."""
    f = np.float32
    w, g, m = (np.asarray(sr.d64(t), dtype=f) for t in (w, g, m))
    v = np.asarray(sr.d64(v), dtype=f) if v is not None else np.zeros_like(w)
    n = len(w)
    lr_e, live = per_element(gmap, lr, n)
    wd_e, _ = per_element(gmap, wd, n)
    lr_e, wd_e = lr_e.astype(f), wd_e.astype(f)
    mom, alpha, eps, max_norm, grad_scale = f(mom), f(alpha), f(eps), f(max_norm), f(grad_scale)
    total = f(np.sqrt(np.sum(g.astype(np.float64) ** 2))) * grad_scale
    coef = min(f(1.0), max_norm / (total + f(1e-6))) if max_norm > 0 else f(1.0)
    gc = g * f(grad_scale * coef)
    d = gc + wd_e * w
    c = f(1.0 - float(alpha))
    if kind == SGD:
        m2 = mom * m + d
        w2 = w - lr_e * (d + mom * m2) if nesterov else w - lr_e * m2
        v2 = v
    elif kind == RMSPROP:
        v2 = alpha * v + c * (d * d)
        u = d / (np.sqrt(v2) + eps)
        if mom > 0:
            m2 = mom * m + u
            w2 = w - lr_e * m2
        else:
            m2, w2 = m, w - lr_e * u
    else:
        v2 = v + c * (d * d - v)
        m2 = mom * m + (lr_e * d) / np.sqrt(v2 + eps)
        w2 = w - m2
    out = dict(g=gc, total=float(total), w=np.where(live, w2, w), m=np.where(live, m2, m), v=np.where(live, v2, v))
    assert all(out[k].dtype == f for k in 'gwmv')
    if ema is not None:
        e = np.asarray(sr.d64(ema), dtype=f)
        a = f(ema_alpha)
        out['ema'] = np.where(live, a * (out['w'] - e) + e, e)
    return out


TOTAL = 3 * 8192 + 5 * 64      # three whole 8192-float chunks and a ragged fourth
LR, WD = [0.05, 0.2], [4e-5, 0.0]
ALPHA, EPS = 0.9, 1e-3
# (name, kind, nesterov, momentum): every kind at momentum 0 and 0.9 (Nesterov needs a momentum)
KINDS = [('sgd', SGD, False, 0.9), ('sgd', SGD, False, 0.0), ('nesterov', SGD, True, 0.9), ('rmsprop', RMSPROP, False, 0.9),
         ('rmsprop', RMSPROP, False, 0.0), ('rmsprop-tf', RMSPROP_TF, False, 0.9), ('rmsprop-tf', RMSPROP_TF, False, 0.0)]


def maps(total=TOTAL):
    """The three group maps of the kernel tests: ids 0, 1, 0, 1, ... per block (a boundary every 64 floats, inside every chunk);
    group 1 holding the single block that starts a chunk (float 8192: a boundary exactly on a chunk boundary, and one inside);
    all zero (with one group in the table)."""
    nb = total // BLOCK
    inter = np.arange(nb, dtype=np.uint8) % 2
    single = np.zeros(nb, dtype=np.uint8)
    single[8192 // BLOCK] = 1
    return dict(interleaved=(inter, 2), single=(single, 2), zero=(np.zeros(nb, dtype=np.uint8), 1))


def make_state(n, seed, gaps=True):
    """w, g, m, v, ema (float32 torch tensors, never modified) for an arena of n floats: v drawn as the Adam tests draw theirs
    (tests/test_gpu_opt_kernels.py: _adam_state) but around the gradient's magnitude -- v = (g^2 + 0.01 rand) * (0.5 + 1.5 rand) --
    so that d / sqrt(v) is O(1) as in a real run and the bounds speak about rounding, not about an amplified ratio.  ``gaps``: the
    last 4 * (1 + b % 6) floats of every third 64-float block are zero in every arena, as the padding between arena slots is."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.3
    m = torch.randn(n, generator=gen) * 0.1
    v = (g ** 2 + 0.01 * torch.rand(n, generator=gen)) * (0.5 + 1.5 * torch.rand(n, generator=gen))
    ema = w + 0.05 * torch.randn(n, generator=gen)
    gap = torch.zeros(n, dtype=torch.bool)
    if gaps:
        for b in range(0, n // BLOCK, 3):
            gap[BLOCK * (b + 1) - 4 * (1 + b % 6):BLOCK * (b + 1)] = True
        for t in (w, g, m, v, ema):
            t[gap] = 0.0
    return w, g, m, v, ema, gap
