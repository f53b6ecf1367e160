"""Float64 restatements of the small per-step kernels (csrc/opt_kernels.hip, csrc/arch_kernels.hip), shared by
tests/test_small_refs.py (which proves them against torch's own float64 CPU path) and by the raw-C-ABI GPU tests
(tests/test_gpu_opt_kernels.py, tests/test_gpu_arch_kernels.py).  Plain formulas from the comments of include/tfnas_hip.h
and from the reference's train_search.py:381-385 (clip_grad_norm_ + SGD) and :414-422 (clip_grad_norm_ + Adam + log_softmax).

Every input is widened to float64 as it comes in (the callers hand over float32 values -- the hyper-parameters too, rounded with
``f32``, because the kernels receive them as C floats); all arithmetic after that is float64."""
import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of fp32


def f32(x):
    """The double that a C float argument holds."""
    return float(np.float32(x))


def d64(t):
    """numpy float64 copy of a tensor / array / list."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.array(t, dtype=np.float64)


# ----------------------------------------------------------------------------------------- clip_grad_norm_ + SGD
def clip_coef(total, max_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (total + 1e-6)); max_norm <= 0 switches clipping off (the library's rule)."""
    return min(1.0, max_norm / (total + 1e-6)) if max_norm > 0 else 1.0


def sgd_clip_ref(w, g, m, ranges, goff, max_norm, lr, mom, wd, grad_scale):
    """ranges: [(off, len)] into w / m (and into g when ``goff`` is None); goff: the ranges' offsets inside g otherwise.
    Returns (w', g', m', total_norm): whole buffers, touched only inside the ranges."""
    w, g, m = d64(w), d64(g), d64(m)
    go = [o for o, _ in ranges] if goff is None else list(goff)
    total = np.sqrt(sum(float(np.sum(g[q:q + n] ** 2)) for q, (_, n) in zip(go, ranges))) * grad_scale
    coef = clip_coef(total, max_norm)
    for q, (o, n) in zip(go, ranges):
        gc = g[q:q + n] * grad_scale * coef                       # the clipped gradient stays readable
        g[q:q + n] = gc
        m[o:o + n] = mom * m[o:o + n] + (gc + wd * w[o:o + n])    # torch.optim.SGD, dampening 0, momentum buffer present
        w[o:o + n] = w[o:o + n] - lr * m[o:o + n]
    return w, g, m, total


def sgd_bounds(w, g_new, m, w_new, ranges, goff, lr, mom, wd):
    """Element-wise error bounds of the fp32 kernel: (for m' and g', for w'), zero outside the ranges.
    m' and g': 16 * 2^-24 * (|g'| + wd |w| + mom |m|) -- at most six fp32 roundings on top of a clip coefficient with about
    three; w': one more subtraction, 2 * 2^-24 |w'| + lr * (that bound).  Returns arrays indexed like w / m; the bound of g' is
    read at the ranges' arena offsets (``at_g`` maps it into g's layout)."""
    w, g_new, m, w_new = d64(w), d64(g_new), d64(m), d64(w_new)
    bm, bw = np.zeros_like(w), np.zeros_like(w)
    go = [o for o, _ in ranges] if goff is None else list(goff)
    for q, (o, n) in zip(go, ranges):
        bm[o:o + n] = 16 * U * (np.abs(g_new[q:q + n]) + wd * np.abs(w[o:o + n]) + mom * np.abs(m[o:o + n]))
        bw[o:o + n] = 2 * U * np.abs(w_new[o:o + n]) + lr * bm[o:o + n]
    return bm, bw


def at_g(arena_values, like_g, ranges, goff):
    """Re-index an arena-layout array into the gradient buffer's layout (zeros elsewhere)."""
    out = np.zeros(len(like_g))
    go = [o for o, _ in ranges] if goff is None else list(goff)
    for q, (o, n) in zip(go, ranges):
        out[q:q + n] = arena_values[o:o + n]
    return out


# ---------------------------------------------------------------- clip_grad_norm_ + Adam + log_softmax projection
def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    s = x - x.max()
    return s - np.log(np.sum(np.exp(s)))


def adam_project_ref(p_list, g_list, m, v, max_norm, lr, b1, b2, eps, wd, step, grad_scale):
    """p_list / g_list: n vectors of 1..8 elements; m / v: [rows >= n][8] moments (row i, first len_i entries).
    Returns (p' after the projection, m', v', total_norm, terms) -- terms = (b1 m, (1-b1) g_eff, b2 v, (1-b2) g_eff^2) as [rows][8]
    arrays: the two summands of each new moment (what the kernel's error is relative to)."""
    ps, gs = [d64(p) for p in p_list], [d64(g) * grad_scale for g in g_list]
    m, v = d64(m), d64(v)
    total = np.sqrt(sum(float(np.sum(g ** 2)) for g in gs))
    coef = clip_coef(total, max_norm)
    bias1, bias2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    terms = [np.zeros_like(m) for _ in range(4)]
    out = []
    for i, (p, g) in enumerate(zip(ps, gs)):
        k = len(p)
        ge = g * coef + wd * p                                    # torch Adam: weight decay is added to the gradient
        terms[0][i, :k], terms[1][i, :k] = b1 * m[i, :k], (1.0 - b1) * ge
        terms[2][i, :k], terms[3][i, :k] = b2 * v[i, :k], (1.0 - b2) * ge * ge
        m[i, :k] = terms[0][i, :k] + terms[1][i, :k]
        v[i, :k] = terms[2][i, :k] + terms[3][i, :k]
        denom = np.sqrt(v[i, :k]) / np.sqrt(bias2) + eps          # eps outside the square root
        out.append(log_softmax64(p - (lr / bias1) * (m[i, :k] / denom)))
    return out, m, v, total, terms


# ------------------------------------------------------------------------------------------- gumbel softmax
def gumbel_ref(la, e, T, lat=None):
    """w[c] = softmax((la[c] - log e[c]) / T); cell_lat[c] = sum_i w[c][i] lat[c][i] (0 without lat).  la, e, lat: [ncell][8]."""
    la, e = d64(la), d64(e)
    y = (la - np.log(e)) / T
    y = np.exp(y - y.max(axis=1, keepdims=True))
    w = y / y.sum(axis=1, keepdims=True)
    cl = (w * d64(lat)).sum(axis=1) if lat is not None else np.zeros(len(w))
    return w, cl


def arch_bwd_ref(w, lat, dw, dcl, T):
    """dla[c][j] = w_j (gt_j - sum_i gt_i w_i) / T,  gt = dw + dcl * lat; a None dw / dcl contributes nothing, and neither does the
    latency term without lat."""
    w = d64(w)
    gt = np.zeros_like(w)
    if dw is not None:
        gt = gt + d64(dw)
    if dcl is not None and lat is not None:
        gt = gt + d64(dcl)[:, None] * d64(lat)
    return w * (gt - (gt * w).sum(axis=1, keepdims=True)) / T


def sample_ref(la, mask, e, T, mode):
    """Position among the switched-on candidates, per cell -- the oracle's convention (MixedOP.forward): the active log_alphas
    compacted, the noise e[c][:n_active].  mode 0: argmax of gumbel_softmax(log_softmax(active), T); 1: argmin(active);
    2: argmax(active); first position on ties (torch's CPU argmax / argmin).  Returns (pos int32[ncell], gap[ncell]): gap = the
    relative difference of the two largest float64 weights in mode 0 (inf with one candidate and in modes 1 / 2)."""
    la = d64(la)
    mask = np.asarray(mask, dtype=bool)
    pos, gap = np.zeros(len(la), dtype=np.int32), np.full(len(la), np.inf)
    for c in range(len(la)):
        a = la[c][mask[c]]
        if mode == 0:
            y = (log_softmax64(a) - np.log(d64(e)[c][:len(a)])) / T
            y = np.exp(y - y.max())
            wt = y / y.sum()
            pos[c] = int(np.argmax(wt))
            if len(a) > 1:
                top = np.sort(wt)[::-1]
                gap[c] = (top[0] - top[1]) / top[0]
        else:
            pos[c] = int(np.argmin(a) if mode == 1 else np.argmax(a))
    return pos, gap


SAMPLE_GAP = 1e-5          # a mode-0 cell whose two largest float64 weights are closer than this (relative) may be left out
SAMPLE_CAP = 0.01          # ... but at most this share of the mode-0 cells


def sample_cases(seed=20):
    """The calls of the tfnas_arch_sample tests: 66 per mode (22 per ncell in {1, 18, 32}, alternating T = 5.0 / 0.1), random
    masks with 1..8 candidates on in every cell; every third call forces a cell with exactly one.  Each case:
    dict(ncell, T, mode, la float32 [ncell][8] (log_softmax rows), mask bool [ncell][8], e float32 [ncell][8])."""
    g = torch.Generator().manual_seed(seed)
    cases = []
    for mode in (0, 1, 2):
        for ncell in (1, 18, 32):
            for k in range(22):
                la = torch.log_softmax(torch.randn(ncell, 8, generator=g), -1)
                mask = torch.zeros(ncell, 8, dtype=torch.bool)
                for c in range(ncell):
                    n_on = int(torch.randint(1, 9, (1,), generator=g))
                    if k % 3 == 0 and c == (k // 3) % ncell:
                        n_on = 1
                    mask[c, torch.randperm(8, generator=g)[:n_on]] = True
                e = torch.empty(ncell, 8).exponential_(generator=g)
                cases.append(dict(ncell=ncell, T=5.0 if k % 2 == 0 else 0.1, mode=mode, la=la, mask=mask, e=e))
    return cases


def tie_cases():
    """Exact ties for modes 1 / 2 (never left out): all-equal log_alphas (the network's initial state) and a duplicated extreme,
    under full and partial masks.  (la float32 [ncell][8], mask bool [ncell][8])."""
    eq = torch.log_softmax(torch.zeros(3, 8), -1)
    m_eq = torch.tensor([[1] * 8, [0, 1, 1, 0, 1, 1, 1, 0], [0, 0, 0, 0, 0, 1, 0, 1]], dtype=torch.bool)
    dup = torch.tensor([[-2.0, -1.0, -3.0, -1.0, -2.5, -3.0, -1.0, -2.0],        # max -1 at 1, 3, 6; min -3 at 2, 5
                        [-3.0, -1.0, -3.0, -1.0, -2.5, -3.0, -1.0, -2.0],
                        [-2.0, -1.0, -3.0, -1.0, -2.5, -3.0, -1.0, -2.0]])
    m_dup = torch.tensor([[1] * 8, [1] * 8, [1, 0, 0, 1, 1, 1, 1, 1]], dtype=torch.bool)
    return [(eq, m_eq), (dup, m_dup)]


# ------------------------------------------------------------------------------------------------ sink mix
def sink_ref(betas, res, cell_lat=None, dout=None, dlat=None):
    """bw = softmax(betas); out = sum_k bw[k] res[k]; out_lat = sum_k bw[k] (cell_lat[0] + .. + cell_lat[k]) (0 without cell_lat).
    With ``dout`` (and optionally ``dlat``): the backward by float64 autograd -- dres[k], dbetas, dcell_lat (zeros without
    cell_lat / dlat).  Returns a dict of numpy float64 arrays."""
    b = torch.from_numpy(d64(betas)).requires_grad_(True)
    rs = [torch.from_numpy(d64(r)).requires_grad_(True) for r in res]
    cl = torch.from_numpy(d64(cell_lat)).requires_grad_(True) if cell_lat is not None else None
    bw = torch.softmax(b, -1)
    out = sum(bw[k] * rs[k] for k in range(len(rs)))
    lat = (bw * torch.cumsum(cl, 0)).sum() if cl is not None else torch.zeros((), dtype=torch.float64)
    r = dict(bw=bw.detach().numpy(), out=out.detach().numpy(), out_lat=float(lat.detach()))
    if dout is not None:
        obj = (out * torch.from_numpy(d64(dout))).sum()
        if cl is not None and dlat is not None:
            obj = obj + float(dlat) * lat
        obj.backward()
        r['dres'] = [t.grad.numpy() for t in rs]
        r['dbetas'] = b.grad.numpy()
        r['dcell_lat'] = cl.grad.numpy() if (cl is not None and cl.grad is not None) else np.zeros(len(rs))
    return r
