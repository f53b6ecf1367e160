#!/usr/bin/env python3
"""What the path level buys an extended-candidate supernet: median time of the w-step and of the alpha-step of
model_search.Network(primitives=..., extended_paths=...) -- every kind, a dilated, a MixConv and a 7 x 7 candidate in every cell, a
skip in every residual one (the network of tests/_pathsext.py) -- on one of its two routes:

  --route per-cell   built without the keyword: one autograd node per cell, torch.optim tails (the only route it had before the
                     keyword; with TFNAS_LIB=<a build of the parent commit> the parent's own time)
  --route paths      extended_paths=True: path runner, weight arena, fused optimizer and classifier tails

The two step kinds run in SEPARATE loops (the w-steps of both routes then sample the same sub-networks from the same NoiseSource:
the architecture parameters do not move between them), warm-up excluded, device-synchronised around every timed step.  After the
timed loops one step of each kind runs with the library's launch hooks on: launches per step (and, with --families, launches and
HIP-event time per kernel family).  Prints ONE JSON line.  Alternate the two routes from a shell loop, each run under its own
`timeout` (DESIGN.md section 4a has the procedure and the numbers).

usage: ext_paths_time.py --route paths|per-cell [--batch 128] [--size 224] [--steps 8] [--warmup 3] [--families]   (GPU box)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tf-nas_amd'))
import torch  # noqa: E402
from tfnas_amd import Network, _lib, geometry, search  # noqa: E402

RES = ['MBI_k3_e3', 'FMB_k3_e6', 'DS_k5d2', 'MBI_k35_e6', 'FMB_k3_e3_se', 'DS_k3_se', 'MBI_k7_e6', 'skip']
NONRES = RES[:7] + ['MBI_k5_e6_se']


class Lut(dict):
    """every key -> {mid: a deterministic latency}; an IdentityLayer costs nothing (no table of this chip has these candidates)"""

    def __missing__(self, key):
        base = 0.0 if key.startswith('IdentityLayer_') else 0.25 + 0.003 * (sum(map(ord, key)) % 97)
        v = self[key] = _Row(base)
        return v


class _Row(dict):
    def __init__(self, base):
        super().__init__()
        self.base = base

    def __missing__(self, mid):
        v = self[mid] = self.base + (0.001 * int(mid) if self.base else 0.0)
        return v


def primitives():
    res = set(geometry.residual_cells())
    prims = {}
    for st, b, *_ in geometry.iter_cells():
        prims.setdefault(st, {})[b] = list(RES if (st, b) in res else NONRES)
    return prims


def launches(lib, f):
    """{family: (launches, ms)} of one call of ``f`` with the library's launch hooks on"""
    n = lib.tfnas_prof_count()
    names = [lib.tfnas_prof_name(i).decode() for i in range(n)]
    cnt, ms = C.c_uint64(), C.c_double()
    lib.tfnas_prof_enable((1 << n) - 1)
    try:
        f()
        torch.cuda.synchronize()
    finally:
        lib.tfnas_prof_enable(0)
    out = {}
    for i in range(n):
        _lib.check(lib.tfnas_prof_collect(i, C.byref(cnt), C.byref(ms)), 'tfnas_prof_collect')
        if cnt.value:
            out[names[i]] = (int(cnt.value), round(ms.value, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--route', choices=('paths', 'per-cell'), required=True)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--families', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(2)
    lut = Lut()
    lut['base'] = 1.5
    kw = {'extended_paths': True} if args.route == 'paths' else {}
    model = Network(100, geometry.initial_mc_num_dddict(), lut, primitives=primitives(), **kw).to(dev)
    model.set_temperature(5.0)
    state = search.SearchState(model)
    assert (state.runner is not None) == (args.route == 'paths')
    opt_w, opt_a = search.make_optimizers(model)
    noise = search.NoiseSource(2)
    x = torch.randn(args.batch, 3, args.size, args.size, device=dev)
    y = torch.randint(0, 100, (args.batch,), device=dev)

    def w():
        search.w_step(state, x, y, opt_w, 5.0, noise.exp(dev), noise.rand_pos())

    def a():
        search.a_step(state, x, y, opt_a, 15.0, 0.1, 5.0, noise.exp(dev))

    def med(f):
        ts = []
        for it in range(args.steps + args.warmup):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if it >= args.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return round(ts[len(ts) // 2], 3), round(ts[0], 3)
    wm, am = med(w), med(a)
    lib = _lib.lib()
    lw, la = launches(lib, w), launches(lib, a)
    res = dict(route=args.route, batch=args.batch, size=args.size, steps=args.steps, w_step_ms=wm[0], w_step_min_ms=wm[1],
               a_step_ms=am[0], a_step_min_ms=am[1], launches_w=sum(v[0] for v in lw.values()),
               launches_a=sum(v[0] for v in la.values()), lib=os.path.basename(_lib.LIB_PATH))
    if args.families:
        res['families_w'], res['families_a'] = lw, la
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
