#!/usr/bin/env python3
"""Depthwise launches of a sampled candidate by kernel size (GPU box): forward, data gradient and weight gradient of one MBConv
candidate with k = 5 (default route, and tile kernels only) and k = 7 (tile kernels) at two benchmark geometries, HIP-event time per
launch from the library's tfnas_prof_* timers.  Weight gradients run on the caller's stream (route bit) so that no launch overlaps
another; the variants alternate and the median over the rounds is printed (DESIGN.md section 4, 7 x 7 table).
   python tools/dw_k_compare.py [batch] [rounds]
With a third argument ``dil``: the dilated candidates beside their undilated twins -- k3, k3d2, k5, k5d2 (the undilated ones on
the default route and on the tile kernels the dilated ones always take) in a late cell (14 x 14, 80 -> 80) and an early cell
(56 x 56, 24 -> 24), both at six times the input width (dilation table).
   python tools/dw_k_compare.py 128 7 dil
With ``mix``: the MixConv candidates beside their plain twins on the tile kernels they always take -- k3, k5, k7, k35, k357 at
14 x 14 x 480 and 56 x 56 x 144.  A MixConv pass is two or three launches (one per kernel size of its segments), so this mode
prints the time of the whole PASS, the sum over its launches (MixConv table).
   python tools/dw_k_compare.py 128 7 mix"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tf-nas_amd'))
import torch  # noqa: E402
from tfnas_amd import _lib, functions as F  # noqa: E402
from tfnas_amd.layers import MBInvertedResBlock  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
GEOMS = [('56 x 56 x 144', 24, 144, 24, 1, 'relu', 56), ('14 x 14 x 672', 112, 672, 112, 1, 'swish', 14)]
VARIANTS = [('k5 default route', 5, {}), ('k5 tile kernels', 5, dict(dw='tiled', dwwg=False)), ('k7 tile kernels', 7, {})]
if len(sys.argv) > 3 and sys.argv[3] == 'dil':
    GEOMS = [('14 x 14 x 480', 80, 480, 80, 1, 'swish', 14), ('56 x 56 x 144', 24, 144, 24, 1, 'relu', 56)]
    TILE = dict(dw='tiled', dwwg=False)
    VARIANTS = [('k3 default route', 3, {}), ('k3 tile kernels', 3, TILE), ('k3d2 tile kernels', (3, 2), {}),
                ('k5 default route', 5, {}), ('k5 tile kernels', 5, TILE), ('k5d2 tile kernels', (5, 2), {})]
PER_PASS = len(sys.argv) > 3 and sys.argv[3] == 'mix'
if PER_PASS:
    GEOMS = [('14 x 14 x 480', 80, 480, 80, 1, 'swish', 14), ('56 x 56 x 144', 24, 144, 24, 1, 'relu', 56)]
    TILE = dict(dw='tiled', dwwg=False)
    VARIANTS = [('k3 tile kernels', 3, TILE), ('k5 tile kernels', 5, TILE), ('k7 tile kernels', 7, {}),
                ('k35 tile kernels', 'mix35', {}), ('k357 tile kernels', 'mix357', {})]
FAMS = ('k_dw_fwd', 'k_dw_bwd_data', 'k_dw_wgrad')

lib = _lib.lib()
ids = {lib.tfnas_prof_name(i).decode(): i for i in range(lib.tfnas_prof_count())}
dev = torch.device('cuda', 0)


def collect(fam):
    n, ms = C.c_uint64(), C.c_double()
    _lib.check(lib.tfnas_prof_collect(ids[fam], C.byref(n), C.byref(ms)), 'tfnas_prof_collect')
    return ms.value if PER_PASS else ms.value / max(1, n.value)      # (one forward + backward per collection: a pass's total)


for name, ic, mc, oc, s, act, hw in GEOMS:
    torch.manual_seed(1)
    x = torch.randn(B, ic, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    blocks = []
    for label, k, route in VARIANTS:
        mix = {'mix35': (3, 5), 'mix357': (3, 5, 7)}.get(k) if isinstance(k, str) else None
        k, dil = (max(mix), 1) if mix else k if isinstance(k, tuple) else (k, 1)
        blk = MBInvertedResBlock(ic, mc, 0, oc, k, s, affine=False, act_func=act, dilation=dil, mix_kernels=mix).to(dev)
        F.adopt_modes(blk, F.HipModes(route=F.route_bits(wgrad_stream=False, **route)))
        blocks.append(blk)

    def step(blk):
        out = blk(x)
        out.backward(out)
        torch.cuda.synchronize()
        blk.zero_grad()
        x.grad = None

    for blk in blocks:            # warm-up
        step(blk)
    times = [{f: [] for f in FAMS} for _ in blocks]
    for _ in range(ROUNDS):
        for i, blk in enumerate(blocks):
            lib.tfnas_prof_enable(sum(1 << ids[f] for f in FAMS))
            step(blk)
            lib.tfnas_prof_enable(0)
            for f in FAMS:
                times[i][f].append(collect(f))
    print('%s, B = %d, median of %d alternating rounds (ms per %s)' % (name, B, ROUNDS, 'pass' if PER_PASS else 'launch'))
    for (label, k, route), t in zip(VARIANTS, times):
        print('  %-19s' % label + '  '.join('%s %.3f' % (f, statistics.median(t[f])) for f in FAMS))
