#!/usr/bin/env python3
"""Launches of a block WITHOUT an expand convolution next to the expand block of the same ic / oc / k (GPU box): one sampled
candidate with SE and weight gradients at 56 x 56 and 14 x 14, batch 128, HIP-event time per launch from the library's
tfnas_prof_* timers, per kernel family.  Both run on the SAME route where they share one -- the LDS tile depthwise kernels, the
BN2-backward tables in their own pass, weight gradients on the caller's stream so that no launch overlaps another (route bits) --
which is the only route the expand-free block has; the expand block is also run on the library's default route.  The variants
alternate and the median over the rounds is printed (expand-free table).
   python tools/noexp_compare.py [batch] [rounds]"""
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
# name, ic, mid of the expand block, se, oc, k, stride, hw
GEOMS = [('56 x 56, 24 -> 24, k3, SE 24 (expand block: mid 72)', 24, 72, 24, 24, 3, 1, 56),
         ('14 x 14, 80 -> 80, k5, SE 80 (expand block: mid 240)', 80, 240, 80, 80, 5, 1, 14)]
FAMS = ('k_expand_fwd', 'k_dw_fwd', 'k_se_pool<fwd>', 'k_project_fwd', 'k_project_wgrad', 'k_project_dgrad', 'k_se_pool<bwd>',
        'k_bn2_bwd', 'k_dw_bwd_data', 'k_dw_wgrad', 'k_expand_dgrad', 'k_expand_wgrad')
TILED = dict(wgrad_stream=False, dw='tiled', dwwg=False, dwwg2=False, fold=False, fx=False)
VARIANTS = (('no expand (mid = in)', None, TILED), ('expand, tile route', 'mid', TILED),
            ('expand, default route', 'mid', dict(wgrad_stream=False)))

lib = _lib.lib()
ids = {lib.tfnas_prof_name(i).decode(): i for i in range(lib.tfnas_prof_count())}
fams = [f for f in FAMS if f in ids]
dev = torch.device('cuda', 0)


def collect(fam):
    n, ms = C.c_uint64(), C.c_double()
    _lib.check(lib.tfnas_prof_collect(ids[fam], C.byref(n), C.byref(ms)), 'tfnas_prof_collect')
    return ms.value, n.value


for name, ic, mid, se, oc, k, s, hw in GEOMS:
    torch.manual_seed(1)
    x = torch.randn(B, ic, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    blocks = []
    for _, which, route in VARIANTS:
        blk = MBInvertedResBlock(ic, mid if which else ic, se, oc, k, s, affine=False, act_func='swish').to(dev)
        F.adopt_modes(blk, F.HipModes(route=F.route_bits(**route)))
        blocks.append(blk)

    def step(blk):
        out = blk(x)
        out.backward(out)
        torch.cuda.synchronize()
        blk.zero_grad()
        x.grad = None

    for blk in blocks:            # warm-up
        step(blk)
    times = [{f: [] for f in fams} for _ in blocks]       # ms of the family's launches of one step
    steps = [[] for _ in blocks]
    for _ in range(ROUNDS):
        for i, blk in enumerate(blocks):
            lib.tfnas_prof_enable(sum(1 << ids[f] for f in fams))
            step(blk)
            lib.tfnas_prof_enable(0)
            total = 0.0
            for f in fams:
                ms, n = collect(f)
                times[i][f].append(ms)
                total += ms
            steps[i].append(total)
    print('%s, B = %d, swish, median of %d alternating rounds (ms of the family\'s launches in one forward + backward; last '
          'column: these families together)' % (name, B, ROUNDS))
    print('  %-22s' % '' + ' '.join('%15s' % f for f in fams) + '%10s' % 'step')
    for (vn, _, _), t, st in zip(VARIANTS, times, steps):
        print('  %-22s' % vn + ' '.join('%15.3f' % statistics.median(t[f]) for f in fams) + '%10.3f' % statistics.median(st))
