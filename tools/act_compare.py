#!/usr/bin/env python3
"""Launches of a sampled candidate by activation (GPU box): swish against h-swish and ReLU against ReLU6 on one stride-1 and one
stride-2 cell at batch 128, HIP-event time per launch from the library's tfnas_prof_* timers, for every kernel family that
applies the activation (depthwise forward / data gradient / weight gradient, SE squeeze, project forward / weight gradient, the
BN2-backward pass).  All four activations run on the SAME route -- E materialised, the LDS tile depthwise kernels, the
BN2-backward tables in their own pass, weight gradients on the caller's stream so that no launch overlaps another (route bits) --
which is the only route 'relu6' / 'h-swish' have: the comparison isolates the activation.  The variants alternate and the median
over the rounds is printed (activation table).
   python tools/act_compare.py [batch] [rounds]"""
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
# name, ic, mc, se, oc, k, stride, hw
GEOMS = [('stride 1, 14 x 14 x 480 (80 -> 80, k5, SE 80)', 80, 480, 80, 80, 5, 1, 14),
         ('stride 2, 56 x 56 x 144 (24 -> 40, k5, SE 24)', 24, 144, 24, 40, 5, 2, 56)]
ACTS = ('swish', 'h-swish', 'relu', 'relu6')
FAMS = ('k_dw_fwd', 'k_se_pool<fwd>', 'k_project_fwd', 'k_project_wgrad', 'k_se_pool<bwd>', 'k_bn2_bwd', 'k_dw_bwd_data',
        'k_dw_wgrad')
ROUTE = dict(wgrad_stream=False, dw='tiled', dwwg=False, dwwg2=False, fold=False, fx=False)

lib = _lib.lib()
ids = {lib.tfnas_prof_name(i).decode(): i for i in range(lib.tfnas_prof_count())}
dev = torch.device('cuda', 0)


def collect(fam):
    n, ms = C.c_uint64(), C.c_double()
    _lib.check(lib.tfnas_prof_collect(ids[fam], C.byref(n), C.byref(ms)), 'tfnas_prof_collect')
    return ms.value, n.value


for name, ic, mc, se, oc, k, s, hw in GEOMS:
    torch.manual_seed(1)
    x = torch.randn(B, ic, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    blocks = []
    for act in ACTS:
        blk = MBInvertedResBlock(ic, mc, se, oc, k, s, affine=False, act_func=act).to(dev)
        F.adopt_modes(blk, F.HipModes(route=F.route_bits(**ROUTE)))
        blocks.append(blk)

    def step(blk):
        out = blk(x)
        out.backward(out)
        torch.cuda.synchronize()
        blk.zero_grad()
        x.grad = None

    for blk in blocks:            # warm-up
        step(blk)
    times = [{f: [] for f in FAMS} for _ in blocks]       # ms per launch
    steps = [[] for _ in blocks]                            # ms per step, all these families together
    for _ in range(ROUNDS):
        for i, blk in enumerate(blocks):
            lib.tfnas_prof_enable(sum(1 << ids[f] for f in FAMS))
            step(blk)
            lib.tfnas_prof_enable(0)
            total = 0.0
            for f in FAMS:
                ms, n = collect(f)
                times[i][f].append(ms / max(1, n))
                total += ms
            steps[i].append(total)
    print('%s, B = %d, median of %d alternating rounds (ms per launch; last column: these launches of one step together)'
          % (name, B, ROUNDS))
    print('  %-8s' % '' + ' '.join('%15s' % f for f in FAMS) + '%10s' % 'step')
    for act, t, st in zip(ACTS, times, steps):
        print('  %-8s' % act + ' '.join('%15.3f' % statistics.median(t[f]) for f in FAMS) + '%10.3f' % statistics.median(st))
