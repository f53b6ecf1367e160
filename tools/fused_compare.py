#!/usr/bin/env python3
"""A Fused-MBConv block next to the MBConv k3 block of the same (in, mid, out) (GPU box): the training forward + backward at
N = 128 (search form, SE, weight gradients on the caller's stream so that no launch overlaps another) and the eval forward at
N = 32 (derived form, running statistics), at three supernet geometries -- 112 x 112 16 -> 48 -> 24 stride 2, 56 x 56
24 -> 72 -> 24 stride 1, 14 x 14 80 -> 240 -> 80 stride 1.  The two blocks alternate; per round the wall time of a step between
HIP events on the stream and, in a second pass, the HIP-event time of each kernel family's launches (the library's tfnas_prof_*
timers); medians over the rounds are printed (Fused-MBConv tables).
   python tools/fused_compare.py [rounds] [train batch] [eval batch]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tf-nas_amd'))
import torch  # noqa: E402
from tfnas_amd import _lib, functions as F  # noqa: E402
from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
B_TRAIN = int(sys.argv[2]) if len(sys.argv) > 2 else 128
B_EVAL = int(sys.argv[3]) if len(sys.argv) > 3 else 32
# name, ic, mid, se, oc, stride, hw, act
GEOMS = [('112 x 112, 16 -> 48 -> 24, stride 2, SE 16, relu', 16, 48, 16, 24, 2, 112, 'relu'),
         ('56 x 56, 24 -> 72 -> 24, stride 1, SE 24, relu', 24, 72, 24, 24, 1, 56, 'relu'),
         ('14 x 14, 80 -> 240 -> 80, stride 1, SE 80, swish', 80, 240, 80, 80, 1, 14, 'swish')]
FAMS = ('k_conv_fwd', 'k_expand_fwd', 'k_dw_fwd', 'k_se_pool<fwd>', 'k_project_fwd', 'k_project_wgrad', 'k_project_dgrad',
        'k_se_pool<bwd>', 'k_bn2_bwd', 'k_conv_dd', 'k_dw_bwd_data', 'k_dw_wgrad', 'k_expand_dgrad', 'k_expand_wgrad', 'k_conv_dgrad',
        'k_conv_wgrad', 'k_reduce_rows')
KINDS = (('fused', FusedMBConvBlock), ('mbconv k3', MBInvertedResBlock))

lib = _lib.lib()
ids = {lib.tfnas_prof_name(i).decode(): i for i in range(lib.tfnas_prof_count())}
fams = [f for f in FAMS if f in ids]
dev = torch.device('cuda', 0)


def collect(fam):
    n, ms = C.c_uint64(), C.c_double()
    _lib.check(lib.tfnas_prof_collect(ids[fam], C.byref(n), C.byref(ms)), 'tfnas_prof_collect')
    return ms.value


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def table(title, steps, rounds, with_families, per=1):
    for fn in steps:                      # warm-up
        fn(); fn()
    torch.cuda.synchronize()
    wall = [[] for _ in steps]
    fam_ms = [{f: [] for f in fams} for _ in steps]
    for _ in range(rounds):               # alternating: wall time of one step
        for i, fn in enumerate(steps):
            wall[i].append(timed(fn) / per)
    if with_families:
        for _ in range(rounds):           # alternating: per-family device time of one step
            for i, fn in enumerate(steps):
                lib.tfnas_prof_enable(sum(1 << ids[f] for f in fams))
                fn()
                torch.cuda.synchronize()
                lib.tfnas_prof_enable(0)
                for f in fams:
                    fam_ms[i][f].append(collect(f))
    print(title)
    for (kind, _), w, fm in zip(KINDS, wall, fam_ms):
        line = '  %-10s step %.3f ms (min %.3f, max %.3f)' % (kind, statistics.median(w), min(w), max(w))
        if with_families:
            used = [(f, statistics.median(fm[f])) for f in fams if max(fm[f]) > 0]
            line += '  launches %.3f ms: ' % sum(v for _, v in used) + ', '.join('%s %.3f' % fv for fv in used)
        print(line)


for name, ic, mid, se, oc, s, hw, act in GEOMS:
    torch.manual_seed(1)
    x = torch.randn(B_TRAIN, ic, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    blocks = []
    for _, cls in KINDS:
        blk = cls(ic, mid, se, oc, 3, s, affine=False, act_func=act).to(dev)
        F.adopt_modes(blk, F.HipModes(route=F.route_bits(wgrad_stream=False)))
        blocks.append(blk)

    def train_step(blk):
        def run():
            out = blk(x)
            out.backward(out)
            blk.zero_grad()
            x.grad = None
        return run
    table('%s -- training forward + backward, N = %d, median of %d alternating rounds' % (name, B_TRAIN, ROUNDS),
          [train_step(b) for b in blocks], ROUNDS, True)

    xe = torch.randn(B_EVAL, ic, hw, hw, device=dev).contiguous(memory_format=torch.channels_last)
    evals = [cls(ic, mid, se, oc, 3, s, affine=True, act_func=act).to(dev).eval() for _, cls in KINDS]

    def eval_step(blk):
        def run():
            with torch.no_grad():
                for _ in range(10):
                    blk(xe)
        return run
    table('%s -- eval forward, N = %d (mean of ten forwards per round)' % (name, B_EVAL), [eval_step(b) for b in evals], ROUNDS,
          False, per=10)
