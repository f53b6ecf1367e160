#!/usr/bin/env python3
"""A mixed 8-candidate launch (TFNAS_CELL_KINDS: 4 plain + 2 Fused-MBConv + 2 expand-free candidates in ONE cell) next to what
the same weighted sum costs without it (GPU box): the plain subset as one 4-candidate launch, each of the other four candidates as
a one-block launch, and the weighted sum in torch.  Forward + backward in the alpha-step form (frozen weights: d input and d mix
weights only), batch 128, at the supernet's cell geometries; the two variants alternate and the median HIP-event time over the
rounds is printed (mixed-cell table).  The widths are the search's initial ones (ic x 3 / ic x 6), SE = ic.
   python tools/kinds_compare.py [batch] [rounds] [first cell] [last cell]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tf-nas_amd'))
import torch  # noqa: E402
from tfnas_amd import geometry  # noqa: E402
from tfnas_amd.functions import CellPlan, MixedOpFn  # noqa: E402
from tfnas_amd.model_search import OPS  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
FIRST = int(sys.argv[3]) if len(sys.argv) > 3 else 0
LAST = int(sys.argv[4]) if len(sys.argv) > 4 else 17
# 4 plain + 2 fused + 2 expand-free, in the caller's order (what MixedOP(primitives=NAMES) launches)
NAMES = ['MBI_k3_e3', 'FMB_k3_e3', 'MBI_k5_e6', 'DS_k3_se', 'MBI_k3_e3_se', 'FMB_k3_e6_se', 'MBI_k5_e6_se', 'DS_k5']
dev = torch.device('cuda', 0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


print('B = %d, alpha-step form (frozen weights), forward + backward, median of %d alternating rounds, ms' % (B, ROUNDS))
print('%-34s %10s %10s %8s' % ('cell', 'mixed', 'emulated', 'ratio'))
for ci, (stage, block, ic, oc, s, act, size) in enumerate(geometry.iter_cells()):
    if not FIRST <= ci <= LAST:
        continue
    torch.manual_seed(ci)
    ops = [OPS[n](ic, ic * (6 if '_e6' in n else 3), oc, s, False, act).to(dev) for n in NAMES]
    for op in ops:
        for p in op.parameters():
            p.requires_grad_(False)
    plain = [i for i, op in enumerate(ops) if op.kind.name == 'MBCONV']
    other = [i for i in range(8) if i not in plain]
    mixed = CellPlan(ic, oc, s, act, ops, mixed_kinds=True)
    sub = CellPlan(ic, oc, s, act, [ops[i] for i in plain])
    ones = [CellPlan(ic, oc, s, act, [ops[i]]) for i in other]
    x = torch.randn(B, ic, size, size, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = torch.softmax(torch.randn(8, device=dev), -1).requires_grad_(True)
    r = torch.randn(B, oc, (size - 1) // s + 1, (size - 1) // s + 1, device=dev).contiguous(memory_format=torch.channels_last)

    def run_mixed():
        out = MixedOpFn.apply(mixed, x, w, *mixed.params())
        out.backward(r)
        x.grad = w.grad = None

    def run_emulated():
        out = MixedOpFn.apply(sub, x, w[plain], *sub.params())
        for i, p in zip(other, ones):
            out = out + w[i] * MixedOpFn.apply(p, x, None, *p.params())
        out.backward(r)
        x.grad = w.grad = None

    for fn in (run_mixed, run_emulated):                  # warm-up: plans, workspaces, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    t = ([], [])
    for _ in range(ROUNDS):
        for k, fn in enumerate((run_mixed, run_emulated)):
            t[k].append(timed(fn))
    a, b = statistics.median(t[0]), statistics.median(t[1])
    print('%-34s %10.3f %10.3f %8.2f' % ('%d %s.%s %dx%d %d->%d s%d %s' % (ci, stage, block, size, size, ic, oc, s, act), a, b, a / b))
    del ops, mixed, sub, ones, x, w, r
    torch.cuda.empty_cache()
