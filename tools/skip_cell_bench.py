"""Device time of the alpha-step launch pair (forward + backward, frozen weights, dx and d wmix wanted) of one late residual cell
-- 14 x 14, ic = oc = 80, batch 128 -- with seven plain candidates plus a skip (TFNAS_CELL_SKIP: always a mixed cell, E
materialised) against the same seven without the skip (the fused per-image route), same process, alternating.
    python tools/skip_cell_bench.py [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tf-nas_amd'))
import torch  # noqa: E402
from tfnas_amd import geometry, load_lat_lookup, model_search as ms  # noqa: E402
from tfnas_amd.functions import MixedOpFn  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
INNER = 10
dev = torch.device('cuda', 0)
ic, size, batch = 80, 14, 128
mc = {i: geometry.init_mid_channels(ic, i) for i in range(8)}
lut = load_lat_lookup('gpu')
cell = ms.MixedOP(ic, ic, 1, False, 'swish', 8, mc, lut, primitives=ms.PRIMITIVES[:7] + ['skip']).to(dev)
for p in cell.parameters():
    p.requires_grad_(False)
x = torch.randn(batch, ic, size, size, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
r = torch.randn(batch, ic, size, size, device=dev).contiguous(memory_format=torch.channels_last)
plans = {'seven + skip': cell._plan(tuple(range(8))), 'seven': cell._plan(tuple(range(7)))}
ws = {k: torch.softmax(torch.randn(len(p.blocks), device=dev), -1).requires_grad_(True) for k, p in plans.items()}


def pair(name):
    plan = plans[name]
    y = MixedOpFn.apply(plan, x, ws[name], *plan.params())
    y.backward(r)


times = {k: [] for k in plans}
for name in plans:
    for _ in range(10):
        pair(name)
torch.cuda.synchronize()
for _ in range(reps):
    for name in plans:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):                     # (several pairs per event pair: the queue stays full, the host is hidden)
            pair(name)
        b.record()
        b.synchronize()
        times[name].append(a.elapsed_time(b) / INNER)
for name, t in times.items():
    t = sorted(t)
    print('%-14s median %.3f ms  min %.3f  max %.3f  (%d x %d launch pairs)' % (name, t[len(t) // 2], t[0], t[-1], len(t), INNER))
