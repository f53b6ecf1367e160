"""Cost of the accumulate epilogue (TFNAS_CELL_ACCUM_WGRAD, include/tfnas_hip.h): one sampled-mode cell backward at batch 128
with its weight gradients stored into fixed tensors, alternately written (bit clear) and added (bit set), in pairs whose order
alternates.  Prints per geometry the median backward time of each (HIP events around backward()) and the median and
interquartile range of the paired difference (accumulate - write).  GPU only:

    python tools/accum_cost.py [--iters 200]
"""
import argparse
import os
import sys
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tf-nas_amd'))

from tfnas_amd import _lib                              # noqa: E402
from tfnas_amd.functions import HipModes, MixedOpFn     # noqa: E402
from tfnas_amd.model_search import MixedOP              # noqa: E402

# (ic, oc, stride, act, H = W, candidate): supernet cells 1, 10 and 17 at their widest candidate (k5, expand 6, SE)
CELLS = OrderedDict([('cell1_56x56', (24, 24, 1, 'relu', 56, 7)), ('cell10_14x14', (112, 112, 1, 'swish', 14, 7)),
                     ('cell17_7x7', (192, 320, 1, 'swish', 7, 7))])


class AccumModes(HipModes):
    accum = False

    def apply(self, d):
        HipModes.apply(self, d)
        if self.accum:
            d.flags |= _lib.CELL_ACCUM_WGRAD


def measure(ic, oc, stride, act, hw, idx, iters, warm=10):
    mids = [3 * ic, 6 * ic] * 4

    class Lut(dict):
        def __missing__(self, key):
            v = self[key] = {m: 1.0 for m in mids}
            return v
    m = MixedOP(ic, oc, stride, False, act, 8, OrderedDict(enumerate(mids)), Lut()).cuda()
    plan = m._plan((idx,))
    params = plan.params()
    modes = AccumModes()
    plan._modes = modes
    plan.grad_targets = [torch.zeros_like(p) for p in params]
    x = torch.randn(128, ic, hw, hw, device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_(True)
    r = None
    t = {False: [], True: []}
    for it in range(warm + iters):
        for acc in ((False, True) if it % 2 == 0 else (True, False)):
            modes.accum = acc
            out = MixedOpFn.apply(plan, x, None, *params)
            r = torch.randn_like(out) if r is None else r
            x.grad = None
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out.backward(r)
            e1.record()
            torch.cuda.synchronize()
            if it >= warm:
                t[acc].append(e0.elapsed_time(e1) * 1e3)
    diff = sorted(b - a for a, b in zip(t[False], t[True]))

    def q(v, f):
        return sorted(v)[int(f * (len(v) - 1))]
    return dict(write_us=round(q(t[False], 0.5), 1), accum_us=round(q(t[True], 0.5), 1), diff_us_median=round(q(diff, 0.5), 1),
                diff_us_p25=round(q(diff, 0.25), 1), diff_us_p75=round(q(diff, 0.75), 1), pairs=len(diff))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    a = ap.parse_args()
    for name, geo in CELLS.items():
        print(name, measure(*geo, a.iters), flush=True)


if __name__ == '__main__':
    main()
