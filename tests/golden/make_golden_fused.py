#!/usr/bin/env python3
"""Golden vectors of Fused-MBConv blocks.  The REFERENCE has no such block, so the pin is a composition of the reference's own
classes (imported from $TFNAS_REFERENCE, tests/_refload.py), run on the CPU in float64: a reference MBInvertedResBlock built
without an inverted_bottleneck (in = mid), whose ``depth_conv`` slot is given the reference's ConvLayer(in, mid, 3, stride, affine,
act) and whose ``point_linear`` slot its ConvLayer(mid, out, 1, 1, affine, act_func=None).  The block's OWN forward then runs
unchanged: the dense convolution layer, the reference's squeeze-excite arithmetic, the project layer, the residual with the
reference's drop_connect.

Where the reference exists:   TFNAS_REFERENCE=<reference dir> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fused.py
Output (committed):     tests/golden/oracle_fused_pin.npz
The fixture is data only (the composition's outputs).  While recording, the restatement of tests/_fused.py is compared with the
composition on the spot (the same comparison tests/test_fused_oracle_pin.py replays from the recorded side)."""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tf-nas_amd')):
    sys.path.insert(0, p)
import _fused  # noqa: E402
import _refload  # noqa: E402

ref = _refload.import_reference()
SLOT = {'fused_conv': 'depth_conv'}          # restatement's sub-module name -> the slot of the reference block that holds it


def composition(o):
    """The reference's classes put together as a Fused-MBConv block, with the weights of the restatement's block ``o``."""
    L = ref.layers
    ic, mid, se, oc, s, act, aff = o.in_channels, o.mid_channels, o.se_channels, o.out_channels, o.stride, o.act_func, o.derived
    blk = L.MBInvertedResBlock(mid, mid, se, oc, 3, s, affine=aff, act_func=act)
    assert blk.inverted_bottleneck is None
    blk.depth_conv = L.ConvLayer(ic, mid, 3, s, affine=aff, act_func=act)
    blk.point_linear = L.ConvLayer(mid, oc, 1, 1, affine=aff, act_func=None)
    blk.in_channels, blk.has_residual = ic, o.has_residual
    blk.drop_connect_rate = o.drop_connect_rate
    blk.load_state_dict({'.'.join([SLOT.get(k.split('.')[0], k.split('.')[0])] + k.split('.')[1:]): v
                         for k, v in o.state_dict().items()})
    return blk


def run_composition(o, x, r, seed):
    """pin_run of the composition, its results under the restatement's parameter names"""
    back = {v: k for k, v in SLOT.items()}
    res = _fused.pin_run(composition(o).double().train(), x, r, seed)
    out = OrderedDict()
    for k, v in res.items():
        head, _, rest = k.partition('.')
        if head in ('g', 'b'):
            first, _, tail = rest.partition('.')
            k = head + '.' + back.get(first, first) + '.' + tail
        out[k] = v
    return out


def pin_fixture():
    out = OrderedDict()
    for form in _fused.PIN_FORMS:
        for case in _fused.PIN_CASES:
            o, x, r, seed = _fused.pin_block(form, case)
            want = run_composition(o, x, r, seed)
            got = _fused.pin_run(o, x, r, seed)
            assert sorted(got) == sorted(want), (sorted(got), sorted(want))
            for k in got:
                scale = max(float(np.abs(want[k]).max()), 1e-30)
                assert float(np.abs(got[k] - want[k]).max()) <= 1e-12 * scale, (form, case, k)
            rec = _fused.pin_record(OrderedDict((k, want[k]) for k in got))
            for k, v in rec.items():
                out[_fused.pin_tag(form, case) + '/' + k] = v
            print('pin', _fused.pin_tag(form, case), 'ok')
    np.savez_compressed(os.path.join(HERE, 'oracle_fused_pin.npz'), **out)


if __name__ == '__main__':
    pin_fixture()
