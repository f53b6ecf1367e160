#!/usr/bin/env python3
"""Golden vectors of the MixConv candidates, recorded by running the REFERENCE itself (imported from $TFNAS_REFERENCE,
tests/_refload.py) on the CPU in float64 -- for tests/test_mix_oracle_pin.py.

The reference's MBInvertedResBlock has one kernel size; its ``depth_conv.conv`` is an ``nn.Conv2d`` module, and the block's
forward runs it as a module.  The MixConv block of the reference is therefore the reference's block with that one module replaced
by ``SplitConv`` below -- per-segment ``nn.Conv2d(mc_s, mc_s, k_s, stride, padding=k_s // 2, groups=mc_s, bias=False)`` modules
over ``torch.split`` / ``torch.cat``, their weights views of the same packed weight; everything else -- BatchNorm, activations,
squeeze-excite, the residual, drop-connect -- is the reference's own code.

Where the reference exists:   TFNAS_REFERENCE=<reference dir> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mix.py
Output (committed):     tests/golden/oracle_mix_pin.npz
The fixture is data only (float64 arrays: the packed depthwise weight gradients whole, _golden.probe of every other tensor).
While recording, the restatement of tests/_mix.py is compared with the reference on the spot (the same comparison
tests/test_mix_oracle_pin.py replays from the recorded side)."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tf-nas_amd')):
    sys.path.insert(0, p)
import _mix  # noqa: E402
import _refload  # noqa: E402

ref = _refload.import_reference()


class SplitConv(torch.nn.Module):
    """per-segment depthwise nn.Conv2d modules over torch.split / torch.cat; ``weight`` is the ONE packed parameter (so the
    block's parameter names stay what they were), the modules' weights are re-pointed at its views before every forward"""

    def __init__(self, packed, mc, ks, stride):
        super().__init__()
        self.weight = torch.nn.Parameter(packed.detach().clone())
        self.mc, self.ks = mc, tuple(ks)
        self.cs = _mix.split(mc, len(ks))
        self.convs = [torch.nn.Conv2d(c, c, k, stride, padding=k // 2, groups=c, bias=False) for c, k in zip(self.cs, ks)]

    def forward(self, x):
        o = 0
        for conv, c, k in zip(self.convs, self.cs, self.ks):
            conv._parameters.pop('weight', None)
            conv.weight = self.weight[o:o + c * k * k].view(c, 1, k, k)       # (a view: its gradient lands in the packed one)
            o += c * k * k
        return torch.cat([conv(xi) for conv, xi in zip(self.convs, torch.split(x, self.cs, dim=1))], dim=1)


def reference_block(o, affine):
    """The reference's MBInvertedResBlock with the geometry and weights of the restatement block ``o``, its depth_conv.conv
    replaced by SplitConv carrying the same packed weight."""
    blk = ref.layers.MBInvertedResBlock(o.in_channels, o.mid_channels, o.se_channels, o.out_channels, int(o.kernel_size), o.stride,
                                        affine=affine, act_func=o.act_func)
    assert (blk.inverted_bottleneck is None) == (o.inverted_bottleneck is None)
    sd = o.state_dict()
    packed = sd.pop('depth_conv.conv.weight')
    own = blk.state_dict()
    sd['depth_conv.conv.weight'] = own['depth_conv.conv.weight']
    blk.load_state_dict(sd)
    blk.depth_conv.conv = SplitConv(packed, o.mid_channels, _mix.mix_of(o), o.stride)
    blk.drop_connect_rate = getattr(o, 'drop_connect_rate', 0.0)
    return blk.double().train()


def pin_fixture(out):
    for form in _mix.PIN_FORMS:
        for case in _mix.pin_cases(form):
            o, x, r, seed = _mix.pin_oracle_block(form, case)
            want = _mix.pin_run(reference_block(o, form == 'derived'), x, r, seed)
            got = _mix.pin_run(o, x, r, seed)
            assert list(got) == list(want), (list(got), list(want))
            for k in want:
                assert got[k].shape == want[k].shape, (form, case, k)
                assert np.allclose(got[k], want[k], atol=2e-6, rtol=1e-4), (form, case, k)
            for k, v in _mix.pin_record(want).items():
                out[_mix.pin_tag(form, case) + '/' + k] = np.asarray(v, dtype=np.float64)
            print('pin', _mix.pin_tag(form, case), 'ok')


if __name__ == '__main__':
    fx = OrderedDict()
    pin_fixture(fx)
    np.savez_compressed(os.path.join(HERE, 'oracle_mix_pin.npz'), **fx)
    print('bytes', os.path.getsize(os.path.join(HERE, 'oracle_mix_pin.npz')))
