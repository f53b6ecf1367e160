#!/usr/bin/env python3
"""Golden vectors of cells whose candidates differ in kind.  The pin composes the REFERENCE's own MixedOP.forward (soft branch:
F.gumbel_softmax over its log_alphas, the weighted sum over its m_ops; imported from $TFNAS_REFERENCE, tests/_refload.py) with
``m_ops`` entries replaced, run on the CPU in float64: plain and expand-free entries are the reference's MBInvertedResBlock (the
reference builds the expand-free form itself when mid <= in), Fused-MBConv entries -- which the reference does not have -- are
_fused.FusedRef (pinned to a composition of reference classes by tests/test_fused_oracle_pin.py).

Where the reference exists:   TFNAS_REFERENCE=<reference dir> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kinds.py
Output (committed):     tests/golden/kinds_pin.npz
The fixture is data only (probes of the composition's outputs).  While recording, the restatement of tests/_kinds.py is compared
with the composition on the spot (the same comparison tests/test_kinds_oracle_pin.py replays from the recorded side)."""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tf-nas_amd')):
    sys.path.insert(0, p)
import _fused  # noqa: E402
import _kinds  # noqa: E402
import _refload  # noqa: E402

ref = _refload.import_reference()


def composition(o, la):
    """The reference's MixedOP with the candidates (and weights) of the restatement ``o`` in its m_ops."""
    G = len(o.m_ops)
    cell = ref.MixedOP(o.in_channels, o.out_channels, o.stride, False, o.act_func, G,
                       {g: 4 * o.in_channels for g in range(G)}, _kinds.AnyLut())
    ops = []
    for op in o.m_ops:
        if isinstance(op, _fused.FusedRef):
            blk = copy.deepcopy(op)
            blk.name = 'FusedMBConvBlock'
        else:
            blk = ref.layers.MBInvertedResBlock(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, op.kernel_size,
                                                op.stride, affine=False, act_func=o.act_func)
            assert (blk.inverted_bottleneck is None) == (op.inverted_bottleneck is None)
            blk.load_state_dict(op.state_dict())
        ops.append(blk.double().train())
    cell.m_ops = torch.nn.ModuleList(ops)
    cell.log_alphas = torch.nn.Parameter(la.clone())
    cell.set_temperature(_kinds.PIN_T)
    return cell


def run_composition(o, x, r, la, seed):
    cell = composition(o, la)
    xs = x.clone().requires_grad_(True)
    torch.manual_seed(seed)
    y, lat = cell(xs, False, None)
    (y * r).sum().backward()
    return _kinds.pin_collect(y, xs, cell.log_alphas, cell.m_ops)


def pin_fixture():
    out = OrderedDict()
    for case in _kinds.PIN_CASES:
        o, x, r, la, seed = _kinds.pin_case(case)
        want = run_composition(o, x, r, la, seed)
        got = _kinds.pin_run(o, x, r, la, seed)
        assert sorted(got) == sorted(want), (sorted(got), sorted(want))
        for k in got:
            scale = max(float(np.abs(want[k]).max()), 1e-30)
            assert float(np.abs(got[k] - want[k]).max()) <= 1e-12 * scale, (case[1:], k)
        for k, v in _kinds.pin_record(OrderedDict((k, want[k]) for k in got)).items():
            out[_kinds.pin_tag(case) + '/' + k] = v
        print('pin', _kinds.pin_tag(case), 'ok')
    np.savez_compressed(os.path.join(HERE, 'kinds_pin.npz'), **out)


if __name__ == '__main__':
    pin_fixture()
