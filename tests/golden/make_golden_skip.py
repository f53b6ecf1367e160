#!/usr/bin/env python3
"""Golden vectors of residual cells with a skip (identity) candidate.  The pin composes the REFERENCE's own MixedOP.forward (soft
branch; imported from $TFNAS_REFERENCE, tests/_refload.py) with ``m_ops`` entries replaced as tests/golden/make_golden_kinds.py
replaces them, and the reference's own IdentityLayer (models/layers.py:274-319) in the skip slots, run on the CPU in float64.
Recorded: probes of out, dx, d log_alphas and every parameter gradient, the expected latency ``out_lat`` the forward returns and
the row of the reference's own get_lookup_latency (its branch at models/model_search.py:96-97 prices the identity at 0).

Where the reference exists:   TFNAS_REFERENCE=<reference dir> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_skip.py
Output (committed):     tests/golden/skip_pin.npz
The fixture is data only.  While recording, the restatement of tests/_skip.py is compared with the composition on the spot (the
same comparison tests/test_skip_oracle_pin.py replays from the recorded side)."""
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
import _skip  # noqa: E402

ref = _refload.import_reference()


def composition(o, la):
    """The reference's MixedOP with the candidates (and weights) of the restatement ``o`` in its m_ops."""
    G = len(o.m_ops)
    cell = ref.MixedOP(o.in_channels, o.out_channels, o.stride, False, o.act_func, G,
                       {g: 4 * o.in_channels for g in range(G)}, _kinds.AnyLut())
    ops = []
    for op in o.m_ops:
        if isinstance(op, _skip.IdentityRef):
            blk = ref.layers.IdentityLayer(op.in_channels, op.out_channels)
        elif isinstance(op, _fused.FusedRef):
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
    cell.set_temperature(_skip.PIN_T)
    return cell


def run_composition(o, x, r, la, seed):
    cell = composition(o, la)
    xs = x.clone().requires_grad_(True)
    torch.manual_seed(seed)
    y, lat = cell(xs, False, None)
    (y * r).sum().backward()
    res = _kinds.pin_collect(y, xs, cell.log_alphas, cell.m_ops)
    lats = cell.get_lookup_latency(x.size(-1))
    assert lats[-1] == 0
    res['out_lat'] = np.asarray([float(lat.detach())])
    res['lats'] = np.asarray([float(v) for v in lats])
    # every sampled mode that picks the skip returns (x, 0)
    skip = [g for g, op in enumerate(cell.m_ops) if op.name == 'IdentityLayer'][0]
    cell.reset_switches()
    ys, ls = cell.m_ops[skip](xs), 0
    assert ys is xs and ls == 0
    return res


def pin_fixture():
    out = OrderedDict()
    for case in _skip.PIN_CASES:
        o, x, r, la, seed = _skip.pin_case(case)
        want = run_composition(o, x, r, la, seed)
        got = _skip.pin_run(o, x, r, la, seed)
        assert sorted(got) == sorted(want), (sorted(got), sorted(want))
        for k in got:
            scale = max(float(np.abs(want[k]).max()), 1e-30)
            assert float(np.abs(got[k] - want[k]).max()) <= 1e-12 * scale, (case[1:], k)
        nskip = sum(c[0] == 'S' for c in case[0])
        assert float(np.abs(want['dla'][-nskip:]).min()) > 0          # the skip slots get a gradient
        for k, v in _kinds.pin_record(OrderedDict((k, want[k]) for k in got)).items():
            out[_skip.pin_tag(case) + '/' + k] = v
        print('pin', _skip.pin_tag(case), 'ok')
    np.savez_compressed(os.path.join(HERE, 'skip_pin.npz'), **out)


if __name__ == '__main__':
    pin_fixture()
