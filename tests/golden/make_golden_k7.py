#!/usr/bin/env python3
"""Golden vectors of the 7 x 7 depthwise candidates, recorded by running the REFERENCE itself (imported from $TFNAS_REFERENCE,
tests/_refload.py) on the CPU -- the companion of make_golden.py for tests/test_k7_oracle_pin.py and tests/test_gpu_k7.py.

Where the reference exists:   TFNAS_REFERENCE=<reference dir> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_k7.py
Outputs (committed):    tests/golden/oracle_k7_pin.npz, tests/golden/cell_k7_s1_swish_res.npz, tests/golden/cell_k7_s2_relu_odd.npz
The fixtures are data only (inputs, weights and the reference's outputs).  While recording, the oracle's blocks are compared
with the reference's on the spot (the same comparison tests/test_k7_oracle_pin.py replays from the recorded side)."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tf-nas_amd')):
    sys.path.insert(0, p)
import _golden  # noqa: E402
import _k7  # noqa: E402
import _refload  # noqa: E402

ref = _refload.import_reference()


def reference_block(form, case, oracle_blk):
    """The reference's MBInvertedResBlock(kernel_size=7) of one pin case with the oracle block's weights."""
    s, act, se = case
    q = _k7.PIN_GEOM
    blk = ref.layers.MBInvertedResBlock(q['ic'], q['mc'], se, q['oc'], 7, s, affine=(form == 'derived'), act_func=act)
    blk.load_state_dict(oracle_blk.state_dict())
    blk.drop_connect_rate = getattr(oracle_blk, 'drop_connect_rate', 0.0)
    return blk.double().train()


def pin_fixture():
    out = OrderedDict()
    for form in ('search', 'derived'):
        for case in _k7.PIN_CASES:
            o, x, r, seed = _k7.pin_oracle_block(form, case)
            want = _k7.pin_run(reference_block(form, case, o), x, r, seed)
            got = _k7.pin_run(o, x, r, seed)
            assert list(got) == list(want), (list(got), list(want))
            for k in want:
                assert np.allclose(got[k], want[k], atol=2e-6, rtol=1e-4), (form, case, k)
            for k, v in _k7.pin_record(want).items():
                out[_k7.pin_tag(form, case) + '/' + k] = v
            print('pin', _k7.pin_tag(form, case), 'ok')
    np.savez_compressed(os.path.join(HERE, 'oracle_k7_pin.npz'), **out)


def cell_fixtures():
    for name, ic, oc, s, act, H, W, B, mids in _k7.K7_CELLS:
        g = torch.Generator().manual_seed(len(name) * 131 + ic)
        mc = OrderedDict((i, m) for i, m in enumerate(mids))
        fake = {}
        torch.manual_seed(ic * 7 + oc)
        cell = ref.MixedOP(ic, oc, s, False, act, 8, mc, fake)
        for i, k in enumerate(_k7.SOFT_KS):
            op = cell.m_ops[i]
            if op.kernel_size != k:
                cell.m_ops[i] = ref.layers.MBInvertedResBlock(ic, mids[i], op.se_channels, oc, k, s, affine=False, act_func=act)
        for i, op in enumerate(cell.m_ops):
            key = '{}_{}_{}_{}_{}_k{}_s{}_{}'.format(op.name, W, op.in_channels, op.se_channels, op.out_channels,
                                                     op.kernel_size, op.stride, op.act_func)
            fake.setdefault(key, {})[op.mid_channels] = 0.3 + 0.17 * i + 0.01 * ic
        with torch.no_grad():
            for p in cell.parameters():       # non-trivial SE biases
                if p.dim() == 1 and p.numel() != 8:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            cell.log_alphas.copy_(F.log_softmax(torch.randn(8, generator=g) * 0.5, -1))
        cell.set_temperature(2.5)
        cell.train()
        x = torch.randn(B, ic, H, W, generator=g)
        e = torch.empty(8).exponential_(generator=g)
        r = torch.randn(B, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=g)          # cotangent
        fx = dict(x=x.numpy(), e=e.numpy(), r=r.numpy(), T=2.5, mids=np.array(mids), ks=np.array(_k7.SOFT_KS),
                  geom=np.array([ic, oc, s, H, W, B]), act=act)
        for k, v in cell.state_dict().items():
            fx['p.' + k] = v.numpy()
        xs = x.clone().requires_grad_(True)
        with _refload.inject_gumbel([e]):
            out, lat = cell(xs, sampling=False, mode=None)
        ((out * r).sum() + 3.0 * lat).backward()
        fx.update(soft_out=out.detach().numpy(), soft_lat=float(lat.detach()), soft_dx=xs.grad.numpy(),
                  soft_dalpha=cell.log_alphas.grad.numpy(), lats=np.array(cell.get_lookup_latency(W), dtype=np.float64))
        for k, p in cell.named_parameters():
            if k != 'log_alphas':
                fx['softg.' + k] = _golden.probe(p.grad)
        for idx in _k7.K7_SAMPLED:
            cell.zero_grad()
            xs = x.clone().requires_grad_(True)
            out = cell.m_ops[idx](xs)
            (out * r).sum().backward()
            fx['samp%d_out' % idx] = out.detach().numpy()
            fx['samp%d_dx' % idx] = xs.grad.numpy()
            for k, p in cell.m_ops[idx].named_parameters():
                fx['samp%d_g.%s' % (idx, k)] = p.grad.numpy()
        np.savez_compressed(os.path.join(HERE, 'cell_%s.npz' % name), **fx)
        print('cell', name, 'lat', float(lat))


if __name__ == '__main__':
    pin_fixture()
    cell_fixtures()
