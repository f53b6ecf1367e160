"""Replay the committed golden vectors (captured from the imported reference by tests/golden/make_golden.py)
against the CPU oracle.  Runs anywhere -- this is what keeps the oracle pinned on the GPU box."""
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _golden
import tfnas_oracle as orc


def test_gumbel_softmax_known_answers():
    z = _golden.load('gumbel_kat.npz')
    for i in range(5):
        w = orc.gumbel_softmax(torch.from_numpy(z['logits%d' % i]), float(z['T%d' % i]), torch.from_numpy(z['e%d' % i]))
        assert np.allclose(w.numpy(), z['w%d' % i], atol=1e-7, rtol=1e-6)
        assert abs(float(w.sum()) - 1) < 1e-6


@pytest.mark.parametrize('name', _golden.CELL_NAMES)
def test_cell_soft_mode(name):
    fx = _golden.load('cell_%s.npz' % name)
    cell = _golden.oracle_cell_from(fx)
    x = torch.from_numpy(fx['x']).requires_grad_(True)
    out, lat = cell(x, False, None, exp_noise=torch.from_numpy(fx['e']))
    assert np.allclose(out.detach().numpy(), fx['soft_out'], atol=2e-5, rtol=1e-4)
    assert abs(float(lat) - float(fx['soft_lat'])) < 1e-6
    ((out * torch.from_numpy(fx['r'])).sum() + 3.0 * lat).backward()
    assert np.allclose(x.grad.numpy(), fx['soft_dx'], atol=2e-5, rtol=1e-3)
    assert np.allclose(cell.log_alphas.grad.numpy(), fx['soft_dalpha'], atol=2e-4, rtol=1e-3)
    for k, p in cell.named_parameters():
        if k != 'log_alphas':
            got, want = _golden.probe(p.grad), fx['softg.' + k]
            assert np.allclose(got, want, atol=1e-4 + 1e-4 * abs(want).max(), rtol=1e-3), k
    assert cell.get_lookup_latency(int(fx['geom'][4])) == [float(v) for v in fx['lats']]


@pytest.mark.parametrize('name', _golden.CELL_NAMES)
@pytest.mark.parametrize('idx', [1, 6])
def test_cell_sampled_candidate(name, idx):
    fx = _golden.load('cell_%s.npz' % name)
    cell = _golden.oracle_cell_from(fx)
    x = torch.from_numpy(fx['x']).requires_grad_(True)
    out = cell.m_ops[idx](x)
    assert np.allclose(out.detach().numpy(), fx['samp%d_out' % idx], atol=2e-5, rtol=1e-4)
    (out * torch.from_numpy(fx['r'])).sum().backward()
    assert np.allclose(x.grad.numpy(), fx['samp%d_dx' % idx], atol=2e-5, rtol=1e-3)
    for k, p in cell.m_ops[idx].named_parameters():
        want = fx['samp%d_g.%s' % (idx, k)]
        assert np.allclose(p.grad.numpy(), want, atol=1e-4 + 1e-4 * abs(want).max(), rtol=1e-3), k


@pytest.fixture(scope='module')
def lut():
    from tfnas_amd.latency import load_lat_lookup
    return load_lat_lookup('gpu')


def _net(lut, seed=2, T=5.0):
    torch.manual_seed(seed)
    m = orc.Network(100, orc.initial_mc_num_dddict(), lut)
    m.set_temperature(T)
    return m


def test_network_init_and_zero_noise_latency(lut):
    z = _golden.load('network.npz')
    m = _net(lut)
    got = np.array([v.abs().sum().item() for v in m.state_dict().values()])
    assert np.allclose(got, z['init_abs_sum'], rtol=1e-6), 'torch RNG stream differs from the fixture box'
    ones = torch.ones(18, 8)         # e = 1 -> gumbel noise -log(1) = 0
    with torch.no_grad():
        _, lat = m(torch.zeros(1, 3, 224, 224), False, exp_noise=ones)
    assert abs(float(lat) - float(z['zero_noise_lat'])) < 1e-5
    assert abs(float(lat) - 10.806680679) < 1e-5


def test_network_sampled_indices(lut):
    z = _golden.load('network.npz')
    m = _net(lut)
    g = torch.Generator().manual_seed(int(z['samp_x_seed']))
    noise = torch.empty(18, 8).exponential_(generator=g)
    assert np.array_equal(noise.numpy(), z['samp_noise'])
    x = torch.randn(1, 3, 224, 224, generator=g)
    random.seed(int(z['samp_random_seed']))
    with torch.no_grad():
        lg, _ = m(x, True, 'gumbel', exp_noise=noise)
        assert [c.last_idx for c in m.cells()] == z['samp_gumbel_idx'].tolist()
        lr_, _ = m(x, True, 'random')
    assert np.allclose(lg.numpy(), z['samp_logits_g'], atol=1e-5)
    assert np.allclose(lr_.numpy(), z['samp_logits_r'], atol=1e-5)


def test_search_trajectory_matches_reference_train_w_arch(lut):
    """6 iterations (3 alpha steps) of the reference's own train_w_arch, B=2 -- final arch params/weights.  Both sides in
    float64: in float32 the Adam steps of the arch parameters amplify rounding noise, which differs with the host and its
    thread count, far beyond these tolerances."""
    z = _golden.load('network.npz')
    m = _net(lut).double()
    B, iters = 2, 6
    g = torch.Generator().manual_seed(int(z['traj_seed']))
    xs = [torch.randn(B, 3, 224, 224, generator=g) for _ in range(iters)]
    ys = [torch.randint(0, 100, (B,), generator=g) for _ in range(iters)]
    xa = [torch.randn(B, 3, 224, 224, generator=g) for _ in range(iters // 2)]
    ya = [torch.randint(0, 100, (B,), generator=g) for _ in range(iters // 2)]
    ng = [torch.empty(18, 8).exponential_(generator=g) for _ in range(iters)]
    na = [torch.empty(18, 8).exponential_(generator=g) for _ in range(iters // 2)]
    assert np.allclose(_golden.probe(xs[0]), z['traj_x0_probe'])
    xs, xa, ng, na = ([t.double() for t in ts] for ts in (xs, xa, ng, na))
    opt_w, opt_a = orc.make_optimizers(m)
    random.seed(int(z['traj_random_seed']))
    for it in range(iters):
        orc.w_step(m, xs[it], ys[it], opt_w, 5.0, noise_g=ng[it])
        if it % 2 == 0:
            orc.a_step(m, xa[it // 2], ya[it // 2], opt_a, 15.0, 0.1, 5.0, noise=na[it // 2])
    arch = np.concatenate([p.detach().reshape(-1).numpy() for p in m.arch_parameters()])
    assert np.allclose(arch, z['traj_final_arch'], atol=2e-5), float(np.abs(arch - z['traj_final_arch']).max())
    wp = np.stack([_golden.probe(p) for p in m.weight_parameters()])
    assert np.allclose(wp, z['traj_final_wprobe'], atol=1e-4, rtol=1e-4)


def test_latency_known_answers(lut):
    from tfnas_amd import geometry as g
    from tfnas_amd.latency import load_lat_lookup, get_lookup_latency
    from tfnas_amd.elasticity import fit_mc_num_by_latency
    kat = json.load(open(os.path.join(_golden.GOLDEN, 'latency_kat.json')))
    mc = g.initial_mc_num_dddict()
    mcmax = g.get_mc_num_dddict(g.make_mc_mask_dddict(), is_max=True)
    keys = g.make_lat_lookup_key_dddict()

    def full_arch(op):
        return OrderedDict((st, OrderedDict((b, op) for b in mc[st])) for st in mc)
    for op in (0, 1, 7):
        assert abs(get_lookup_latency(full_arch(op), mc, keys, lut) - kat['all_op%d_gpu' % op]) < 1e-9
    assert abs(get_lookup_latency(full_arch(1), mc, keys, load_lat_lookup('cpu')) - kat['all_op1_cpu']) < 1e-9
    depth1 = OrderedDict((st, OrderedDict([('block1', 1)])) for st in mc)
    assert abs(get_lookup_latency(depth1, mc, keys, lut) - kat['depth1_op1_gpu']) < 1e-9
    for f in kat['fits']:
        new_mc, new_lat = fit_mc_num_by_latency(full_arch(f['op']), mc, mcmax, keys, lut, f['target'],
                                                list(mc.keys()), f['sign'])
        assert abs(new_lat - f['lat']) < 1e-9
        assert [new_mc[st][b][f['op']] for st in new_mc for b in new_mc[st]] == f['widths']
