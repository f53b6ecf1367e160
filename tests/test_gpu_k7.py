"""GPU parity of depthwise kernel size 7: cells with 7 x 7 candidates (sampled launches with weight gradients, soft launches that
mix kernel sizes 3 / 3 / 5 / 5 / 7 / 7 / 3 / 7), the derived-network block, a derived network with 7 x 7 blocks and the latency
measurement, against the CPU oracle (pinned to the reference at k = 7 in tests/test_k7_oracle_pin.py).

Cells: every stage is compared with _hipcheck.check_cell at its default tolerances (abs err <= 2e-5 + 1e-4 * max|ref| per tensor),
ReLU decisions replayed, as for k = 3 / 5; no kink exemption (a cell with a 7 x 7 group never takes the E-free route).
Shapes: the smallest where each thing can go wrong (images smaller than / equal to the kernel, 1 x 1 images, odd and even sizes at
stride 2, two column tiles, ragged tile borders with the 16-channel tile of the stride-2 forward, widths that are no multiple
of 4)."""
import copy
import math

import numpy as np
import pytest
import torch

import _golden
import _hipcheck as hc
import _k7
import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [
    # name, N, ic, oc, H, W, stride, act, mids
    ('img_smaller_than_kernel_res', 2, 16, 16, 3, 5, 1, 'swish', [20, 33, 24, 40, 17, 35, 28, 44]),
    ('img_1x1', 5, 16, 16, 1, 1, 1, 'swish', [20, 33, 24, 40, 17, 35, 28, 44]),
    ('img_equals_kernel', 3, 32, 48, 7, 7, 1, 'swish', [41, 72, 36, 67, 45, 80, 53, 70]),
    ('s2_swish_odd', 2, 24, 40, 9, 13, 2, 'swish', [36, 72, 40, 60, 33, 66, 44, 71]),
    ('s2_relu_even', 2, 16, 24, 12, 10, 2, 'relu', [24, 40, 20, 36, 29, 44, 24, 50]),
    ('s1_relu_two_column_tiles_res', 2, 24, 24, 10, 22, 1, 'relu', [32, 52, 28, 56, 37, 60, 40, 62]),
    ('s2_relu_ragged_tiles_cc16', 1, 16, 24, 37, 41, 2, 'relu', [48, 96] * 4),
    ('s1_swish_odd_widths_res', 3, 40, 40, 8, 6, 1, 'swish', [53, 107, 44, 88, 61, 96, 48, 79]),
]
_BY_NAME = {c[0]: c for c in SHAPES}
_IDS = [c[0] for c in SHAPES]


def _inputs(cfg, ks=_k7.SOFT_KS):
    name, N, ic, oc, H, W, s, act, mids = cfg
    o, m = _k7.make_cell_pair(ic, oc, s, act, mids, ks=ks, seed=len(name))
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, ic, H, W, generator=g)
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=g)
    e = torch.empty(8).exponential_(generator=g)
    return o, m, x, r, e


@pytest.mark.parametrize('cfg', SHAPES, ids=_IDS)
def test_sampled_k7_candidate_with_weight_grads(cfg):
    """one 7 x 7 candidate (G = 1), weight gradients wanted: candidate 7 (SE width 2 * ic) of the mixed cell"""
    o, m, x, r, e = _inputs(cfg)
    assert o.m_ops[7].kernel_size == m.m_ops[7].kernel_size == 7
    res = hc.check_cell(o, m, x, r, e, [7], need_wgrad=True)
    assert 'g7.grad_dw' in res and 'g7.dEh' in res


@pytest.mark.parametrize('cfg', [_BY_NAME[n] for n in ('img_smaller_than_kernel_res', 's2_swish_odd', 's2_relu_ragged_tiles_cc16',
                                                       's1_relu_two_column_tiles_res')], ids=lambda c: c[0])
def test_sampled_k7_candidate_without_se(cfg):
    """a 7 x 7 candidate without squeeze-excite: candidate 1 of a cell with kernel sizes 3 / 7 / 5 / 5 / 3 / 3 / 5 / 5"""
    o, m, x, r, e = _inputs(cfg, ks=(3, 7, 5, 5, 3, 3, 5, 5))
    assert o.m_ops[1].kernel_size == 7 and not o.m_ops[1].se_channels
    hc.check_cell(o, m, x, r, e, [1], need_wgrad=True)


@pytest.mark.parametrize('cfg', SHAPES, ids=_IDS)
def test_soft_mode_mixing_k3_k5_k7(cfg):
    o, m, x, r, e = _inputs(cfg)
    assert [op.kernel_size for op in m.m_ops] == list(_k7.SOFT_KS)
    res = hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=False)
    assert any(k.endswith('.dEh') for k in res) and 'kink_fraction' not in res      # materialised route, nothing exempted


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_relu_two_column_tiles_res']], ids=lambda c: c[0])
def test_soft_mode_weight_grads_share_one_partial_row_matrix(cfg):
    """all eight candidates' depthwise weight gradients from one pass: the k = 3, 5 and 7 launches fill the same partial rows"""
    o, m, x, r, e = _inputs(cfg)
    res = hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=True)
    assert all('g%d.grad_dw' % i in res for i in range(8))


def test_elasticity_bound_all_k7_weight_grads():
    """eight 7 x 7 groups of 1536 channels: the weight-gradient partial row is 8 x 1536 x 49 floats, of which the partials region
    holds six -- the cap of dw_tile_plan decides the grid of all depthwise weight-gradient workgroups"""
    o, m, x, r, e = _inputs(('max_width_all_k7', 2, 192, 192, 7, 7, 1, 'swish', [1536] * 8), ks=(7,) * 8)
    res = hc.check_cell(o, m, x, r, e, list(range(8)), need_wgrad=True)
    assert all('g%d.grad_dw' % i in res for i in range(8))


def _run(m, x, r, e, idxs, route):
    from tfnas_amd import functions as F
    from tfnas_amd.functions import MixedOpFn
    F.adopt_modes(m, F.HipModes(route=route))
    plan = m._plan(tuple(idxs))
    ps = plan.params()
    for p in ps:
        p.requires_grad_(True)
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = torch.softmax(-e.log(), 0).cuda().requires_grad_(True) if len(idxs) > 1 else None
    out = MixedOpFn.apply(plan, xm, w, *ps)
    (out * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = [out.detach().clone(), xm.grad.clone()] + [p.grad.clone() for p in ps] + ([w.grad.clone()] if w is not None else [])
    for p in ps:
        p.grad = None
    return got


@pytest.mark.parametrize('cfg', [_BY_NAME['s2_swish_odd'], _BY_NAME['s1_relu_two_column_tiles_res']], ids=lambda c: c[0])
@pytest.mark.parametrize('idxs', [(7,), tuple(range(8))], ids=['sampled', 'soft'])
def test_route_word_cannot_move_a_k7_cell(cfg, idxs):
    """TFNAS_ROUTE_DW_*: a cell with a 7 x 7 group runs the tile kernels whatever the route asks -- every value gives the bits of
    the default route (on these shapes a 3 x 3 / 5 x 5 cell takes the register-window kernels at stride 2 and the ring kernels at
    22 columns)"""
    from tfnas_amd import functions as F
    o, m, x, r, e = _inputs(cfg)
    base = _run(m, x, r, e, idxs, F.route_bits())
    for dw in ('direct', 'lds', 'tiled'):
        got = _run(m, x, r, e, idxs, F.route_bits(dw=dw))
        assert len(got) == len(base)
        for i, (a, b) in enumerate(zip(got, base)):
            assert torch.equal(a, b), (dw, i)
    for kw in (dict(dwwg=False), dict(dwwg2=False)):           # (nor is the weight gradient ever fused into the backward-data pass)
        got = _run(m, x, r, e, idxs, F.route_bits(**kw))
        assert all(torch.equal(a, b) for a, b in zip(got, base)), kw


@pytest.mark.parametrize('name', _k7.K7_CELL_NAMES)
def test_hip_cell_matches_committed_k7_reference_vectors(name):
    """HIP path vs vectors captured from the REFERENCE itself (tests/golden/cell_k7_*.npz), replayed as
    tests/test_gpu_cell.py::test_hip_cell_matches_committed_reference_vectors replays the k = 3 / 5 ones."""
    fx = _golden.load('cell_%s.npz' % name)
    m = _k7.hip_cell_like(_k7.oracle_cell_from(fx), T=float(fx['T']))
    x = torch.from_numpy(fx['x']).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out, lat = m(x, False, None, exp_noise=torch.from_numpy(fx['e']).cuda())
    assert np.allclose(out.detach().cpu().numpy(), fx['soft_out'], atol=1e-4, rtol=1e-3)
    assert abs(float(lat.detach()) - float(fx['soft_lat'])) < 1e-5
    ((out * torch.from_numpy(fx['r']).cuda()).sum() + 3.0 * lat).backward()
    assert np.allclose(x.grad.cpu().numpy(), fx['soft_dx'], atol=1e-4, rtol=1e-3)
    assert np.allclose(m.log_alphas.grad.cpu().numpy(), fx['soft_dalpha'], atol=1e-4, rtol=1e-3)
    for idx in _k7.K7_SAMPLED:
        m.zero_grad()
        xs = torch.from_numpy(fx['x']).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        o_ = m.m_ops[idx](xs)
        assert np.allclose(o_.detach().cpu().numpy(), fx['samp%d_out' % idx], atol=1e-4, rtol=1e-3)
        (o_ * torch.from_numpy(fx['r']).cuda()).sum().backward()
        assert np.allclose(xs.grad.cpu().numpy(), fx['samp%d_dx' % idx], atol=1e-4, rtol=1e-3)
        for k, p in m.m_ops[idx].named_parameters():
            want = fx['samp%d_g.%s' % (idx, k)]
            assert np.allclose(p.grad.cpu().numpy(), want, atol=1e-4 + 1e-4 * abs(want).max(), rtol=1e-3), k


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_derived_block_k7_matches_oracle(mode):
    """the affine (derived-network) entry points at k = 7 with injected drop-connect draws; tolerances of tests/test_gpu_derived.py"""
    from tfnas_amd.layers import MBInvertedResBlock
    ic, mc, se, oc, k, s, act, hw, N = 40, 120, 40, 40, 7, 1, 'swish', 14, 4
    gen = torch.Generator().manual_seed(5)
    o = orc.DerivedBlock(ic, mc, se, oc, k, s, act)
    _k7.randomise_bn(o, gen)
    with torch.no_grad():
        o.depth_conv.bn.weight[0] = -0.7              # a negative gamma as well
    m = MBInvertedResBlock(ic, mc, se, oc, k, s, affine=True, act_func=act)
    m.load_state_dict(o.state_dict())
    m = m.cuda()
    x = torch.randn(N, ic, hw, hw, generator=gen)
    r = torch.randn(N, oc, hw, hw, generator=gen)
    o.drop_connect_rate = m.drop_connect_rate = 0.4
    u = torch.tensor([0.9, 0.1, 0.7, 0.3])           # floor(0.6 + u): images 0 and 2 kept, 1 and 3 dropped
    o.drop_u, m.drop_u = u, u
    if mode == 'eval':
        o.eval(); m.eval()
    else:
        o.train(); m.train()
    xo = x.clone().requires_grad_(True)
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yo, ym = o(xo), m(xm)
    assert torch.allclose(ym.cpu(), yo, atol=2e-5, rtol=1e-4), float((ym.cpu() - yo).abs().max())
    if mode == 'eval':
        return
    (yo * r).sum().backward()
    (ym * r.cuda()).sum().backward()
    assert torch.allclose(xm.grad.cpu(), xo.grad, atol=2e-5 + 1e-3 * float(xo.grad.abs().max()), rtol=1e-3)
    for (kk, po), (_, pm) in zip(o.named_parameters(), m.named_parameters()):
        err, ref = float((pm.grad.cpu() - po.grad).abs().max()), float(po.grad.abs().max())
        assert err <= 2e-5 + 2e-3 * ref, (kk, err, ref)
    for (kk, bo), (_, bm) in zip(o.named_buffers(), m.named_buffers()):
        assert torch.allclose(bm.cpu().float(), bo.float(), atol=1e-5, rtol=1e-4), kk       # running stats / batch counter


def test_networkcfg_with_k7_blocks_trains_deterministically():
    """NetworkCfg from a config whose stage-3 and stage-5 blocks are 7 x 7: one train_step runs, the loss is finite, every
    parameter changes, and the same step on a fresh copy is bit-identical; MACs against the hand formula"""
    from tfnas_amd import model_eval as me, parsing
    cfg = _k7.k7_network_config(50)
    assert abs(parsing.count_macs_in_M(cfg, 64) - _k7.hand_macs_in_M(cfg, 64)) < 1e-9
    torch.manual_seed(3)
    m0 = me.NetworkCfg(50, cfg, None, 0.0, 0.2)
    assert sorted(b.kernel_size for st in m0._stages() for b in st).count(7) == 4
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(4, 3, 64, 64, generator=gen).cuda()
    y = torch.randint(0, 50, (4,), generator=gen).cuda()
    us = [torch.rand(4, generator=gen) for _ in range(1 + sum(len(st) for st in m0._stages()))]

    def step():
        m = copy.deepcopy(m0).cuda()
        m.train()
        for b, u in zip([m.second_stem] + [b for st in m._stages() for b in st], us):
            b.drop_u = u
        opt = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
        torch.manual_seed(11)
        loss, _ = me.train_step(m, x, y, me.CrossEntropyLabelSmooth(50, 0.1), opt, 5.0)
        torch.cuda.synchronize()
        return float(loss), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    loss_a, sd_a = step()
    assert math.isfinite(loss_a)
    for k, p in m0.named_parameters():
        assert not torch.equal(sd_a[k], p.detach()), k
    loss_b, sd_b = step()
    assert loss_a == loss_b
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k


def test_latency_measurement_of_a_k7_block():
    from tfnas_amd import lut_builder
    ms = lut_builder.Measurer(torch.device('cuda:0')).measure(24, 72, 0, 24, 7, 1, 'relu', 28, batch=4, iters=2, reps=1)
    assert math.isfinite(ms) and ms > 0
