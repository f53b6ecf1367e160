"""CPU proof of the float64 reference of tests/_affineref.py, for every case tests/test_gpu_affine_f64.py runs on the GPU:
 (a) the fp32 oracle is within gate / 4 of the float64 oracle on every compared tensor -- the condition under which
     ``2e-5 + 1e-4 max|ref|`` (and ``1e-6 + 1e-5 |ref|`` for running statistics) separates a correct fp32 implementation from a
     wrong one; a case that breaks it has to shrink, not the gate;
 (b) the cases are what they claim: |beta / gamma| <= 10 with the edge channels in place, per-channel input means, momentum 0.01,
     dropped and kept images, and -- ReLU -- no pre-activation within _rawcell.KINK_TAU of 0 in the float64 oracle;
 (c) the float64 head + pool restatement equals orc.DerivedNetwork's own head on the same weights."""
import copy
from collections import OrderedDict

import pytest
import torch

import _affineref as ar
import tfnas_oracle as orc
from _rawcell import KINK_TAU


def _report(tag, ratios):
    print('AFFINE_REF %-22s %s' % (tag, '  '.join('%s %.4f' % kv for kv in ar.classes(ratios).items())))


@pytest.mark.parametrize('shape,mode', ar.BLOCK_CASES)
def test_fp32_oracle_is_within_a_quarter_gate_of_float64_blocks(shape, mode):
    case = ar.block_case(shape, mode)
    ratios = ar.compare(ar.reference(case, torch.float32), case.ref, scale=0.25)
    _report(case.name, ratios)
    assert max(ratios.values()) <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}


@pytest.mark.parametrize('key', list(ar.VARIANTS))
def test_fp32_oracle_is_within_a_quarter_gate_of_float64_variants(key):
    case = ar.block_case(key[0], key[1])
    ref = ar.variant_ref(*key)
    ratios = ar.compare(ar.reference(case, torch.float32, **ar.VARIANTS[key](case)), ref, scale=0.25)
    _report('%s-%s' % (case.name, key[2]), ratios)
    assert max(ratios.values()) <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}


@pytest.mark.parametrize('idx,form', ar.HEAD_CASES)
def test_fp32_oracle_is_within_a_quarter_gate_of_float64_heads(idx, form):
    case = ar.head_case(idx, form)
    ratios = ar.compare(ar.head_reference(case, torch.float32), case.ref, scale=0.25)
    _report(case.name, ratios)
    assert max(ratios.values()) <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}


def _check_bn_edges(mod):
    for bn in ar.batchnorms(mod):
        assert bn.momentum == ar.MOMENTUM
        for c, (g, b) in enumerate(ar.EDGES):
            assert float(bn.weight.detach()[c]) == pytest.approx(g, rel=1e-6)
            if b is not None:
                assert float(bn.bias.detach()[c]) == pytest.approx(b, rel=1e-6)
        assert float((bn.running_mean != 0).float().mean()) == 1.0 and float(bn.running_var.min()) >= 1.0
    worst = ar.worst_beta_over_gamma(mod)
    assert 10.0 * (1 - 1e-6) <= worst <= 10.0 * (1 + 1e-6), worst      # (the edge channels sit AT the limit)


@pytest.mark.parametrize('shape,mode', ar.BLOCK_CASES)
def test_block_cases_are_what_they_claim(shape, mode):
    case = ar.block_case(shape, mode)
    ic, mc, se, oc, k, s, act, N, H, W = case.geom
    assert tuple(case.x.shape) == (N, ic, H, W) and case.x.dtype == torch.float32
    _check_bn_edges(case.o)
    assert float(case.x.mean((0, 2, 3)).abs().max()) > 1.0            # per-channel means
    # the same seed gives the same case (everything comes from torch.Generator)
    again = ar._build_block(shape, mode, case.seed)
    assert torch.equal(again.x, case.x) and torch.equal(again.r, case.r)
    assert all(torch.equal(a, b) for a, b in zip(again.o.state_dict().values(), case.o.state_dict().values()))
    taps = case.ref['_taps']
    assert len(taps.sites) == 3
    if act == 'relu':
        # (b): every BatchNorm output that feeds a ReLU, and the SE hidden layer's pre-activation, clear of the kink
        assert min(taps.kink[:2] + taps.pre_kink) >= KINK_TAU, (taps.kink, taps.pre_kink)
        assert len(taps.pre_kink) == (1 if se else 0)
    if mode == 'drop':
        scale = torch.floor(ar.KEEP + case.u)
        assert scale.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]                # dropped and kept images
    if mode == 'alldrop':
        assert torch.floor(ar.KEEP + case.u).abs().max() == 0
        assert torch.equal(case.ref['y'], case.x.double())
        assert all(float(v.abs().max()) == 0.0 for k_, v in case.ref.items() if k_.startswith('g.'))
        before = {('b.' + k_): v for k_, v in case.o.named_buffers() if 'running' in k_}
        assert all(not torch.equal(case.ref[k_], v.double()) for k_, v in before.items())      # ... the statistics still move
    if mode == 'eval':
        before = {('b.' + k_): v for k_, v in case.o.named_buffers() if 'running' in k_}
        assert all(torch.equal(case.ref[k_], v.double()) for k_, v in before.items())


def test_the_doubled_batch_models_two_ranks_with_identical_shards():
    """the float64 oracle on cat([x, x]): y and dx repeat the one-shard run's (same statistics), parameter gradients double, and
    running_var carries 2 cnt / (2 cnt - 1) instead of cnt / (cnt - 1)"""
    case = ar.block_case('D', 'train')
    one, two = case.ref, ar.variant_ref('D', 'train', 'doubled')
    N = case.x.shape[0]
    for k in ('y', 'dx'):
        assert torch.allclose(two[k][:N], one[k], rtol=1e-10, atol=1e-12) and torch.allclose(two[k][N:], one[k], rtol=1e-10, atol=1e-12)
    for k in one:
        if k.startswith('g.'):
            assert torch.allclose(two[k], 2 * one[k], rtol=1e-9, atol=1e-11), k
    miss = []
    for i, name in enumerate(('inverted_bottleneck', 'depth_conv', 'point_linear')):
        cnt = float(N * 5 * 7)
        var = one['_taps'].sites[i]['var']
        rv0 = getattr(case.o, name).bn.running_var.double()
        want = (1 - ar.MOMENTUM) * rv0 + ar.MOMENTUM * var * (2 * cnt / (2 * cnt - 1))
        assert torch.allclose(two['b.%s.bn.running_var' % name], want, rtol=1e-12)
        wrong = (1 - ar.MOMENTUM) * rv0 + ar.MOMENTUM * var * (cnt / (cnt - 1))
        miss.append(ar.running_ratio(wrong, want))
    # the one-shard correction would miss the running-statistics gate where the variance is not small (sites 0 and 1)
    assert miss[0] > 1.0 and miss[1] > 1.0, miss


@pytest.mark.parametrize('idx', range(len(ar.HEADS)))
def test_head_cases_are_what_they_claim(idx):
    case = ar.head_case(idx, 'train')
    ic, mc, N, H, W = case.geom
    assert mc % 4 == 0                                                  # (a ragged head is never launched)
    assert tuple(case.x.shape) == (N, ic, H, W) and tuple(case.r.shape) == (N, mc)
    _check_bn_edges(case.o)
    assert float(case.x.mean((0, 2, 3)).abs().max()) > 1.0
    for form in ('search', 'eval'):
        other = ar.head_case(idx, form)
        assert torch.equal(other.x, case.x) and torch.equal(other.o.conv.weight, case.o.conv.weight)


def test_head_restatement_equals_the_derived_networks_own_head():
    """(c): _ConvBN + adaptive_avg_pool2d of _affineref.head_forward IS what orc.DerivedNetwork computes between its last block and
    its classifier, in train and in eval mode, in float64, on the network's own weights"""
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 1))
                       for i, (st, bl) in enumerate(orc.initial_mc_num_dddict().items()))
    torch.manual_seed(1)
    net = orc.DerivedNetwork(10, arch, orc.initial_mc_num_dddict())
    ar.randomise(net.feature_mix_layer, torch.Generator().manual_seed(4))
    net = net.double()
    seen = {}
    h1 = net.feature_mix_layer.register_forward_pre_hook(lambda m, inp: seen.__setitem__('x', inp[0].detach().clone()))
    h2 = net.classifier.linear.register_forward_pre_hook(lambda m, inp: seen.__setitem__('pooled', inp[0].detach().clone()))
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(2)).double()
    for train in (True, False):
        net.train(train)
        cb = copy.deepcopy(net.feature_mix_layer)              # (before the network's forward moves the running statistics)
        with torch.no_grad():
            net(x)
            pooled = ar.head_forward(cb, seen['x'], affine=True)
        assert tuple(seen['x'].shape[:2]) == (3, 320) and tuple(pooled.shape) == (3, 1280)
        assert torch.equal(pooled, seen['pooled'])
        assert torch.equal(cb.bn.running_var, net.feature_mix_layer.bn.running_var)
    h1.remove()
    h2.remove()
    # the search form is the same convolution under BatchNorm without affine part: gamma 1, beta 0 of the affine form in train mode
    with torch.no_grad():
        cb.train()
        cb.bn.weight.fill_(1.0)
        cb.bn.bias.fill_(0.0)
        assert torch.allclose(ar.head_forward(cb, seen['x'], affine=False), ar.head_forward(cb, seen['x'], affine=True),
                              rtol=1e-12, atol=1e-14)
