"""Pin the CPU restatement of MixConv candidates -- what tests/test_gpu_mix*.py then compare the HIP path with.

tests/_mix.py runs the oracle's own blocks with the one depthwise ``F.conv2d`` call of tfnas_oracle, when it is handed a packed
1-D weight, replaced by split -> grouped conv2d per segment -> cat (``mixed``), nothing else restated.  It is compared here, in
float64, with tests/golden/oracle_mix_pin.npz, which tests/golden/make_golden_mix.py recorded from the REFERENCE's
MBInvertedResBlock with its ``depth_conv.conv`` replaced by per-segment ``nn.Conv2d`` modules over ``torch.split`` / ``torch.cat``
carrying the same packed weight: forward and every gradient, k35 and k357, both strides, with and without SE, ReLU and swish, the
batch-statistic and the affine form (running statistics, drop-connect), at 2 x 16 x 9 x 13 with mid 44 (24 | 20 and 20 | 12 | 12), a
ragged mid 53 (28 | 25 and 24 | 16 | 13) and an expand-free block (8 | 8 and 8 | 4 | 4).  Tolerances: those of
tests/test_dil_oracle_pin.py (1e-5 / 1e-5 forward and buffers, 2e-6 / 1e-4 gradients).  Where a checkout of the reference is at
hand (TFNAS_REFERENCE) the generator's own reference block is run as well and must agree with what was recorded."""
import os

import numpy as np
import pytest
import torch

import _golden
import _mix
import _refload
import tfnas_oracle as orc

FWD = dict(atol=1e-5, rtol=1e-5)
GRAD = dict(atol=2e-6, rtol=1e-4)
_CASES = [(form, case) for form in _mix.PIN_FORMS for case in _mix.pin_cases(form)]


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('oracle_mix_pin.npz')


def _check(res, recorded, tag, nw):
    want_keys = [n[len(tag) + 1:] for n in recorded.files if n.startswith(tag + '/')]
    assert list(res) == want_keys
    for key, v in res.items():
        want = recorded[tag + '/' + key]
        tol = FWD if key == 'out' or key.startswith('b.') else GRAD
        if key == 'g.depth_conv.conv.weight':
            assert v.shape == want.shape == (nw,)              # (the packed layout: sum of mc_s * k_s * k_s floats)
            assert np.allclose(v, want, **tol), (tag, key, float(abs(v - want).max()))
        else:
            t = torch.from_numpy(np.asarray(v))
            assert _golden.probe_close(_golden.probe(t), want, t.numel(), tol['atol'], tol['rtol']), (tag, key)


def test_split_rule():
    """q = ceil(mc / 4) quads, q // n each, the remainder to segment 0, the last segment cut at mc"""
    assert _mix.split(44, 2) == [24, 20] and _mix.split(44, 3) == [20, 12, 12]
    assert _mix.split(53, 3) == [24, 16, 13] and _mix.split(53, 2) == [28, 25]
    assert _mix.split(9, 3) == [4, 4, 1] and _mix.split(12, 3) == [4, 4, 4]
    assert _mix.split(107, 2) == [56, 51] and _mix.split(107, 3) == [36, 36, 35]
    assert _mix.split(1536, 3) == [512, 512, 512] and _mix.split(480, 2) == [240, 240]      # (MixNet's own equal split)
    assert _mix.packed_size(53, (3, 5, 7)) == 24 * 9 + 16 * 25 + 13 * 49


@pytest.mark.parametrize('form,case', _CASES, ids=[_mix.pin_tag(f, c) for f, c in _CASES])
def test_restatement_matches_the_reference_block_with_a_split_depth_conv(recorded, form, case):
    ks, s, act, se, mid = case
    blk, x, r, seed = _mix.pin_oracle_block(form, case)
    assert _mix.mix_of(blk) == ks and blk.kernel_size == max(ks)
    assert (blk.inverted_bottleneck is None) == (mid == 16)
    nw = _mix.packed_size(blk.mid_channels, ks)
    assert blk.depth_conv.conv.weight.shape == (nw,) and 'depth_conv.conv.weight' in blk.state_dict()
    res = _mix.pin_run(blk, x, r, seed)
    assert res['out'].shape == (2, 16, (9 - 1) // s + 1, (13 - 1) // s + 1)
    _check(res, recorded, _mix.pin_tag(form, case), nw)
    if _refload.available():                      # the reference itself, where it can be imported
        import importlib.util
        spec = importlib.util.spec_from_file_location('make_golden_mix', os.path.join(_golden.GOLDEN, 'make_golden_mix.py'))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        o = _mix.pin_oracle_block(form, case)[0]          # (before a step moved the running statistics)
        _check(_mix.pin_run(gen.reference_block(o, form == 'derived'), x, r, seed), recorded, _mix.pin_tag(form, case), nw)


@pytest.mark.parametrize('form', _mix.PIN_FORMS)
@pytest.mark.parametrize('ks', [(3, 5), (3, 7), (5, 7), (3, 5, 7)])
def test_restatement_equals_plain_blocks_on_each_segment(form, ks):
    """the depthwise output of a MixConv block on segment s IS the plain k_s x k_s depthwise convolution of those channels: the
    restatement's mix_conv2d against nn.Conv2d run segment by segment on the sliced input (float64, exact)"""
    torch.manual_seed(17)
    mc, stride = 53, 2 if form == 'derived' else 1
    dw = _mix.PackedDW(mc, ks, stride).double()
    x = torch.randn(2, mc, 9, 13, dtype=torch.float64)
    y = dw(x)
    c0 = 0
    for c, k, w in zip(_mix.split(mc, len(ks)), ks, _mix.segments(dw.weight, mc, ks)):
        conv = torch.nn.Conv2d(c, c, k, stride, k // 2, groups=c, bias=False).double()
        with torch.no_grad():
            conv.weight.copy_(w)
        assert torch.equal(conv(x[:, c0:c0 + c]), y[:, c0:c0 + c])
        c0 += c
    assert c0 == mc


def test_only_the_depthwise_call_is_rewritten_and_only_for_a_packed_weight():
    """under mixed() the oracle's 1 x 1 convolutions and SE convolutions keep their arguments: one rewritten call per forward of a
    MixConv block, none for a plain block (bit-identical to the plain oracle), and the oracle module is what it was afterwards"""
    F0 = orc.F
    torch.manual_seed(3)
    blk = _mix.mix_block(orc.MBConv, 16, 44, 8, 16, (3, 5, 7), 1, 'swish')
    x = torch.randn(2, 16, 9, 13)
    with _mix.mixed((3, 5, 7)) as hits:
        y = orc.MBConv.forward(blk, x)             # (the oracle's own forward: MixMBConv.forward is this, inside mixed())
        assert hits == [1]
    assert torch.equal(y, blk(x))
    assert y.shape == (2, 16, 9, 13) and orc.F is F0
    plain = orc.MBConv(16, 44, 8, 16, 5, 2, 'relu')
    with _mix.mixed((3, 5)) as hits:
        a = plain(x)
    assert hits == [0] and torch.equal(a, plain(x))


def test_fixture_holds_arrays_only_and_is_small():
    path = os.path.join(_golden.GOLDEN, 'oracle_mix_pin.npz')
    fx = np.load(path, allow_pickle=False)
    assert os.path.getsize(path) <= 512 * 1024
    for n in fx.files:
        assert fx[n].dtype == np.float64, (n, fx[n].dtype)
    assert {n.split('/')[0] for n in fx.files} == {_mix.pin_tag(f, c) for f, c in _CASES}
    cover = {(c[0], c[1], bool(c[3])) for _, c in _CASES}
    assert cover == {(ks, s, se) for ks in (_mix.K35, _mix.K357) for s in (1, 2) for se in (True, False)}
    assert any(c[4] % 4 for _, c in _CASES)            # one ragged width


def test_product_cpu_module_is_the_restatement():
    """layers.MixDepthwiseConv2d (the product's parameter holder): the same packed layout, the same segment views, the same CPU
    forward as the restatement's PackedDW; its state_dict key is the plain block's"""
    from tfnas_amd.layers import MBInvertedResBlock, MixDepthwiseConv2d
    for mc, ks, s in ((53, (3, 5, 7), 1), (44, (3, 5), 2), (107, (5, 7), 1), (9, (3, 5, 7), 2)):
        torch.manual_seed(mc)
        ref = _mix.PackedDW(mc, ks, s)
        m = MixDepthwiseConv2d(mc, ks, s)
        assert m.splits == _mix.split(mc, len(ks)) and m.weight.shape == ref.weight.shape and m.weight.dim() == 1
        m.load_state_dict(ref.state_dict())
        assert [tuple(w.shape) for w in m.segment_weights()] == [(c, 1, k, k) for c, k in zip(m.splits, ks)]
        x = torch.randn(2, mc, 7, 9)
        assert torch.equal(m(x), ref(x))
    blk = MBInvertedResBlock(16, 53, 8, 16, stride=1, mix_kernels=(3, 5, 7))
    plain = MBInvertedResBlock(16, 53, 8, 16, 7, 1)
    assert list(blk.state_dict()) == list(plain.state_dict()) and blk.kernel_size == 7 and blk.mix_kernels == (3, 5, 7)
    # every segment is initialised as a depthwise convolution of its size is: bounded by 1 / sqrt(fan_in) = 1 / k_s
    for w, k in zip(blk.depth_conv.conv.segment_weights(), (3, 5, 7)):
        assert 0.5 / k < float(w.detach().abs().max()) <= 1.0 / k
