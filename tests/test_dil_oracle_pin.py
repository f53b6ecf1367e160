"""Pin the CPU restatement of dilated depthwise candidates -- what tests/test_gpu_dil*.py then compare the HIP path with.

tests/_dil.py runs the oracle's own blocks with the one depthwise ``F.conv2d`` call of tfnas_oracle given padding d * (k // 2) and
dilation d (``dilated``), nothing else restated.  It is compared here, in float64, with tests/golden/oracle_dil_pin.npz, which
tests/golden/make_golden_dil.py recorded from the REFERENCE's MBInvertedResBlock with its ``depth_conv.conv`` replaced by the
dilated ``nn.Conv2d`` carrying the same weight: forward and every gradient, both (k, d) pairs, both strides, with and without SE,
with and without expand convolution, ReLU and swish, the batch-statistic and the affine form (running statistics, drop-connect),
at 2 x 16 x 9 x 13 and at 1 x 1, 3 x 5 and 12 x 10 images.  Tolerances: those of tests/test_k7_oracle_pin.py (1e-5 / 1e-5 forward
and buffers, 2e-6 / 1e-4 gradients).  With dilation 1 the wrapped call is delegated unchanged: bit-identical to the plain oracle.
The ``_kinds.MixedRef`` mix of dilated and undilated candidates equals the reference's ``MixedOP.forward`` over replaced
candidates (1e-11 relative, as tests/test_kinds_oracle_pin.py).  Where a checkout of the reference is at hand (TFNAS_REFERENCE)
the reference itself is run as well and must agree with what was recorded."""
import os

import numpy as np
import pytest
import torch

import _dil
import _golden
import _kinds
import _refload
import tfnas_oracle as orc

FWD = dict(atol=1e-5, rtol=1e-5)
GRAD = dict(atol=2e-6, rtol=1e-4)
MIX_RTOL = 1e-11
_CASES = [(form, case) for form in _dil.PIN_FORMS for case in _dil.pin_cases(form)]


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('oracle_dil_pin.npz')


def _tol(key):
    return FWD if key == 'out' or key.startswith('b.') else GRAD


def _check(res, recorded, tag, mc, k):
    want_keys = [n[len(tag) + 1:] for n in recorded.files if n.startswith(tag + '/')]
    assert list(res) == want_keys
    for key, v in res.items():
        want = recorded[tag + '/' + key]
        tol = _tol(key)
        if key == 'g.depth_conv.conv.weight':
            assert v.shape == want.shape == (mc, 1, k, k)          # (dilation never changes the weight's shape)
            assert np.allclose(v, want, **tol), (tag, key, float(abs(v - want).max()))
        else:
            t = torch.from_numpy(np.asarray(v))
            assert _golden.probe_close(_golden.probe(t), want, t.numel(), tol['atol'], tol['rtol']), (tag, key)


@pytest.mark.parametrize('form,case', _CASES, ids=[_dil.pin_tag(f, c) for f, c in _CASES])
def test_restatement_matches_the_reference_block_with_a_dilated_depth_conv(recorded, form, case):
    k, d, s, act, se, mid, N, H, W = case
    blk, x, r, seed = _dil.pin_oracle_block(form, case)
    assert _dil.dilation_of(blk) == d == 2 and tuple(blk.depth_conv.conv.padding) == (d * (k // 2),) * 2
    assert (blk.inverted_bottleneck is None) == (mid == 16)
    res = _dil.pin_run(blk, x, r, seed)
    assert res['out'].shape == (N, 16, (H - 1) // s + 1, (W - 1) // s + 1)        # the output size of every k, dilated or not
    _check(res, recorded, _dil.pin_tag(form, case), blk.mid_channels, k)
    # the dilation is not a no-op of the case: the undilated block of the same weights computes something else
    plain, _, _, _ = _dil.pin_oracle_block(form, case, dilation=1)
    if H > 1 or W > 1:
        assert float(np.abs(_dil.pin_run(plain, x, r, seed)['out'] - res['out']).max()) > 1e-3
    if _refload.available():                      # the reference itself, where it can be imported
        ref = _refload.import_reference()
        state = _dil.pin_oracle_block(form, case)[0].state_dict()          # (before a step moved the running statistics)
        rb = ref.layers.MBInvertedResBlock(16, mid, se, 16, k, s, affine=(form == 'derived'), act_func=act)
        rb.load_state_dict(state)
        mc = blk.mid_channels
        conv = torch.nn.Conv2d(mc, mc, k, s, padding=d * (k // 2), dilation=d, groups=mc, bias=False)
        conv.weight = rb.depth_conv.conv.weight
        rb.depth_conv.conv = conv
        rb.drop_connect_rate = getattr(blk, 'drop_connect_rate', 0.0)
        _check(_dil.pin_run(rb.double().train(), x, r, seed), recorded, _dil.pin_tag(form, case), mc, k)


@pytest.mark.parametrize('form', _dil.PIN_FORMS)
@pytest.mark.parametrize('k,stride,se,mid', [(3, 1, 8, 24), (5, 2, 0, 24), (5, 1, 8, 16), (7, 2, 8, 24)])
def test_dilation_1_is_bit_identical_to_the_plain_oracle(form, k, stride, se, mid):
    """the wrapped depthwise call is delegated with the arguments it came with: same bits, forward and every gradient"""
    def build():
        torch.manual_seed(31 + k)
        cls = orc.MBConv if form == 'search' else orc.DerivedBlock
        return cls(16, mid, se, 16, k, stride, 'swish').train()
    plain, wrapped = build(), _dil.dilate(build(), 1)
    assert type(wrapped) is not type(plain) or form == 'derived'
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 9, 13, generator=gen)
    r = torch.randn(2, 16, (9 - 1) // stride + 1, (13 - 1) // stride + 1, generator=gen)
    a, b = _dil.pin_run(plain, x, r, 3), _dil.pin_run(wrapped, x, r, 3)
    assert list(a) == list(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    with _dil.dilated(1) as hits:                      # (and inside the wrapper nothing is rewritten)
        c = _dil.pin_run(build(), x, r, 3)
    assert hits == [0] and all(np.array_equal(a[key], c[key]) for key in a)


def test_only_the_depthwise_call_is_rewritten():
    """under dilated(2) the oracle's 1 x 1 convolutions, SE convolutions and stem keep their arguments: one rewritten call per
    block forward, and the oracle module is what it was afterwards"""
    F0 = orc.F
    blk = orc.MBConv(16, 24, 8, 16, 5, 1, 'swish')
    with _dil.dilated(2) as hits:
        y = blk(torch.randn(2, 16, 9, 13))
    assert hits == [1] and y.shape == (2, 16, 9, 13) and orc.F is F0


@pytest.mark.parametrize('case', _dil.MIX_CASES, ids=_dil.mix_tag)
def test_mix_of_dilated_and_undilated_candidates_reproduces_the_reference_mixedop(recorded, case):
    o, x, r, la, seed = _dil.mix_case(case)
    assert [(_dil.dilation_of(op)) for op in o.m_ops] == list(_dil.MIX_DILS) and {1, 2} == set(_dil.MIX_DILS)
    assert any(op.inverted_bottleneck is None and _dil.dilation_of(op) == 2 for op in o.m_ops)      # a dilated expand-free one
    res = _kinds.pin_run(o, x, r, la, seed)
    tag = _dil.mix_tag(case)
    rec = _dil.record(res)
    assert sorted(rec) == sorted(n[len(tag) + 1:] for n in recorded.files if n.startswith(tag + '/'))
    assert res['dla'].shape == (8,) and float(np.abs(res['dla']).max()) > 0
    for n, v in rec.items():                     # (sum, sum of magnitudes, 24 sampled elements)
        want = recorded[tag + '/' + n]
        assert v.shape == want.shape
        assert abs(v[0] - want[0]) <= MIX_RTOL * want[1] and abs(v[1] - want[1]) <= MIX_RTOL * want[1], (tag, n)
        scale = max(float(np.abs(want[2:]).max()), 1e-300)
        assert float(np.abs(v[2:] - want[2:]).max()) <= MIX_RTOL * scale, (tag, n)


def test_fixture_holds_arrays_only_and_is_small():
    path = os.path.join(_golden.GOLDEN, 'oracle_dil_pin.npz')
    fx = np.load(path, allow_pickle=False)
    assert os.path.getsize(path) <= 512 * 1024
    for n in fx.files:
        assert fx[n].dtype == np.float64, (n, fx[n].dtype)
    want = {_dil.pin_tag(f, c) for f, c in _CASES} | {_dil.mix_tag(c) for c in _dil.MIX_CASES}
    assert {n.split('/')[0] for n in fx.files} == want
    cover = {(c[0], c[1], c[2], c[3], bool(c[4]), c[5] > 16) for _, c in _CASES}
    assert {c[:3] for c in cover} == {(k, d, s) for k, d in _dil.PAIRS for s in (1, 2)}
    assert {c[3] for c in cover} == {'relu', 'swish'} and {c[4] for c in cover} == {c[5] for c in cover} == {True, False}


def test_networkcfg_reads_the_dilation_key():
    """what catches, on the CPU, a NetworkCfg that drops the key and computes an undilated block: the module built from a config
    with dilated stage-5 blocks holds dilated depthwise convolutions of the unchanged weight shape, exports the config it was
    built from, and the restatement's network gets the same blocks from _dil.dilate_network"""
    from tfnas_amd import model_eval as me
    cfg = _dil.dil_network_config(20)
    net = me.NetworkCfg(20, cfg)
    got = [(b.kernel_size, b.dilation, tuple(b.depth_conv.conv.dilation), tuple(b.depth_conv.conv.padding)) for b in net.stage5]
    assert got == [(k, d, (d, d), (d * (k // 2),) * 2) for k, d in _dil.DIL_STAGE5]
    assert [tuple(b.depth_conv.conv.weight.shape[1:]) for b in net.stage5] == [(1, k, k) for k, _ in _dil.DIL_STAGE5]
    assert all(b.dilation == 1 for st in (net.stage1, net.stage2, net.stage3, net.stage4, net.stage6) for b in st)
    assert net.config == cfg
    arch = {st: {'block%d' % (i + 1): (j * 3 + i) % 8 for i in range(2)} for j, st in enumerate(orc.STAGE_CFG)}
    arch['stage6'] = {'block1': 7}
    o = _dil.dilate_network(orc.DerivedNetwork(20, arch, orc.initial_mc_num_dddict()))
    assert [(b.kernel_size, tuple(b.depth_conv.conv.dilation)) for b in o.stage5] == [(k, (d, d)) for k, d in _dil.DIL_STAGE5]
    sd = net.state_dict()
    assert list(sd) == list(o.state_dict()) and all(sd[k].shape == v.shape for k, v in o.state_dict().items())
