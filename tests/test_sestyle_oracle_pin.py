"""Pin the CPU restatement of squeeze-excite styles (tests/_sestyle.py) -- what tests/test_gpu_sestyle*.py then rely on it for.

  * Default style: a restyled oracle block is the oracle block, bit for bit (the wrapper delegates both swapped calls).
  * Hidden activation: oracle.MBConv / oracle.DerivedBlock restyled with another hidden activation against the reference's own
    MBInvertedResBlock.forward over a block whose ``squeeze_excite.act`` module was replaced (recorded by
    tests/golden/make_golden_sestyle.py into tests/golden/oracle_sestyle_pin.npz and replayed here; where a checkout of the
    reference is at hand -- TFNAS_REFERENCE -- the reference itself runs as well): output, dx, every parameter gradient and the
    derived form's buffers, both forms, strides 1 and 2, float64, the tolerances of make_golden_act.py's on-the-spot comparison.
  * Gate: the reference hard-codes torch.sigmoid in that forward, so the hard-sigmoid gate is pinned to
    torch.nn.functional.hardsigmoid composed in float64 with autograd gradients (_sestyle.GateTwin); the same composition around
    torch.sigmoid must reproduce the reference's recorded logistic twin, which is what proves the composition."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fused
import _golden
import _k7
import _kinds
import _refload
import _sestyle as S
import tfnas_oracle as orc

TOL = dict(atol=2e-6, rtol=1e-4)           # make_golden_act.py's on-the-spot comparison


@pytest.fixture(scope='module')
def recorded():
    return _golden.load('oracle_sestyle_pin.npz')


def _check(res, recorded, tag):
    want_keys = [k[len(tag) + 1:] for k in recorded.files if k.startswith(tag + '/')]
    assert list(res) == want_keys
    for k, v in res.items():
        want = recorded[tag + '/' + k]
        if k == 'g.depth_conv.conv.weight':
            assert np.allclose(v, want, **TOL), (tag, k, float(abs(v - want).max()))
        else:
            t = torch.from_numpy(np.asarray(v))
            assert _golden.probe_close(_golden.probe(t), want, t.numel(), TOL['atol'], TOL['rtol']), (tag, k)


# ------------------------------------------------------------------------------------------------ default style
@pytest.mark.parametrize('act', ('relu', 'swish', 'relu6', 'h-swish'))
def test_default_style_is_the_oracle_block_bitwise(act):
    o = _kinds.make_ref(_kinds.EIGHT, 8, 8, 1, act, 11)
    s = S.restyle_all(copy.deepcopy(o))
    assert all(type(a) is not type(b) for a, b in zip(o.m_ops, s.m_ops))
    gen = torch.Generator().manual_seed(12)
    x, r, w = torch.randn(2, 8, 7, 9, generator=gen), torch.randn(2, 8, 7, 9, generator=gen), torch.rand(8, generator=gen)
    a, b = _kinds.ref_run(o, x, r, w), _kinds.ref_run(s, x, r, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert list(a[3]) == list(b[3]) and all(torch.equal(a[3][k], b[3][k]) for k in a[3])
    assert list(o.state_dict()) == list(s.state_dict())


def test_default_style_of_a_derived_block_is_the_oracle_block_bitwise():
    blk, x, r, seed = S.pin_block('derived', S.PIN_HIDDEN[0])
    styled = S.restyle(copy.deepcopy(blk))
    with S._acts.wrapped_oracle():                 # (the unstyled h-swish block needs the activation wrapper, the styled one brings it)
        a = _k7.pin_run(copy.deepcopy(blk), x, r, seed)
    b = _k7.pin_run(styled, x, r, seed)
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ hidden activation
@pytest.mark.parametrize('case', S.PIN_HIDDEN, ids=lambda c: '%s_se-%s_s%d' % c)
@pytest.mark.parametrize('form', S.PIN_FORMS)
def test_restyled_hidden_activation_matches_reference(recorded, form, case):
    cell, se_act, s = case
    blk, x, r, seed = S.pin_block(form, case)
    state = copy.deepcopy(blk.state_dict())
    res = _k7.pin_run(S.restyle(blk, se_act, 'sigmoid'), x, r, seed)
    assert res['out'].shape == (2, 16, (9 - 1) // s + 1, (13 - 1) // s + 1)
    _check(res, recorded, S.pin_tag(form, case))
    # the swap changes the result (the pinned cases are not the default style in disguise)
    plain, _, _, _ = S.pin_block(form, case)
    with S._acts.wrapped_oracle():
        base = _k7.pin_run(plain, x, r, seed)
    assert float(abs(base['out'] - res['out']).max()) > 1e-3
    if _refload.available():                      # the reference itself, where it can be imported
        import torch.nn as nn
        ref = _refload.import_reference()
        q = S.PIN_GEOM
        rb = ref.layers.MBInvertedResBlock(q['ic'], q['mc'], q['se'], q['oc'], 3, s, affine=(form == 'derived'), act_func=cell)
        rb.load_state_dict(state)
        rb.squeeze_excite.act = {'relu': nn.ReLU(), 'swish': ref.layers.Swish()}[se_act]
        rb.drop_connect_rate = getattr(blk, 'drop_connect_rate', 0.0)
        live = _k7.pin_run(rb.double().train(), x, r, seed)
        _check(live, recorded, S.pin_tag(form, case))
        for kk in live:
            assert np.allclose(res[kk], live[kk], **TOL), (form, case, kk)


def test_hidden_layer_of_the_pin_reaches_both_sides_of_its_kink():
    for form in S.PIN_FORMS:
        for case in S.PIN_HIDDEN:
            if case[1] != 'relu':
                continue
            blk, x, r, seed = S.pin_block(form, case)
            blk = S.restyle(blk, case[1], 'sigmoid')
            with torch.no_grad():
                blk(x)
            h = blk._last_state.hpre[0]
            assert int((h > 0).sum()) > 0 and int((h < 0).sum()) > 0


# ------------------------------------------------------------------------------------------------ gate
@pytest.mark.parametrize('case', S.PIN_HIDDEN, ids=lambda c: '%s_se-%s_s%d' % c)
@pytest.mark.parametrize('form', S.PIN_FORMS)
def test_gate_twin_reproduces_the_reference_and_pins_the_hard_sigmoid(recorded, form, case):
    cell, se_act, s = case
    blk, x, r, seed = S.pin_block(form, case)
    # the composition around torch.sigmoid is the reference's recorded block ...
    _check(_k7.pin_run(S.GateTwin(blk, se_act, torch.sigmoid), x, r, seed), recorded, S.pin_tag(form, case))
    # ... and around hardsigmoid it is what the hard-sigmoid restatement computes; the gate biases are spread over (-5, 5) so that
    # the gate saturates on both sides (all three branches of hardsigmoid and of its derivative)
    with torch.no_grad():
        bias = blk.squeeze_excite.conv_expand.bias
        bias.copy_(torch.linspace(-5.0, 5.0, bias.numel(), dtype=bias.dtype))
    want = _k7.pin_run(S.GateTwin(blk, se_act, F.hardsigmoid), x, r, seed)
    styled = S.restyle(copy.deepcopy(blk), se_act, 'h-sigmoid')
    got = _k7.pin_run(styled, x, r, seed)
    v = styled._last_state.gpre[0]
    assert min(int((v <= -3).sum()), int(((v > -3) & (v < 3)).sum()), int((v >= 3).sum())) > 0
    assert float((v.abs() - 3).abs().min()) > 1e-6
    assert list(got) == list(want)
    for k in want:
        assert np.allclose(got[k], want[k], **TOL), (form, case, k, float(abs(got[k] - want[k]).max()))
    assert float(abs(got['out'] - _k7.pin_run(S.GateTwin(blk, se_act, torch.sigmoid), x, r, seed)['out']).max()) > 1e-3


def test_gate_function_is_torch_hardsigmoid():
    v = torch.linspace(-8, 8, 161, dtype=torch.float64)
    assert torch.allclose(S.gate_fn(v, 'h-sigmoid'), F.hardsigmoid(v), atol=1e-15)
    assert torch.equal(S.gate_fn(v, 'sigmoid'), torch.sigmoid(v))
    with pytest.raises(ValueError):
        S.gate_fn(v, 'tanh')


def test_fused_restatement_takes_the_style():
    """_fused.FusedRef under a style: default bit for bit, and the styled forward written out by hand"""
    blk = _fused.ref_block(8, 22, 8, 8, 1, 'h-swish', 5).double()
    x = torch.randn(2, 8, 7, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        base = blk(x)
        assert torch.equal(S.restyle(copy.deepcopy(blk))(x), base)
        got = S.restyle(copy.deepcopy(blk), 'relu', 'h-sigmoid')(x)
        z = _fused._act(F.batch_norm(blk.fused_conv.conv(x), None, None, None, None, True, 0.0, 1e-5), 'h-swish')
        h = F.relu(blk.squeeze_excite.conv_reduce(z.mean((2, 3), keepdim=True)))
        z = z * F.hardsigmoid(blk.squeeze_excite.conv_expand(h))
        want = F.batch_norm(blk.point_linear.conv(z), None, None, None, None, True, 0.0, 1e-5) + x
    assert torch.allclose(got, want, atol=1e-12) and float((got - base).abs().max()) > 1e-3


def test_wrappers_are_removed():
    a, t, f = orc._act, orc.torch, orc.F
    with S.styled('relu', 'h-sigmoid'):
        assert orc._act is not a and orc.torch is not t and _fused.torch is not torch
    assert orc._act is a and orc.torch is t and orc.F is f and _fused.torch is torch and _fused.F is F


def test_fixture_holds_arrays_only_and_is_small():
    path = os.path.join(_golden.GOLDEN, 'oracle_sestyle_pin.npz')
    fx = np.load(path, allow_pickle=False)
    assert os.path.getsize(path) <= 364324
    assert len({k.split('/')[0] for k in fx.files}) == len(S.PIN_FORMS) * len(S.PIN_HIDDEN) == 12
    for k in fx.files:
        assert fx[k].dtype.kind == 'f', (k, fx[k].dtype)
