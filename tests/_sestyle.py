"""Helpers shared by the squeeze-excite style tests (tests/test_sestyle_*.py, tests/test_gpu_sestyle*.py) and by the generator of
their fixture (tests/golden/make_golden_sestyle.py).

A style is a pair (se_act, se_gate): the hidden activation of the SE branch (None: the block's own) and its gate function
('sigmoid' | 'h-sigmoid').  The CPU restatement is the oracle's own block -- ``tfnas_oracle.MBConv`` / ``DerivedBlock``,
``_fused.FusedRef``, and through them ``_kinds.MixedRef`` and the oracle ``Network`` -- run inside ``styled()``, which, in the way
``_acts.wrapped_oracle`` wraps ``tfnas_oracle._act``, swaps exactly two calls of the block's forward for its duration:
  * the ``_act`` call on the SE hidden pre-activation (the first ``_act`` after the squeeze) takes ``se_act`` instead of the block's
    activation;
  * the ``torch.sigmoid`` call that is NOT inside ``_act`` (swish's own stays) -- the gate -- becomes ``gate_fn``.
Nothing else of the oracle is restated, and with the default style both calls are delegated unchanged.  ``restyle(block, ...)``
turns an existing oracle block into its styled twin in place (same parameters, same state_dict keys)."""
import contextlib
import copy

import torch
import torch.nn.functional as F

import _acts
import _fused
import _kinds
import tfnas_oracle as orc
from _rawcell import KINKS, KINK_TAU

DEFAULT = (None, 'sigmoid')
MNV3 = ('relu', 'h-sigmoid')
GATE_KINKS = {'sigmoid': (), 'h-sigmoid': (-3.0, 3.0)}
# (cell activation, se_act, se_gate) of the GPU cell tests
STYLES = [('h-swish', 'relu', 'h-sigmoid'), ('relu', None, 'h-sigmoid'), ('swish', 'relu', 'sigmoid'), ('h-swish', None, 'h-sigmoid')]


def gate_fn(v, se_gate):
    if se_gate == 'sigmoid':
        return torch.sigmoid(v)
    if se_gate == 'h-sigmoid':
        return F.relu6(v + 3.0) / 6.0
    raise ValueError(se_gate)


class _State:
    def __init__(self, se_act, se_gate):
        self.se_act, self.se_gate = se_act, se_gate
        self.depth, self.pending = 0, False
        self.hpre, self.gpre = [], []          # what the two swapped calls were handed (kink_distance reads them)

    def mark(self, *_):
        self.pending = True

    def __deepcopy__(self, memo):              # (a block's last record is not part of the block)
        return None


class _Proxy:
    """A module whose attributes are ``base``'s except the ones given"""

    def __init__(self, base, **over):
        self.__dict__.update(over)
        self._base = base

    def __getattr__(self, name):
        return getattr(self._base, name)


@contextlib.contextmanager
def _patched(mod, st, pool_marks):
    inner, torch0, F0 = mod._act, mod.torch, mod.F

    def _act(x, act):
        if st.pending:                         # the SE hidden layer
            st.pending = False
            st.hpre.append(x.detach())
            act = act if st.se_act is None else st.se_act
        st.depth += 1
        try:
            return inner(x, act)
        finally:
            st.depth -= 1

    def sigmoid(v):
        if st.depth:                           # swish's own
            return torch.sigmoid(v)
        st.gpre.append(v.detach())
        return gate_fn(v, st.se_gate)

    def pool(x, size):
        st.mark()
        return F.adaptive_avg_pool2d(x, size)
    mod._act, mod.torch = _act, _Proxy(torch, sigmoid=sigmoid)
    if pool_marks:
        mod.F = _Proxy(F, adaptive_avg_pool2d=pool)
    try:
        yield st
    finally:
        mod._act, mod.torch, mod.F = inner, torch0, F0


@contextlib.contextmanager
def styled(se_act, se_gate):
    """The oracle (tfnas_oracle, with _acts' ReLU6 / hard-swish underneath) and _fused run a block's SE branch in this style;
    yields the record of the swapped calls' inputs."""
    st = _State(se_act, se_gate)
    with _acts.wrapped_oracle(), _patched(orc, st, True), _patched(_fused, st, False):
        yield st


class _Styled:
    se_act, se_gate = DEFAULT

    def forward(self, *a, **k):
        with styled(self.se_act, self.se_gate) as st:
            self.__dict__['_last_state'] = st      # (kink_distance reads what the two swapped calls were handed)
            hook = None
            if isinstance(self, _fused.FusedRef) and self.squeeze_excite is not None:     # (its squeeze is a tensor method)
                hook = self.squeeze_excite.conv_reduce.register_forward_pre_hook(st.mark)
            try:
                return super().forward(*a, **k)
            finally:
                if hook is not None:
                    hook.remove()


class StyledMBConv(_Styled, orc.MBConv):
    pass


class StyledDerived(_Styled, orc.DerivedBlock):
    pass


class StyledFused(_Styled, _fused.FusedRef):
    pass


_TWINS = {orc.MBConv: StyledMBConv, orc.DerivedBlock: StyledDerived, _fused.FusedRef: StyledFused}


def restyle(block, se_act=None, se_gate='sigmoid'):
    """``block`` (an oracle MBConv / DerivedBlock or a FusedRef, styled or not) as its styled twin, in place; returns it."""
    for base, twin in _TWINS.items():
        if isinstance(block, base):
            block.__class__ = twin
            block.se_act, block.se_gate = se_act, se_gate
            return block
    raise TypeError(type(block))


def restyle_all(root, se_act=None, se_gate='sigmoid', skip=()):
    """every block under ``root`` (a MixedRef, an oracle MixedOP / MixedStage / Network ...) except those under ``skip``"""
    skipped = {id(m) for s in skip for m in s.modules()}
    for m in list(root.modules()):
        if isinstance(m, tuple(_TWINS)) and id(m) not in skipped:
            restyle(m, se_act, se_gate)
    return root


# ------------------------------------------------------------------------------------------------ kinks and seeds
def kink_distance(o, x):
    """_kinds.kink_distance (BatchNorm outputs and SE hidden pre-activations against the kinks of the cell's activation) extended
    by the two kinks a style adds, all in a float64 copy of the styled MixedRef ``o``: the SE hidden pre-activations against the
    kinks of the hidden activation the style names, the gate pre-activations against +-3 of a hard-sigmoid gate."""
    dist = _kinds.kink_distance(o, x)
    o64 = copy.deepcopy(o).double()
    with torch.no_grad():
        for op in o64.m_ops:
            if op.squeeze_excite is None:
                continue
            op(x.double())
            st = op._last_state
            assert len(st.hpre) == 1 and len(st.gpre) == 1, (len(st.hpre), len(st.gpre))
            hidden = op.act_func if getattr(op, 'se_act', None) is None else op.se_act
            for kk in KINKS[hidden]:
                dist = min(dist, float((st.hpre[0] - kk).abs().min()))
            for kk in GATE_KINKS[getattr(op, 'se_gate', 'sigmoid')]:
                dist = min(dist, float((st.gpre[0] - kk).abs().min()))
    return dist


GATE_BIAS_GAIN = 30.0


def make_ref(cands, ic, oc, stride, act, se_act, se_gate, seed):
    """_kinds.make_ref with every candidate restyled.  Under a hard-sigmoid gate the gate biases (0.1 randn there) are scaled to
    a standard deviation of 3, so that a cell's gate pre-activations lie below -3, inside (-3, 3) and above 3: all three branches
    of the gate and of its derivative (gate_branches counts them)."""
    o = restyle_all(_kinds.make_ref(cands, ic, oc, stride, act, seed), se_act, se_gate)
    if se_gate == 'h-sigmoid':
        with torch.no_grad():
            for op in o.m_ops:
                if op.squeeze_excite is not None:
                    op.squeeze_excite.conv_expand.bias.mul_(GATE_BIAS_GAIN)
    return o


def gate_branches(o, x):
    """numbers of gate pre-activations (float32 restatement) at or below -3, strictly inside (-3, 3), at or above 3"""
    if not any(op.squeeze_excite is not None for op in o.m_ops):
        return None
    lo = mid = hi = 0
    with torch.no_grad():
        for op in o.m_ops:
            if op.squeeze_excite is None:
                continue
            op(x)
            v = op._last_state.gpre[0]
            lo, mid, hi = lo + int((v <= -3).sum()), mid + int(((v > -3) & (v < 3)).sum()), hi + int((v >= 3).sum())
    return lo, mid, hi


def case_data(cands, N, ic, oc, H, W, stride, act, se_act, se_gate, base=300, span=400):
    """_kinds.case_data for a styled cell: the first seed from ``base`` up whose float64 pre-activations -- the two new kinks
    included -- stay at least KINK_TAU from every kink and, under a hard-sigmoid gate, whose gate pre-activations reach all three
    branches of the gate.  Chosen on the CPU from the restatement alone."""
    for seed in range(base, base + span):
        o = make_ref(cands, ic, oc, stride, act, se_act, se_gate, seed)
        gen = torch.Generator().manual_seed(seed + 2)
        x = torch.randn(N, ic, H, W, generator=gen)
        r = torch.randn(N, oc, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
        w = torch.softmax(torch.randn(len(cands), generator=gen), -1)
        if kink_distance(o, x) >= KINK_TAU and (se_gate != 'h-sigmoid' or min(gate_branches(o, x) or (1,)) > 0):
            return o, x, r, w, seed
    raise AssertionError('no seed keeps the pre-activations clear of the kinks')


# ------------------------------------------------------------------------------------------------ product side
def style_of(o):
    """the one style of the SE candidates of a restatement (DEFAULT if it has none)"""
    st = {(getattr(op, 'se_act', None), getattr(op, 'se_gate', 'sigmoid')) for op in o.m_ops if op.squeeze_excite is not None}
    assert len(st) <= 1
    return st.pop() if st else DEFAULT


def hip_blocks_like(o):
    """_kinds.hip_blocks_like with the restatement's style on every block"""
    blocks = _kinds.hip_blocks_like(o)
    for b in blocks:
        b.set_se_style(style_of(o))
    return blocks


# ------------------------------------------------------------------------------------------------ pin (float64)
PIN_GEOM = _acts.PIN_GEOM
# (cell activation, hidden activation, stride), both forms: MobileNetV3's pairing, and one swap in each direction
PIN_HIDDEN = [(cell, se_act, s) for cell, se_act in (('h-swish', 'relu'), ('swish', 'relu'), ('relu', 'swish')) for s in (1, 2)]
PIN_FORMS = ('search', 'derived')


def pin_tag(form, case):
    return '%s_%s_se-%s_s%d' % ((form,) + tuple(case))


def pin_block(form, case, k=3):
    """The oracle's block of one pin case (float64, train mode, UNSTYLED), its input, cotangent and RNG seed (for _k7.pin_run)."""
    import _k7
    cell, _se_act, s = case
    q = PIN_GEOM
    seed = 7000 + 101 * PIN_HIDDEN.index(case) + (0 if form == 'search' else 50)
    torch.manual_seed(seed)
    cls = orc.MBConv if form == 'search' else orc.DerivedBlock
    blk = cls(q['ic'], q['mc'], q['se'], q['oc'], k, s, cell)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    if form == 'derived':
        _k7.randomise_bn(blk, gen)
        blk.drop_connect_rate = _k7.PIN_DROP
    blk = blk.double().train()
    x = torch.randn(q['N'], q['ic'], q['H'], q['W'], generator=gen).double()
    r = torch.randn(q['N'], q['oc'], (q['H'] - 1) // s + 1, (q['W'] - 1) // s + 1, generator=gen).double()
    return blk, x, r, seed + 2


class GateTwin(torch.nn.Module):
    """The gate pin's independent composition: the forward of an oracle MBConv / DerivedBlock with SE written out once more from
    torch ops around a given gate function -- ``torch.sigmoid`` must reproduce the reference's recorded block (which proves the
    composition), ``torch.nn.functional.hardsigmoid`` is then what the hard-sigmoid restatement is held to.  Holds a deep copy of
    the block's sub-modules under their names (same parameter and buffer names; the block's own buffers do not move)."""

    def __init__(self, blk, hidden, gate):
        super().__init__()
        blk = copy.deepcopy(blk)
        self.inverted_bottleneck, self.depth_conv = blk.inverted_bottleneck, blk.depth_conv
        self.squeeze_excite, self.point_linear = blk.squeeze_excite, blk.point_linear
        self.act_func, self.hidden, self.gate = blk.act_func, hidden, gate
        self.has_residual, self.drop_connect_rate = blk.has_residual, getattr(blk, 'drop_connect_rate', 0.0)
        if hasattr(blk, 'drop_u'):
            self.drop_u = None

    @staticmethod
    def _bn(seq, t):
        return seq.bn(t) if hasattr(seq, 'bn') else F.batch_norm(t, None, None, None, None, True, 0.0, orc.BN_EPS)

    def forward(self, x):
        act = _fused._act
        y = act(self._bn(self.inverted_bottleneck, self.inverted_bottleneck.conv(x)), self.act_func)
        y = act(self._bn(self.depth_conv, self.depth_conv.conv(y)), self.act_func)
        h = act(self.squeeze_excite.conv_reduce(y.mean((2, 3), keepdim=True)), self.hidden)
        y = y * self.gate(self.squeeze_excite.conv_expand(h))
        y = self._bn(self.point_linear, self.point_linear.conv(y))
        if self.has_residual:
            if self.training and self.drop_connect_rate > 0.0:
                keep = 1.0 - self.drop_connect_rate
                y = y.div(keep) * torch.floor(keep + self.drop_u.view(-1, 1, 1, 1))
            y = y + x
        return y
