"""Helpers shared by the tests of the skip (identity) candidate of residual cells (TFNAS_CELL_SKIP / TFNAS_GROUP_SKIP:
tests/test_skip_oracle_pin.py, tests/test_skip_abi.py, tests/test_gpu_skip.py, tests/test_gpu_skip_search.py), built on
tests/_kinds.py and tests/_rawcell.py as they are.

A candidate is written as in _kinds -- ('M', mid, k, se), ('N', k, se), ('F', mid, se) -- or ('S',): the identity.  The restatement
is _kinds.MixedRef with an identity module in the ('S',) slots: out = sum_g w[g] candidate_g(x), every MBConv candidate adding x
itself and the identity candidate being x.  A skip has no pre-activation, so the kink distance of a cell is that of its computing
candidates."""
import ctypes as C
from collections import OrderedDict

import torch
import torch.nn as nn

import _kinds
import _rawcell

S = ('S',)
M, N, F = ('M', 22, 3, 0), ('N', 3, 0), ('F', 22, 8)
MNFS = [M, N, F, S]
EIGHT_S = _kinds.EIGHT[:7] + [S]
EIGHT_SS = _kinds.EIGHT[:6] + [S, S]
MSS = [M, S, S]
SMALL_SHAPE = _kinds.SMALL_SHAPE                  # 2 x 8 x 7 x 9, in = out = 8
SMALL_GEOM = SMALL_SHAPE + (1,)
# ic = oc = 40: another row-lane split of the BN3-backward sums than oc = 8; all-plain computing groups, and one alone.  (A plain
# MBConv block is wider than its input -- mid <= in is the expand-free kind, _kinds.ref_candidate -- so the second plain group of
# the two-group case has 64 mid channels, not fewer than its 40 input channels.)
WIDE_GEOM = (2, 40, 40, 5, 6, 1)
WIDE_CASES = [[('M', 48, 3, 0), S], [('M', 48, 5, 8), ('M', 64, 3, 0), S]]
# the fx-eligible late cell of tests/test_act_abi.py (14 x 14, ic = oc = 80, N = 8, mids 240 / 480, SE 0 / 80) plus a skip
FX_GEOM = (8, 80, 80, 14, 14, 1)
FX_CANDS = [('M', 240, 3, 0), ('M', 480, 5, 80)]
# every GPU case with a kinked activation (asserted to find its seed by tests/test_skip_oracle_pin.py)
KINKED_CASES = [(MNFS, SMALL_GEOM, act) for act in _kinds.KINKED_ACTS]


def is_skip(c):
    return c[0] == 'S'


def computing(cands):
    return [c for c in cands if not is_skip(c)]


class IdentityRef(nn.Module):
    """The identity candidate of the restatement: no parameters; the attributes oracle.MixedOP.get_lookup_latency reads."""
    name = 'IdentityLayer'
    se_channels = kernel_size = mid_channels = 0
    stride = 1
    act_func = None
    squeeze_excite = inverted_bottleneck = None

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels

    def forward(self, x, det=None):
        return x


def identity_lut_key(op, size):
    """the key oracle.MixedOP.get_lookup_latency forms for an IdentityRef"""
    return '{}_{}_{}_{}_{}_k{}_s{}_{}'.format(op.name, size, op.in_channels, op.se_channels, op.out_channels, op.kernel_size,
                                              op.stride, op.act_func)


class SkipLut(_kinds.AnyLut):
    """_kinds.AnyLut whose IdentityLayer keys map to {0: 0.0}"""

    def __missing__(self, key):
        if key.startswith('IdentityLayer_'):
            v = self[key] = {0: 0.0}
            return v
        return super().__missing__(key)


class SkipRef(_kinds.MixedRef):
    """_kinds.MixedRef over candidates that may be ('S',)"""

    def __init__(self, cands, ic, oc, stride, act, ops=None):
        nn.Module.__init__(self)
        self.cands, self.in_channels, self.out_channels, self.stride, self.act_func = list(cands), ic, oc, stride, act
        if ops is None:
            ops = [IdentityRef(ic, oc) if is_skip(c) else _kinds.ref_candidate(c, ic, oc, stride, act) for c in cands]
        self.m_ops = nn.ModuleList(ops)


def make_ref(cands, ic, oc, stride, act, seed):
    """SkipRef (float32, train mode) seeded as _kinds.make_ref seeds a MixedRef"""
    torch.manual_seed(seed)
    o = SkipRef(cands, ic, oc, stride, act)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    return o.train()


def without_skips(o):
    """the restatement of the same cell without its skip candidates, over the SAME modules (shared weights)"""
    keep = [g for g, c in enumerate(o.cands) if not is_skip(c)]
    return SkipRef([o.cands[g] for g in keep], o.in_channels, o.out_channels, o.stride, o.act_func,
                   ops=[o.m_ops[g] for g in keep]).train()


def case_data(cands, N, ic, oc, H, W, stride, act, base=300):
    """_kinds.case_data for candidates that may be ('S',): the first seed from ``base`` up, within 200 tries, whose float64
    pre-activations of every candidate stay KINK_TAU from every kink; chosen from the restatement alone, no element exempted."""
    for seed in range(base, base + 200):
        o = make_ref(cands, ic, oc, stride, act, seed)
        gen = torch.Generator().manual_seed(seed + 2)
        x = torch.randn(N, ic, H, W, generator=gen)
        r = torch.randn(N, oc, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
        w = torch.softmax(torch.randn(len(cands), generator=gen), -1)
        if _kinds.kink_distance(o, x) >= _kinds.KINK_TAU:
            return o, x, r, w, seed
    raise AssertionError('no seed keeps the pre-activations clear of the kinks')


# ------------------------------------------------------------------------------------------------ product side
def hip_blocks_like(o):
    """the product's blocks on cuda with the restatement's geometry and weights, in candidate order (IdentityLayer for a skip)"""
    from tfnas_amd.layers import IdentityLayer
    comp = _kinds.hip_blocks_like(without_skips(o))
    it = iter(comp)
    return [IdentityLayer(o.in_channels, o.out_channels) if is_skip(c) else next(it) for c in o.cands]


def hip_plan(o, blocks=None):
    from tfnas_amd.functions import CellPlan
    blocks = hip_blocks_like(o) if blocks is None else blocks
    return CellPlan(o.in_channels, o.out_channels, o.stride, o.act_func, blocks, mixed_kinds=True)


def primitives_of(cands):
    """registry names of an 8-candidate list that may hold ('S',)"""
    return [('skip' if is_skip(c) else _kinds.primitives_of([c])[0]) for c in cands]


# ------------------------------------------------------------------------------------------------ raw ABI
def skip_desc(cands, N, H, W, ic, oc, stride=1, act=0, flags=None, mode=0):
    """An unplanned TFNAS_CELL_KINDS | TFNAS_CELL_SKIP descriptor of ``cands`` (in their order: a wrong order stays wrong);
    ``flags`` overrides what a well-formed one says."""
    from tfnas_amd import _lib
    comp = computing(cands)
    d = _kinds.mixed_desc(comp, N, H, W, ic, oc, stride, act, mode=mode)
    src = [(d.g[g].mc, d.g[g].k, d.g[g].se, d.g[g].kind) for g in range(len(comp))]
    it = iter(src)
    for g, c in enumerate(cands):
        gr = d.g[g]
        gr.mc, gr.k, gr.se, gr.kind = (0, 0, 0, _lib.GROUP_SKIP) if is_skip(c) else next(it)
    d.G = len(cands)
    d.flags = (d.flags | _lib.CELL_SKIP) if flags is None else flags
    return d


def ws_fields(ws):
    return OrderedDict((n, int(getattr(ws, n))) for n, _ in ws._fields_)


class RawSkip(_kinds.RawMixed):
    """_kinds.RawMixed for a restatement with skip candidates: a KINDS | SKIP descriptor, guard bands after every buffer, Pr and
    stats sized by tfnas_cell_ws (the computing groups'), wmix and dwmix by the caller's G."""

    def __init__(self, o, x, w, guard=64):
        lb = self._lib = _rawcell._lib()
        self.lib, self.o, self.guard = lb.lib(), o, guard
        self.dev = torch.device('cuda')
        N, _, H, W = x.shape
        self.xh = x.permute(0, 2, 3, 1).contiguous().cuda()
        self.wmix = w.float().contiguous().cuda()
        self.d = skip_desc(o.cands, N, H, W, o.in_channels, o.out_channels, o.stride, lb.act_id(o.act_func))
        lb.check(self.lib.tfnas_cell_plan(C.byref(self.d)), 'tfnas_cell_plan')
        self.ws = _rawcell.ws_of(self.lib, self.d)
        self.names, self.w, self.slots = [], [], []
        for g, (c, op) in enumerate(zip(o.cands, o.m_ops)):
            if is_skip(c):
                continue
            kind = _kinds.kind_of(c)
            sd = dict(op.named_parameters())
            for k, n in zip(kind.bound(op.se_channels > 0), _rawcell.param_names(kind, op.se_channels)):
                t = sd[n].detach().float().contiguous().cuda()
                self.names.append('g%d.%s' % (g, n))
                self.w.append(t)
                self.slots.append((g, k))
                setattr(self.d.g[g], lb._W_FIELDS[k], t.data_ptr())
        self.bufs = OrderedDict()


# ------------------------------------------------------------------------------------------------ pin (float64)
PIN_T = _kinds.PIN_T
PIN_CASES = [(tuple(MNFS), act, 1) for act in _kinds.PIN_ACTS] + [(tuple(EIGHT_S), 'swish', 1), (tuple(MSS), 'swish', 1)]


def pin_tag(case):
    return 'G%d_%s_%s' % (len(case[0]), ''.join(c[0] for c in case[0]), case[1])


def pin_case(case):
    """The restatement of one pin case (float64, train mode), its input, cotangent, log_alphas and the Gumbel seed"""
    cands, act, s = case
    N, ic, oc, H, W = SMALL_SHAPE
    seed = 9100 + 97 * PIN_CASES.index(case)
    o = make_ref(cands, ic, oc, s, act, seed).double()
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(N, ic, H, W, generator=gen).double()
    r = torch.randn(N, oc, H, W, generator=gen).double()
    la = torch.log_softmax(0.5 * torch.randn(len(cands), generator=gen), -1).double()
    return o, x, r, la, seed + 3


def pin_lat(o, w, size):
    """sum_g w_g lat_g as MixedOP.forward forms it, from the restatement's own lookup (SkipLut) -- the skip's latency is 0"""
    import tfnas_oracle as orc
    cell = orc.MixedOP.__new__(orc.MixedOP)
    nn.Module.__init__(cell)
    for op in o.m_ops:                           # (_fused.FusedRef carries no name of its own: the product block's)
        if not hasattr(op, 'name'):
            op.name = 'FusedMBConvBlock'
    cell.m_ops, cell.lat_lookup = o.m_ops, SkipLut()
    lats = cell.get_lookup_latency(size)
    return lats, sum(w_g * lat for w_g, lat in zip(w, lats))


def pin_run(o, x, r, la, seed):
    """_kinds.pin_run plus 'out_lat' (the expected latency) and 'lats' (the looked-up row, which ends in the skip's 0)"""
    import numpy as np
    import tfnas_oracle as orc
    for p in o.parameters():
        p.grad = None
    xs = x.clone().requires_grad_(True)
    lap = la.clone().requires_grad_(True)
    torch.manual_seed(seed)
    w = orc.gumbel_softmax(lap, PIN_T, None)
    y = o(xs, w)
    (y * r).sum().backward()
    res = _kinds.pin_collect(y, xs, lap, o.m_ops)
    lats, out_lat = pin_lat(o, w, x.size(-1))
    res['out_lat'] = np.asarray([float(out_lat.detach())])
    res['lats'] = np.asarray([float(v) for v in lats])
    return res
