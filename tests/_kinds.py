"""Helpers shared by the tests of cells whose candidates differ in kind (TFNAS_CELL_KINDS: tests/test_kinds_abi.py,
tests/test_gpu_kinds.py): a CPU restatement of such a cell as the weighted sum of the existing restatement blocks (the oracle's
MBConv for plain and expand-free candidates, _fused.FusedRef for Fused-MBConv ones), product blocks / a product MixedOP with
identical weights, seeds whose float64 pre-activations stay clear of every activation kink, and a raw-ABI launcher for what the
Python modules do not expose (accumulation, dx == NULL, need_wgrad = 0, guard bands).

A candidate is written ('M', mid, k, se) -- plain MBConv --, ('N', k, se) -- expand-free, mid = in -- or ('F', mid, se) --
Fused-MBConv."""
import contextlib
import copy
import ctypes as C
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

import _acts
import _fused
import _rawcell
import tfnas_oracle as orc
from _rawcell import KINKS, KINK_TAU

# the 8-candidate cell of tests/test_gpu_kinds.py (ic = 8): every kind, kernel sizes 3 / 5 / 7, SE on and off, ragged widths, a
# fused block of mid == in
EIGHT = [('M', 22, 3, 0), ('F', 22, 8), ('N', 5, 0), ('M', 44, 5, 8), ('F', 36, 0), ('N', 3, 8), ('M', 24, 7, 0), ('F', 8, 0)]
THREE = [('M', 22, 3, 0), ('N', 3, 0), ('F', 22, 8)]
TILE5 = [('F', 50, 8), ('M', 50, 3, 0), ('N', 5, 8), ('M', 72, 5, 0), ('F', 24, 0)]
# (N, ic, oc, H, W, stride) of the 8-candidate swish cells: residual + ragged width, stride 2, an even width
EIGHT_SHAPES = [(2, 8, 8, 7, 9, 1), (2, 8, 12, 7, 9, 2), (2, 8, 8, 9, 6, 2)]
SMALL_SHAPE = (2, 8, 8, 7, 9)
KINKED_ACTS = ('relu', 'relu6', 'h-swish')


def kind_of(c):
    from tfnas_amd import _lib
    return {'M': _lib.MBCONV, 'N': _lib.NOEXPAND, 'F': _lib.FUSED}[c[0]]


def acts_ctx(act):
    """the oracle's activation table covers relu / swish; relu6 / h-swish run inside _acts.wrapped_oracle()"""
    return _acts.wrapped_oracle() if act in _acts.NEW_ACTS else contextlib.nullcontext()


def ref_candidate(c, ic, oc, stride, act):
    if c[0] == 'M':
        assert c[1] > ic
        return orc.MBConv(ic, c[1], c[3], oc, c[2], stride, act)
    if c[0] == 'N':
        return orc.MBConv(ic, ic, c[2], oc, c[1], stride, act)
    return _fused.FusedRef(ic, c[1], c[2], oc, stride, act)


class MixedRef(nn.Module):
    """out = sum_g w[g] * candidate_g(x): the soft branch of MixedOP.forward over restatement blocks of any kind (each block adds
    its own residual, as the reference's do)."""

    def __init__(self, cands, ic, oc, stride, act):
        super().__init__()
        self.cands, self.in_channels, self.out_channels, self.stride, self.act_func = list(cands), ic, oc, stride, act
        self.m_ops = nn.ModuleList(ref_candidate(c, ic, oc, stride, act) for c in cands)

    def forward(self, x, w, dets=None):
        with acts_ctx(self.act_func):
            ys = []
            for g, op in enumerate(self.m_ops):
                det = None if dets is None else dets.setdefault(g, {})
                ys.append(op(x, det))
        return sum(w[g] * y for g, y in enumerate(ys))


def make_ref(cands, ic, oc, stride, act, seed):
    """MixedRef (float32, train mode) with seeded weights and non-trivial SE biases"""
    torch.manual_seed(seed)
    o = MixedRef(cands, ic, oc, stride, act)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    return o.train()


def kink_distance(o, x):
    """Smallest distance, in a float64 copy of ``o``, of any BatchNorm output that feeds an activation or any SE hidden
    pre-activation of any candidate from a kink of the cell's activation (inf for swish)."""
    kinks = KINKS[o.act_func]
    if not kinks:
        return float('inf')
    o64 = copy.deepcopy(o).double()
    dets = {}
    with torch.no_grad():
        o64(x.double(), torch.ones(len(o.m_ops), dtype=torch.float64), dets)
        zs = []
        for g, op in enumerate(o64.m_ops):
            det = dets[g]
            if isinstance(op, _fused.FusedRef):
                zs += list(det.values())                     # zh, hpre
                continue
            zs += [det[k] for k in ('Eh', 'Dh') if k in det]
            if op.squeeze_excite is not None:
                se = op.squeeze_excite
                zs.append(F.conv2d(det['pooled'], se.conv_reduce.weight, se.conv_reduce.bias))
    return min(float((z - kk).abs().min()) for z in zs for kk in kinks)


def case_data(cands, N, ic, oc, H, W, stride, act, base=300):
    """(restatement, x, cotangent, Exp(1) noise -> mix weights, seed): the first seed from ``base`` up whose float64
    pre-activations of EVERY candidate stay at least KINK_TAU from every kink (swish takes ``base``).  Chosen on the CPU from the
    restatement alone; no element is ever exempted from a comparison."""
    for seed in range(base, base + 200):
        o = make_ref(cands, ic, oc, stride, act, seed)
        gen = torch.Generator().manual_seed(seed + 2)
        x = torch.randn(N, ic, H, W, generator=gen)
        r = torch.randn(N, oc, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
        w = torch.softmax(torch.randn(len(cands), generator=gen), -1)
        if kink_distance(o, x) >= KINK_TAU:
            return o, x, r, w, seed
    raise AssertionError('no seed keeps the pre-activations clear of the kinks')


def ref_run(o, x, r, w):
    """out, dx, dw and {'g<g>.<parameter>': gradient} of one forward + backward of the restatement"""
    for p in o.parameters():
        p.grad = None
    xs = x.clone().requires_grad_(True)
    ws = w.clone().requires_grad_(True)
    y = o(xs, ws)
    (y * r).sum().backward()
    grads = OrderedDict()
    for g, op in enumerate(o.m_ops):
        for k, p in op.named_parameters():
            grads['g%d.%s' % (g, k)] = p.grad.clone()
    return y.detach(), xs.grad, ws.grad, grads


# ------------------------------------------------------------------------------------------------ product side
def hip_blocks_like(o):
    """the product's blocks on cuda with the restatement's geometry and weights, in candidate order"""
    from tfnas_amd.layers import FusedMBConvBlock, MBInvertedResBlock
    out = []
    for op in o.m_ops:
        cls = FusedMBConvBlock if isinstance(op, _fused.FusedRef) else MBInvertedResBlock
        m = cls(op.in_channels, op.mid_channels, op.se_channels, op.out_channels, op.kernel_size, op.stride, affine=False,
                act_func=o.act_func)
        m.load_state_dict(op.state_dict())
        out.append(m.cuda())
    return out


def hip_plan(o, blocks=None):
    from tfnas_amd.functions import CellPlan
    blocks = hip_blocks_like(o) if blocks is None else blocks
    return CellPlan(o.in_channels, o.out_channels, o.stride, o.act_func, blocks, mixed_kinds=True)


def hip_run(plan, x, r, w, need_wgrad):
    """out, dx, dw and the gradients (ref_run's names; None without need_wgrad) of one launch pair through MixedOpFn"""
    from tfnas_amd.functions import MixedOpFn
    params = plan.params()
    for p in params:
        p.requires_grad_(need_wgrad)
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wm = w.cuda().requires_grad_(True)
    y = MixedOpFn.apply(plan, xm, wm, *params)
    (y * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = None
    if need_wgrad:
        grads = OrderedDict()
        for g, b in enumerate(plan.blocks):
            for k, p in b.named_parameters():
                assert p.grad is not None, (g, k)
                grads['g%d.%s' % (g, k)] = p.grad.clone()
    return y.detach(), xm.grad, wm.grad, grads


def compare(ref, got):
    """{name: (max abs error, max |reference|)} for _hipcheck.worst"""
    import _hipcheck as hc
    res = OrderedDict(out=hc.err(got[0], ref[0]), dx=hc.err(got[1], ref[1]), dwmix=hc.err(got[2], ref[2]))
    if got[3] is not None:
        assert list(got[3]) == list(ref[3])
        for k in ref[3]:
            res[k] = hc.err(got[3][k], ref[3][k])
    return res


def primitives_of(cands):
    """registry names (model_search.OPS) of an 8-candidate list; widths go through mc_num_dict"""
    names = []
    for c in cands:
        if c[0] == 'M':
            names.append('MBI_k%d_e3%s' % (c[2], '_se' if c[3] else ''))
        elif c[0] == 'N':
            names.append('DS_k%d%s' % (c[1], '_se' if c[2] else ''))
        else:
            names.append('FMB_k3_e3%s' % ('_se' if c[2] else ''))
    return names


class AnyLut(dict):
    """every key -> {mid: a deterministic latency}"""

    def __missing__(self, key):
        base = 0.25 + 0.003 * (sum(map(ord, key)) % 97)
        v = self[key] = _Row(base)
        return v


class _Row(dict):
    def __init__(self, base):
        super().__init__()
        self.base = base

    def __missing__(self, mid):
        v = self[mid] = self.base + 0.001 * int(mid)
        return v


def hip_mixedop_like(o, T=2.5):
    """the product's MixedOP(primitives=...) on cuda for an 8-candidate restatement whose SE widths are the registry's (ic x 1)"""
    from tfnas_amd.model_search import MixedOP
    mc = OrderedDict((g, op.mid_channels) for g, op in enumerate(o.m_ops))
    m = MixedOP(o.in_channels, o.out_channels, o.stride, False, o.act_func, 8, mc, AnyLut(), primitives=primitives_of(o.cands))
    for op, blk in zip(o.m_ops, m.m_ops):
        blk.load_state_dict(op.state_dict())
    m.set_temperature(T)
    return m.cuda()


# ------------------------------------------------------------------------------------------------ raw ABI
def mixed_desc(cands, N, H, W, ic, oc, stride=1, act=0, flags=None, kinds=None, mode=0):
    """An unplanned TFNAS_CELL_KINDS descriptor of ``cands``; ``flags`` / ``kinds`` override what a well-formed one says."""
    from tfnas_amd import _lib
    d = _lib.TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, H, W, ic, oc, stride, act, len(cands), mode
    d.has_res, d.eps = int(ic == oc and stride == 1), _lib.BN_EPS
    k7 = False
    for g, c in enumerate(cands):
        gr = d.g[g]
        if c[0] == 'M':
            gr.mc, gr.k, gr.se = c[1], c[2], c[3]
        elif c[0] == 'N':
            gr.mc, gr.k, gr.se = ic, c[1], c[2]
        else:
            gr.mc, gr.k, gr.se = c[1], 3, c[2]
        gr.kind = _lib.group_kind_id(kind_of(c)) if kinds is None else kinds[g]
        k7 = k7 or gr.k == 7
    d.flags = (_lib.CELL_KINDS | (_lib.CELL_K7 if k7 else 0) | _lib.act_flags(act)) if flags is None else flags
    return d


class RawMixed(_rawcell.RawCell):
    """A mixed cell through tfnas_mixedop_fwd / _bwd with caller-made buffers: ``guard`` sentinel floats follow EVERY workspace
    buffer; TFNAS_CELL_ACCUM_WGRAD, need_wgrad and dx == NULL are the caller's choice.  Weights: the restatement's."""

    def __init__(self, o, x, w, guard=64):
        lb = self._lib = _rawcell._lib()
        self.lib, self.o, self.guard = lb.lib(), o, guard
        self.dev = torch.device('cuda')
        N, _, H, W = x.shape
        self.xh = x.permute(0, 2, 3, 1).contiguous().cuda()
        self.wmix = w.float().contiguous().cuda()
        self.d = mixed_desc(o.cands, N, H, W, o.in_channels, o.out_channels, o.stride, lb.act_id(o.act_func))
        lb.check(self.lib.tfnas_cell_plan(C.byref(self.d)), 'tfnas_cell_plan')
        self.ws = _rawcell.ws_of(self.lib, self.d)
        self.names, self.w, self.slots = [], [], []
        for g, (c, op) in enumerate(zip(o.cands, o.m_ops)):
            kind = kind_of(c)
            sd = dict(op.named_parameters())
            for k, n in zip(kind.bound(op.se_channels > 0), _rawcell.param_names(kind, op.se_channels)):
                t = sd[n].detach().float().contiguous().cuda()
                self.names.append('g%d.%s' % (g, n))
                self.w.append(t)
                self.slots.append((g, k))
                setattr(self.d.g[g], lb._W_FIELDS[k], t.data_ptr())
        self.bufs = OrderedDict()

    # What a launch pair allocates, one method per kind of buffer, so that a subclass (tests/_wsprobe.py) changes the buffers
    # without restating the launches.
    fwd_need_wgrad = 0             # TfnasCellDesc.need_wgrad of the forward

    def _gbuf(self, name, n, dtype=torch.float32):
        t = self.bufs[name] = (self._buf(n, self.guard, dtype), int(n))
        return t[0]

    def _partbuf(self, name, floats):
        from tfnas_amd.functions import _part
        return _part(floats, self.dev)

    def _gradbufs(self, accum_into):
        return [g.clone() for g in accum_into] if accum_into is not None else [torch.full_like(w, 3.5) for w in self.w]

    def _keeps_E(self):
        return bool(self.ws.E)

    def guards_ok(self):
        return {k: self.guard_ok(t, n) for k, (t, n) in self.bufs.items()}

    def forward(self):
        from tfnas_amd.functions import _stream
        d, ws, ptr = self.d, self.ws, self._lib.ptr
        d.need_wgrad = self.fwd_need_wgrad
        self.E = self._gbuf('E', ws.E) if self._keeps_E() else None
        self.D, self.Pr, self.fsmall = self._gbuf('D', ws.D), self._gbuf('Pr', ws.Pr), self._gbuf('fsmall', ws.fsmall)
        self.stats = self._gbuf('stats', ws.stats, torch.float64)
        self.out = self._gbuf('out', ws.out)
        part = self._partbuf('part_fwd', ws.part)
        try:
            self._lib.check(self.lib.tfnas_mixedop_fwd(C.byref(d), ptr(self.xh), ptr(self.wmix), ptr(self.E), ptr(self.D),
                                                       ptr(self.Pr), ptr(self.fsmall), ptr(self.stats), ptr(part), ptr(self.out),
                                                       _stream(self.dev)), 'tfnas_mixedop_fwd')
            torch.cuda.synchronize()
        finally:
            d.need_wgrad = 0
        return self.out[:ws.out].view(d.N, d.Ho, d.Wo, d.oc).permute(0, 3, 1, 2)

    def backward(self, r, need_wgrad=True, want_dx=True, accum_into=None):
        """(rc, dx or None, dwmix (None without mix weights), {name: gradient} or None); accum_into: gradients are ADDED to copies
        of these tensors"""
        from tfnas_amd.functions import _stream
        d, ws, ptr = self.d, self.ws, self._lib.ptr
        d.need_wgrad = int(need_wgrad)
        base = d.flags
        grads = None
        if need_wgrad:
            grads = self._gradbufs(accum_into)
            for (g, k), t in zip(self.slots, grads):
                setattr(d.g[g], self._lib._G_FIELDS[k], t.data_ptr())
            if accum_into is not None:
                d.flags = base | self._lib.CELL_ACCUM_WGRAD
        rh = r.permute(0, 2, 3, 1).contiguous().cuda()
        P = d.N * d.H * d.W
        light = not want_dx and not need_wgrad
        dx = self._gbuf('dx', P * d.ic) if want_dx else None
        dxp = self._gbuf('dxp', ws.dxp) if want_dx else None
        dZ, dEh = self._gbuf('dZ', 4 if light else ws.dZ), self._gbuf('dEh', 4 if light else ws.dEh)
        bsmall, red = self._gbuf('bsmall', ws.bsmall), self._gbuf('red', ws.red, torch.float64)
        dwmix = self._gbuf('dwmix', d.G) if self.wmix is not None else None
        part = self._partbuf('part_bwd', ws.part * 2)
        try:
            rc = self.lib.tfnas_mixedop_bwd(C.byref(d), ptr(self.xh), ptr(self.wmix), ptr(self.E), ptr(self.D), ptr(self.Pr),
                                            ptr(self.fsmall), ptr(self.stats), ptr(rh), ptr(dZ), ptr(dEh), ptr(bsmall), ptr(red),
                                            ptr(part), ptr(dx), ptr(dxp), ptr(dwmix), _stream(self.dev))
            torch.cuda.synchronize()
        finally:
            d.flags, d.need_wgrad = base, 0
            for g in range(d.G):
                for f in self._lib._G_FIELDS:
                    setattr(d.g[g], f, None)
        dxo = None if dx is None else dx[:P * d.ic].view(d.N, d.H, d.W, d.ic).permute(0, 3, 1, 2)
        return (rc, dxo, None if dwmix is None else dwmix[:d.G],
                None if grads is None else OrderedDict(zip(self.names, grads)))


# ------------------------------------------------------------------------------------------------ pin (float64)
# one 3-candidate cell per activation x stride and one 8-candidate swish cell, at 2 x 8 x 7 x 9 (out 8: residual at stride 1)
PIN_ACTS = ('relu', 'swish', 'relu6', 'h-swish')
PIN_CASES = [(tuple(THREE), act, s) for act in PIN_ACTS for s in (1, 2)] + [(tuple(EIGHT), 'swish', 1)]
PIN_T = 2.5


def pin_tag(case):
    return 'G%d_%s_s%d' % (len(case[0]), case[1], case[2])


def pin_case(case):
    """The restatement of one pin case (float64, train mode) with seeded weights, its input, cotangent, log_alphas and the seed
    the Gumbel noise is drawn under."""
    cands, act, s = case
    N, ic, oc, H, W = SMALL_SHAPE
    seed = 9000 + 97 * PIN_CASES.index(case)
    o = make_ref(cands, ic, oc, s, act, seed).double()
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(N, ic, H, W, generator=gen).double()
    r = torch.randn(N, oc, (H - 1) // s + 1, (W - 1) // s + 1, generator=gen).double()
    la = torch.log_softmax(0.5 * torch.randn(len(cands), generator=gen), -1).double()
    return o, x, r, la, seed + 3


def pin_collect(y, xs, la, ops):
    import numpy as np
    res = OrderedDict(out=y.detach().numpy(), dx=xs.grad.numpy(), dla=la.grad.numpy())
    for g, op in enumerate(ops):
        for k, p in op.named_parameters():
            res['g%d.%s' % (g, k)] = np.asarray(p.grad.numpy())
    return res


def pin_run(o, x, r, la, seed):
    """out, dx, d log_alphas and every parameter gradient of the soft forward out = sum_g w_g candidate_g(x),
    w = gumbel_softmax(log_alphas, T) with the noise torch draws under ``seed`` (the oracle's gumbel_softmax draws as torch's)."""
    for p in o.parameters():
        p.grad = None
    xs = x.clone().requires_grad_(True)
    lap = la.clone().requires_grad_(True)
    torch.manual_seed(seed)
    w = orc.gumbel_softmax(lap, PIN_T, None)
    y = o(xs, w)
    (y * r).sum().backward()
    return pin_collect(y, xs, lap, o.m_ops)


def pin_record(res):
    import _golden
    return OrderedDict((k, _golden.probe(torch.from_numpy(v))) for k, v in res.items())
