"""The workspace probe (tests/test_wsprobe_host.py, tests/test_gpu_ws_independence.py, tests/test_gpu_path_arena_independence.py):
a planned plain cell through tfnas_mixedop_fwd / _bwd on buffers the PROBE made -- every one between two guard bands of GUARD
elements, every interior filled with a seeded, finite poison before the launch -- with the descriptor exactly as the module route
makes it (MixedOP._plan -> CellPlan.desc / bind; need_wgrad, fwd_route, E == NULL as functions._cell_forward decides them).

No cell kernel uses floating-point atomics, so two launches with equal inputs agree in every bit whatever their workspaces held
before; a value that reaches a result from memory the call did not write shows as a bit difference between two poisons, a store
past a reported size as a touched guard word.  The poison is finite on purpose: masked or dropped reads of padding are legitimate.
Nothing here has a tolerance.  TFNAS_CELL_ACCUM_WGRAD is not probed: it reads its destinations by contract."""
import ctypes as C
from collections import OrderedDict

import torch

import _kinds
import _rawcell

GUARD = 4096                       # elements before and after every buffer, float32 and float64 alike
SENTINEL = _rawcell.RawCell.SENTINEL
SEED_A, SEED_B = 1, 2              # (poison() writes the seed's low four bits into every element: these two differ everywhere)
_INT = {torch.float32: torch.int32, torch.float64: torch.int64}
_PART_FILLS = {}                   # (seed, pieces) -> a poisoned `part` buffer on the device


def bits(t):
    """the integer view every comparison here is made through (so -0.0 != 0.0 and a NaN equals itself)"""
    return t.contiguous().view(_INT[t.dtype])


def poison(seed, n, dtype=torch.float32):
    """``n`` finite values of magnitude in [1, 1000] and random sign from a CPU generator seeded with ``seed``.  The low four
    mantissa bits of every element are the seed's low four bits: two seeds that differ there differ at EVERY element, not only
    almost surely (differs_everywhere asserts it for the pair in use)."""
    g = torch.Generator().manual_seed(int(seed))
    mag = 1.0 + 998.0 * torch.rand(int(n), generator=g, dtype=torch.float64)             # [1, 999): the tag cannot reach 1000
    sign = torch.randint(0, 2, (int(n),), generator=g, dtype=torch.int64) * 2 - 1
    v = (mag * sign).to(dtype)
    b = bits(v)
    b.bitwise_and_(~0xf).bitwise_or_(int(seed) & 0xf)
    return v


def differs_everywhere(a, b):
    return a.shape == b.shape and bool((bits(a) != bits(b)).all())


def check_seed_pair(a, b, n=1 << 16):
    """two seeds are a usable pair: their tags differ (so every element of every buffer does), shown on ``n`` elements of both types"""
    assert (int(a) ^ int(b)) & 0xf, (a, b)
    for dtype in _INT:
        assert differs_everywhere(poison(a, n, dtype), poison(b, n, dtype)), (a, b, dtype)


def diff_count(a, b):
    """number of elements of two results that differ in at least one bit"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((bits(a) != bits(b)).sum())


def compare(ra, rb):
    """{name: differing elements} of two result dictionaries, the names that differ only"""
    assert list(ra) == list(rb), (list(ra), list(rb))
    bad = OrderedDict()
    for k in ra:
        n = diff_count(ra[k], rb[k])
        if n:
            bad[k] = n
    return bad


class Slab:
    """``n`` elements between two bands of ``guard`` sentinel elements; ``view``: the interior, 256-byte aligned when
    ``align`` is set (the bands then grow by the elements the alignment skips)."""

    def __init__(self, n, dtype=torch.float32, device='cpu', guard=GUARD, align=False):
        self.n, self.guard = int(n), int(guard)
        self.raw = torch.empty(self.n + 2 * self.guard + (64 if align else 0), dtype=dtype, device=device)
        self.lo = self.guard
        if align:
            while (self.raw.data_ptr() + self.lo * self.raw.element_size()) % 256:
                self.lo += 1
        self.raw.fill_(SENTINEL)
        self.view = self.raw[self.lo:self.lo + self.n]
        self._want = int(bits(torch.tensor([SENTINEL], dtype=dtype))[0])

    def fill(self, seed):
        p = poison(seed, self.n, self.raw.dtype)
        self.view.copy_(p)
        return p

    def touched(self):
        """[(band, index in the band)] of the guard words that no longer hold the sentinel, through the integer view"""
        b = bits(self.raw)
        out = []
        for band, w in (('before', b[:self.lo]), ('after', b[self.lo + self.n:])):
            out += [(band, int(i)) for i in (w != self._want).nonzero().flatten()[:8]]
        return out


def part_sizes():
    l = _rawcell._lib().lib()
    return int(l.tfnas_sizeof(7)), int(l.tfnas_sizeof(8))


def part_fill(view, seed, piece, slots):
    """poison a `part` buffer of whole pieces and zero the reserved words at the end of each piece, as the header requires"""
    assert view.numel() % piece == 0 and 0 < slots < piece
    view.copy_(poison(seed, view.numel(), view.dtype))
    view.view(-1, piece)[:, piece - slots:].zero_()
    return view


def part_reserved_zero(view, piece, slots):
    return not bool(bits(view.view(-1, piece)[:, piece - slots:]).any())


# (soft / sampled, need_wgrad, dx wanted) of the five launch modes
MODES = OrderedDict([
    ('soft_frozen', (None, False, True)),
    ('soft_frozen_nodx', (None, False, False)),
    ('soft_wgrad', (None, True, True)),
    ('sampled0_wgrad', (0, True, True)),
    ('sampled5_wgrad', (5, True, True)),
    ('sampled0_frozen', (0, False, True)),
])


class WsProbe(_kinds.RawMixed):
    """The launch pair of candidates ``idxs`` of the product MixedOP ``m`` (on cuda, its route word in its HipModes) on probe
    buffers.  ``efree``: None -- E == NULL exactly where functions._cell_forward would pass it --, True -- E == NULL (the
    recompute form where the policy keeps the buffer; tfnas_efree_supported must say 1)."""

    def __init__(self, m, idxs, x, r, wmix, need_wgrad, want_dx=True, efree=None):
        from tfnas_amd import functions as F
        lb = self._lib = _rawcell._lib()
        self.lib, self.guard, self.dev = lb.lib(), GUARD, torch.device('cuda')
        self.need_wgrad, self.want_dx, self.fwd_need_wgrad = bool(need_wgrad), bool(want_dx), int(need_wgrad)
        N, _, H, W = x.shape
        self.xh = x.permute(0, 2, 3, 1).contiguous().cuda()
        self.r = r
        self.wmix = None if wmix is None else wmix.float().contiguous().cuda()
        plan = self.plan = m._plan(tuple(idxs))
        d, self.ws = plan.desc(N, H, W)
        self.w = [p.detach() for p in plan.params()]
        plan.bind(d, self.w)
        self.d = type(d)()                                       # a private copy: the module route launches on the cached one
        C.memmove(C.byref(self.d), C.byref(d), C.sizeof(d))
        d = self.d
        d.need_wgrad = int(need_wgrad)                           # (as functions._cell_forward: route and E-free ask with it set)
        self.fwd_route = int(self.lib.tfnas_cell_route(C.byref(d)))
        self.efree_supported = int(self.lib.tfnas_efree_supported(C.byref(d)))
        policy = (F.EFREE and ((plan.stride == 2 and plan.ic <= 24) or F.EFREE_STRIDE1) and not need_wgrad
                  and bool(self.efree_supported))
        self.efree = policy if efree is None else bool(efree)
        d.need_wgrad = 0
        self.names = ['g%d.%s' % (g, n) for g, b in enumerate(plan.blocks)
                      for n in _rawcell.param_names(lb.MBCONV, b.se_channels)]
        self.slots = [(g, lb._G_FIELDS.index(f)) for g, f in plan._g_slots]
        assert len(self.names) == len(self.w) == len(self.slots)
        self.piece, self.part_slots = part_sizes()
        self.bufs, self.seed = OrderedDict(), None

    # ---- buffers: RawMixed's launches, the probe's memory
    def _gbuf(self, name, n, dtype=torch.float32):
        s = self.bufs[name] = Slab(n, dtype, self.dev)
        s.fill(self.seed)
        return s.view

    def _partbuf(self, name, floats):
        pieces = 2 if (name == 'part_bwd' and self.need_wgrad) else 1        # (doubled when need_wgrad is set, as the module's)
        s = self.bufs[name] = Slab(pieces * self.piece, torch.float32, self.dev)
        key = (self.seed, pieces)
        if key not in _PART_FILLS:                               # (16 MiB a piece: drawn once per seed and size, kept on the device)
            _PART_FILLS[key] = part_fill(torch.empty(pieces * self.piece), self.seed, self.piece, self.part_slots).to(self.dev)
        s.view.copy_(_PART_FILLS[key])
        return s.view

    def _gradbufs(self, accum_into):
        assert accum_into is None
        return [self._gbuf('grad.' + n, w.numel()).view(w.shape) for n, w in zip(self.names, self.w)]

    def _keeps_E(self):
        return bool(self.ws.E) and not self.efree

    def guards_ok(self):
        """{buffer: touched guard words}, the touched buffers only"""
        hit = ((k, s.touched()) for k, s in self.bufs.items())
        return {k: t for k, t in hit if t}

    def _columns(self, t, pixels):
        """the valid columns [g.off, g.off + g.mc) of every group of a [pixels][M] tensor"""
        d = self.d
        t = t[:pixels * d.M].view(pixels, d.M)
        return torch.cat([t[:, d.g[g].off:d.g[g].off + d.g[g].mc] for g in range(d.G)], 1).clone()

    def run(self, seed, tamper=None):
        """forward, synchronise, guards, [tamper(self)], backward, synchronise, guards -> {name: result}"""
        d, ws = self.d, self.ws
        self.seed, self.bufs = seed, OrderedDict()
        out = self.forward()
        bad = self.guards_ok()
        assert not bad, ('forward', bad)
        res = OrderedDict(out=out.clone(), Pr=self.Pr.clone(), D=self._columns(self.D, d.N * d.Ho * d.Wo))
        if self.E is not None and not (self.fwd_route & self._lib.ROUTE_TAKEN_FX):
            res['E'] = self._columns(self.E, d.N * d.H * d.W)
        if tamper is not None:
            tamper(self)
        d.fwd_route = self.fwd_route
        try:
            rc, dx, dwmix, grads = self.backward(self.r, self.need_wgrad, self.want_dx)
        finally:
            d.fwd_route = 0
        assert rc == 0, rc
        bad = self.guards_ok()
        assert not bad, ('backward', bad)
        if dx is not None:
            res['dx'] = dx.clone()
        if dwmix is not None:
            res['dwmix'] = dwmix.clone()
        for k, g in (grads or {}).items():
            res[k] = g.clone()
        return res


def module_run(m, idxs, x, r, wmix, need_wgrad, want_dx=True):
    """The same launch pair through MixedOpFn.apply, the route tests/test_gpu_cell.py holds to the oracle: WsProbe.run's names for
    out, D, dx, dwmix and the weight gradients, and whether the launch kept an E buffer."""
    from tfnas_amd.functions import MixedOpFn
    plan = m._plan(tuple(idxs))
    params = plan.params()
    for p in params:
        p.requires_grad_(bool(need_wgrad))
        p.grad = None
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(bool(want_dx))
    wm = None if wmix is None else wmix.float().cuda().requires_grad_(True)
    MixedOpFn.fwd_sink = sink = []
    try:
        y = MixedOpFn.apply(plan, xm, wm, *params)
    finally:
        MixedOpFn.fwd_sink = None
    (y * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    s = sink[0]
    d = s['d']
    Po = d.N * d.Ho * d.Wo
    D = s['D'][:Po * d.M].view(Po, d.M)
    res = OrderedDict(out=y.detach().clone(), D=torch.cat([D[:, d.g[g].off:d.g[g].off + d.g[g].mc] for g in range(d.G)], 1))
    if want_dx:
        res['dx'] = xm.grad.clone()
    if wm is not None:
        res['dwmix'] = wm.grad.clone()
    if need_wgrad:
        names = ['g%d.%s' % (g, n) for g, b in enumerate(plan.blocks)
                 for n in _rawcell.param_names(_rawcell._lib().MBCONV, b.se_channels)]
        for n, p in zip(names, params):
            res[n] = p.grad.clone()
    for p in params:
        p.grad = None
    return res, s['E'] is not None
