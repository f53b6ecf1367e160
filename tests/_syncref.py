"""The two-rank model of the sync-stats tests (tests/test_gpu_sync_cells.py on the GPU, tests/test_sync_refs.py on the CPU).

Two shards ``x_a``, ``x_b`` of ``n`` images each, ONE cell with one set of weights, upstream gradients ``r_a``, ``r_b``.  The
reference is the float64 copy of the existing restatement (_kinds.MixedRef / _skip.SkipRef over the oracle's MBConv and
_fused.FusedRef; a plain cell is a MixedRef of plain candidates) run ONCE on cat([x_a, x_b]) with cat([r_a, r_b]): ordinary
BatchNorm over 2n images and plain autograd.  A rank of a data-parallel run with global-batch statistics must produce its half
of that run's y and dx, and the two ranks' weight gradients and d wmix must add up to that run's.

The hook (include/tfnas_hip.h: TfnasCellDesc.sync_fn) is modelled in one process, without a process group:
  record   leaves every table alone and copies it out (world 1);
  serve    copies the local table out, then overwrites it with total_k / 2, total_k being the table the record run of the joint
           batch produced at call k -- with equal shards exactly all-reduce(SUM) followed by / world;
  skip(k)  as serve, but call k leaves its table alone: a library that forgot that site.
Every hook notes (table pointer, doubles, stream) per call, catches every exception and returns a non-zero code instead.

``x_b`` carries a per-channel offset and scale, so shard and joint statistics differ in every channel (a missed site cannot
hide), and the seeds of the kinked-activation cases keep every float64 pre-activation of the JOINT run (the one all three launches
share: they normalise alike) KINK_TAU from every kink, so no element is ever exempted from a comparison."""
import copy
import ctypes as C
from collections import OrderedDict

import torch

import _fused
import _kinds
import _rawcell
import _sestyle
import _skip

N_RANK = 2                                  # images per rank
ATOL, RTOL = 2e-5, 1e-4                     # the float64 gate of tests/test_gpu_affine_f64.py: 2e-5 + 1e-4 max|ref| per tensor
ADD_RTOL = 1e-4                             # additivity of the backward tables: 1e-4 max|total_k| over the owned columns
FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
S = _skip.S


def gate(refmax):
    return ATOL + RTOL * float(refmax)


def ratio(got, ref):
    """max |got - ref| / gate(max |ref|); 1.0 is the gate"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0
    d = float((got - ref).abs().max())
    return (d if d == d else float('inf')) / gate(ref.abs().max())


# ------------------------------------------------------------------------------------------------ cases
def plain8(mids, se=(8, 16)):
    """eight plain candidates: kernel sizes 3 / 5, SE off and on, the given (ragged) mid widths"""
    ks = ((3, 0), (5, 0), (3, se[0]), (5, se[1]), (3, 0), (5, 0), (3, se[0]), (5, se[1]))
    return [('M', m, k, s) for m, (k, s) in zip(mids, ks)]


RAGGED = [53, 107, 44, 88, 61, 96, 48, 79]                # the mid widths of test_gpu_cell.py's tiny_ragged_res
LATE = [77, 131, 68, 112, 85, 120, 72, 103]               # (a plain candidate is wider than its 64 input channels)
SMALL = _kinds.SMALL_SHAPE[1:]                             # ic 8, oc 8, 7 x 9
K7 = [('M', 24, 7, 0)]
M1, N1, F1 = [_skip.M], [_skip.N], [_skip.F]
RELU2 = [('M', 22, 3, 0), ('M', 24, 5, 8)]
SE3 = [('M', 22, 3, 8), ('N', 3, 8), ('F', 22, 8)]          # every kind with squeeze-excite


class Case:
    """name, candidates, (ic, oc, H, W, stride), activation, route bits (TFNAS_ROUTE_*), first seed tried, squeeze-excite style
    (se_act, se_gate) or None"""

    def __init__(self, name, cands, geom, act='swish', route=0, base=700, style=None):
        self.name, self.cands, self.geom, self.act, self.route, self.base = name, list(cands), tuple(geom), act, route, base
        self.style = style

    @property
    def key(self):
        """cases that differ in their route bits alone share data and reference"""
        return (tuple(self.cands), self.geom, self.act, self.base, self.style)


def _cases():
    FOLD_OFF, TILED = 0x2, 3 << 6                         # _lib.ROUTE_FOLD_OFF, _lib.ROUTE_DW['tiled'] (test_sync_refs checks)
    cs = [Case('plain_res_9x11', plain8(RAGGED), (24, 24, 9, 11, 1)),
          Case('plain_s2_regwin', plain8(RAGGED), (16, 24, 12, 10, 2)),
          Case('plain_ring_14x14', plain8(RAGGED), (24, 24, 14, 14, 1)),
          Case('plain_ring_14x14_tiled', plain8(RAGGED), (24, 24, 14, 14, 1), route=TILED),
          Case('plain_late_7x7', plain8(LATE), (64, 64, 7, 7, 1)),
          Case('plain_res_9x11_foldoff', plain8(RAGGED), (24, 24, 9, 11, 1), route=FOLD_OFF),
          Case('k7', K7, SMALL + (1,))]
    for s in (1, 2):
        oc = 8 if s == 1 else 12
        for tag, cands in (('M', M1), ('N', N1), ('F', F1), ('three', _kinds.THREE), ('eight', _kinds.EIGHT)):
            cs.append(Case('%s_s%d' % (tag, s), cands, (8, oc, 7, 9, s)))
    cs += [Case('three_s1_foldoff', _kinds.THREE, (8, 8, 7, 9, 1), route=FOLD_OFF),
           Case('mnfs', _skip.MNFS, SMALL + (1,)),
           Case('eight_s', _skip.EIGHT_S, SMALL + (1,)),
           Case('se_relu_hsigmoid', SE3, SMALL + (1,), style=_sestyle.MNV3),
           Case('relu_plain', RELU2, SMALL + (1,), 'relu'),
           Case('relu6_three', _kinds.THREE, SMALL + (1,), 'relu6'),
           Case('hswish_mnfs_s1', _skip.MNFS, SMALL + (1,), 'h-swish')]
    return OrderedDict((c.name, c) for c in cs)


CASES = _cases()
KINKED = [n for n, c in CASES.items() if c.act != 'swish' or c.style is not None]


class Data:
    pass


def kink_distance(case, o, x):
    """_kinds.kink_distance; with a squeeze-excite style _sestyle's, which adds the kinks of the hidden activation and the gate"""
    return _sestyle.kink_distance(o, x) if case.style is not None else _kinds.kink_distance(o, x)


def branches_ok(case, o, x):
    """a hard-sigmoid gate: pre-activations below -3, inside (-3, 3) and above 3 all occur"""
    if case.style is None or case.style[1] != 'h-sigmoid':
        return True
    return min(_sestyle.gate_branches(o, x)) > 0


_DATA = {}


def case_data(case):
    """restatement (float32), x = cat([x_a, x_b]), r = cat([r_a, r_b]), mix weights; computed once per case.key"""
    if case.key in _DATA:
        return _DATA[case.key]
    ic, oc, H, W, stride = case.geom
    n = N_RANK
    for seed in range(case.base, case.base + 400):
        if case.style is not None:
            o = _sestyle.make_ref(case.cands, ic, oc, stride, case.act, case.style[0], case.style[1], seed)
        else:
            o = _skip.make_ref(case.cands, ic, oc, stride, case.act, seed)
        gen = torch.Generator().manual_seed(seed + 2)
        xa = torch.randn(n, ic, H, W, generator=gen)
        xb = torch.randn(n, ic, H, W, generator=gen)
        # shard b: its own per-channel scale (0.5 .. 1.5) and offset (+-0.4 .. +-1.2)
        scale = 0.5 + torch.rand(ic, generator=gen)
        sign = torch.where(torch.rand(ic, generator=gen) < 0.5, -1.0, 1.0)
        off = sign * (0.4 + 0.8 * torch.rand(ic, generator=gen))
        xb = xb * scale.view(1, -1, 1, 1) + off.view(1, -1, 1, 1)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        r = torch.randn(2 * n, oc, Ho, Wo, generator=gen)
        r[n:] *= 1.5
        w = torch.softmax(torch.randn(len(case.cands), generator=gen), -1)
        x = torch.cat([xa, xb])
        if kink_distance(case, o, x) >= _kinds.KINK_TAU and branches_ok(case, o, x):
            break
    else:
        raise AssertionError('no seed keeps the pre-activations clear of the kinks')
    dt = Data()
    dt.o, dt.x, dt.r, dt.w, dt.seed, dt.n = o, x, r, w, seed, n
    _DATA[case.key] = dt
    return dt


def _run(o, x, r, w, taps=None):
    """out, dx, d wmix and {name: gradient} of one forward + backward; taps: {} that receives the pre-BatchNorm convolution
    outputs 'g<g>.E' / '.D' / '.P' of every computing candidate"""
    if taps is None:
        return _kinds.ref_run(o, x, r, w)
    # the oracle's MBConv runs on functional convolutions and reports E / D / P in its detail dict; _fused.FusedRef calls its
    # convolution modules, which forward hooks tap
    handles, dets = [], {}
    for g, op in enumerate(o.m_ops):
        for tag, mod in (('D', getattr(op, 'fused_conv', None)), ('P', getattr(op, 'point_linear', None))):
            if isinstance(op, _fused.FusedRef):
                handles.append(mod.conv.register_forward_hook(
                    lambda _m, _i, out, key='g%d.%s' % (g, tag): taps.__setitem__(key, out.detach())))
    try:
        for p in o.parameters():
            p.grad = None
        xs, ws = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = o(xs, ws, dets)
        (y * r).sum().backward()
    finally:
        for h in handles:
            h.remove()
    for g, det in dets.items():
        for tag in ('E', 'D', 'P'):
            if tag in det:
                taps['g%d.%s' % (g, tag)] = det[tag].detach()
    grads = OrderedDict()
    for g, op in enumerate(o.m_ops):
        for k, p in op.named_parameters():
            grads['g%d.%s' % (g, k)] = p.grad.clone()
    return y.detach(), xs.grad, ws.grad, grads


class Ref:
    pass


_REFS = {}


def reference(case):
    """the float64 restatement on the joint batch: y, dx, dwmix, grads; per-shard (sum, sum of squares) of every pre-BatchNorm
    convolution output (``shard[rank]['g<g>.E' | '.D' | '.P']``: [channels, 2]); computed once per case.key, never changed"""
    if case.key in _REFS:
        return _REFS[case.key]
    dt = case_data(case)
    o64 = copy.deepcopy(dt.o).double()
    taps = {}
    y, dx, dw, grads = _run(o64, dt.x.double(), dt.r.double(), dt.w.double(), taps)
    ref = Ref()
    ref.y, ref.dx, ref.dwmix, ref.grads = y, dx, dw, grads
    ref.shard = []
    for half in (slice(0, dt.n), slice(dt.n, 2 * dt.n)):
        ref.shard.append({k: torch.stack([t[half].sum((0, 2, 3)), (t[half] ** 2).sum((0, 2, 3))], 1) for k, t in taps.items()})
    _REFS[case.key] = ref
    return ref


def f32_joint(case):
    """the float32 restatement on the joint batch (tests/test_sync_refs.py: within a quarter of the gate of the float64 one)"""
    dt = case_data(case)
    return _kinds.ref_run(dt.o, dt.x, dt.r, dt.w)


def local_stats_first_half(case):
    """y of shard a normalised with ITS OWN statistics (float64): what a rank computes when no site is synced"""
    dt = case_data(case)
    o64 = copy.deepcopy(dt.o).double()
    with torch.no_grad():
        return o64(dt.x[:dt.n].double(), dt.w.double())


# ------------------------------------------------------------------------------------------------ what a descriptor implies
def groups_of(cands):
    """(number of computing groups, whether any of them is plain)"""
    comp = _skip.computing(cands)
    return len(comp), any(c[0] == 'M' for c in comp)


def expected_calls(G, has_plain, M, oc, ws, want_dx=True, need_wgrad=True):
    """[(buffer, offset in doubles, doubles)] of one forward + backward under a hook; ``ws``: anything with TfnasCellWs's
    off_stats1..3 / off_red1..3.  Non-plain kinds have no BatchNorm site 0: no stats1 and no red1 call."""
    fwd = ([('stats', int(ws.off_stats1), 2 * M)] if has_plain else []) + [('stats', int(ws.off_stats2), 2 * M),
                                                                              ('stats', int(ws.off_stats3), 2 * G * oc)]
    bwd = [('red', int(ws.off_red3), 2 * G * oc)]
    if want_dx or need_wgrad:                             # (d wmix alone: the backward returns after the BN3 sums)
        bwd.append(('red', int(ws.off_red2), 2 * M))
        if has_plain:
            bwd.append(('red', int(ws.off_red1), 2 * M))
    return fwd, bwd


def owned_columns(d, cands, table):
    """bool [rows] of a (sum, sumsq)-pair table: the rows some group owns.  'stats1' / 'red1' belong to the plain groups alone
    (csrc/kernels.h: they may hold anything elsewhere); 'stats2' / 'red2' to every computing group's [off, off + mc)."""
    comp = _skip.computing(cands)
    if table in ('stats3', 'red3'):
        return torch.ones(len(comp) * d.oc, dtype=torch.bool)
    m = torch.zeros(d.M, dtype=torch.bool)
    for g, c in enumerate(comp):
        if table in ('stats1', 'red1') and c[0] != 'M':
            continue
        m[d.g[g].off:d.g[g].off + d.g[g].mc] = True
    return m


# ------------------------------------------------------------------------------------------------ the hook
class _RawView:
    """zero-copy view of device memory the library owns (as tfnas_amd.syncbn._Raw)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {'shape': (int(n),), 'typestr': '<f8', 'data': (int(ptr), False), 'version': 2}


class Hook:
    """mode 'record' | 'serve'; totals: the joint record run's tables (serve); skip: a call index whose table stays local;
    fail_at: that call returns ``code`` without touching anything.  ``calls``: (pointer, doubles, stream) per call; ``tables``:
    the local tables as the library handed them over."""

    def __init__(self, mode='record', totals=None, skip=None, fail_at=None, code=-1000):
        assert mode in ('record', 'serve') and (mode == 'record' or totals is not None)
        self.mode, self.totals, self.skip, self.fail_at, self.code = mode, totals, skip, fail_at, code
        self.world = 1 if mode == 'record' else 2
        self.calls, self.tables, self.error = [], [], None
        self.cb = FN(self._call)
        self.fn = C.cast(self.cb, C.c_void_p).value

    def _call(self, _user, table, n, stream):
        try:
            k = len(self.calls)
            self.calls.append((int(table), int(n), int(stream or 0)))
            if self.fail_at is not None and k == self.fail_at:
                return self.code
            dev = torch.device('cuda', torch.cuda.current_device())
            ext = torch.cuda.ExternalStream(int(stream), device=dev) if stream else torch.cuda.default_stream(dev)
            with torch.cuda.stream(ext):
                t = torch.as_tensor(_RawView(table, n), device=dev)
                self.tables.append(t.clone())
                if self.mode == 'serve' and k != self.skip:
                    tot = self.totals[k]
                    assert tot.numel() == int(n), (k, tot.numel(), int(n))
                    t.copy_(tot * 0.5)
            return 0
        except Exception as e:                            # (nothing may unwind through the C frames)
            self.error = e
            return -1001


# ------------------------------------------------------------------------------------------------ the launcher
class SyncCell(_skip.RawSkip):
    """_kinds.RawMixed / _skip.RawSkip whose descriptor carries ``hook`` (set BEFORE tfnas_cell_plan / tfnas_cell_ws: with a
    hook the cell needs its E buffer) and ``route``"""

    def __init__(self, o, x, w, hook, route=0, style=None, guard=64):
        lb = self._lib = _rawcell._lib()
        self.lib, self.o, self.guard, self.hook = lb.lib(), o, guard, hook
        self.dev = torch.device('cuda')
        N, _, H, W = x.shape
        self.xh = x.permute(0, 2, 3, 1).contiguous().cuda()
        self.wmix = w.float().contiguous().cuda()
        self.d = cell_desc(o.cands, N, H, W, o.in_channels, o.out_channels, o.stride, o.act_func, hook, route, style)
        lb.check(self.lib.tfnas_cell_plan(C.byref(self.d)), 'tfnas_cell_plan')
        self.ws = _rawcell.ws_of(self.lib, self.d)
        self.names, self.w, self.slots = [], [], []
        for g, (c, op) in enumerate(zip(o.cands, o.m_ops)):
            if _skip.is_skip(c):
                continue
            kind = _kinds.kind_of(c)
            sd = dict(op.named_parameters())
            for k, nme in zip(kind.bound(op.se_channels > 0), _rawcell.param_names(kind, op.se_channels)):
                t = sd[nme].detach().float().contiguous().cuda()
                self.names.append('g%d.%s' % (g, nme))
                self.w.append(t)
                self.slots.append((g, k))
                setattr(self.d.g[g], lb._W_FIELDS[k], t.data_ptr())
        self.bufs = OrderedDict()

    def launch(self, r, need_wgrad=True, want_dx=True):
        """one forward + backward on a stream of its own; returns a Run"""
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        run = Run()
        with torch.cuda.stream(side):
            run.stream = int(side.cuda_stream)
            run.out = self.forward()
            run.n_fwd = len(self.hook.calls) if self.hook is not None else 0
            run.rc, run.dx, run.dwmix, run.grads = self.backward(r, need_wgrad=need_wgrad, want_dx=want_dx)
            torch.cuda.synchronize()
        run.stats_ptr, run.red_ptr = self.stats.data_ptr(), self.bufs['red'][0].data_ptr()
        run.guards = self.guards_ok()
        return run


class Run:
    pass


def cell_desc(cands, N, H, W, ic, oc, stride, act, hook=None, route=0, style=None):
    """the unplanned descriptor of ``cands`` (TFNAS_CELL_KINDS, + TFNAS_CELL_SKIP with a skip candidate) with hook and route"""
    lb = _rawcell._lib()
    if any(_skip.is_skip(c) for c in cands):
        d = _skip.skip_desc(cands, N, H, W, ic, oc, stride, lb.act_id(act))
    else:
        d = _kinds.mixed_desc(cands, N, H, W, ic, oc, stride, lb.act_id(act))
    d.route = route
    if style is not None:
        d.se_style = lb.se_style_id(*style)
        d.flags |= lb.se_style_flags(d.se_style)
    if hook is not None:
        d.sync_fn, d.sync_user, d.sync_world = hook.fn, None, hook.world
    return d


# ------------------------------------------------------------------------------------------------ the head
HEAD_GEOM = (24, 32, 7, 7)                  # ic, mc (a multiple of 4: a ragged head is refused by the plan), H, W


def head_data(seed=740):
    """the search-form head (1x1 convolution + BatchNorm on batch statistics + swish + global average pool) as the oracle's
    _ConvBN, the joint input of two shards (shard b with its own per-channel scale and offset) and d pooled [2n, mc]"""
    import tfnas_oracle as orc
    if 'head' in _DATA:
        return _DATA['head']
    ic, mc, H, W = HEAD_GEOM
    n = N_RANK
    torch.manual_seed(seed)
    cb = orc._ConvBN(ic, mc, 1, 1, 'swish')
    gen = torch.Generator().manual_seed(seed + 2)
    xa, xb = torch.randn(n, ic, H, W, generator=gen), torch.randn(n, ic, H, W, generator=gen)
    scale = 0.5 + torch.rand(ic, generator=gen)
    sign = torch.where(torch.rand(ic, generator=gen) < 0.5, -1.0, 1.0)
    xb = xb * scale.view(1, -1, 1, 1) + (sign * (0.4 + 0.8 * torch.rand(ic, generator=gen))).view(1, -1, 1, 1)
    r = torch.randn(2 * n, mc, generator=gen)
    r[n:] *= 1.5
    dt = Data()
    dt.o, dt.x, dt.r, dt.n = cb, torch.cat([xa, xb]), r, n
    _DATA['head'] = dt
    return dt


def head_run(cb, x, r):
    """pooled, dx and the convolution's weight gradient of the search-form head (tests/_affineref.head_forward)"""
    import _affineref as ar
    cb.conv.weight.grad = None
    xs = x.clone().requires_grad_(True)
    pooled = ar.head_forward(cb.train(), xs, affine=False)
    (pooled * r).sum().backward()
    return OrderedDict([('pooled', pooled.detach()), ('dx', xs.grad), ('g.conv.weight', cb.conv.weight.grad.clone())])


def head_reference():
    """float64, joint batch; ``shard``: per-rank (sum, sum of squares) [mc, 2] of the convolution's output"""
    if 'head' in _REFS:
        return _REFS['head']
    dt = head_data()
    cb = copy.deepcopy(dt.o).double()
    ref = Ref()
    ref.res = head_run(cb, dt.x.double(), dt.r.double())
    with torch.no_grad():
        e = cb.conv(dt.x.double())
    ref.shard = [torch.stack([e[h].sum((0, 2, 3)), (e[h] ** 2).sum((0, 2, 3))], 1) for h in (slice(0, dt.n), slice(dt.n, 2 * dt.n))]
    _REFS['head'] = ref
    return ref


def head_desc(N, hook=None):
    lb = _rawcell._lib()
    ic, mc, H, W = HEAD_GEOM
    d = lb.TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, H, W, ic, 4, 1, lb.act_id('swish'), 1, lb.MODE_HEAD
    d.has_res, d.eps = 0, lb.BN_EPS
    d.g[0].mc, d.g[0].k, d.g[0].se = mc, 3, 0
    if hook is not None:
        d.sync_fn, d.sync_user, d.sync_world = hook.fn, None, hook.world
    return d


class SyncHead:
    """tfnas_head_fwd / tfnas_head_bwd with caller-made, guard-banded buffers (as tests/test_gpu_affine_f64.RawHead's search form)
    under ``hook``"""
    SENTINEL, GUARD = -777.25, 64

    def __init__(self, cb, x, hook):
        from tfnas_amd import functions as F
        lb = self._lib = _rawcell._lib()
        self.lib, self.F, self.hook, self.dev = lb.lib(), F, hook, torch.device('cuda')
        self.mc = HEAD_GEOM[1]
        self.d = head_desc(x.shape[0], hook)
        lb.check(self.lib.tfnas_cell_plan(C.byref(self.d)), 'tfnas_cell_plan')
        self.ws = _rawcell.ws_of(self.lib, self.d)
        self.xh = x.permute(0, 2, 3, 1).contiguous().cuda()
        self.w = cb.conv.weight.detach().float().contiguous().cuda()
        self.d.g[0].w_expand = self.w.data_ptr()

    def _buf(self, n, guard=0, dtype=torch.float32):
        t = torch.empty(int(n) + guard, device=self.dev, dtype=dtype)
        if guard:
            t[int(n):] = self.SENTINEL
        return t

    def launch(self, r):
        """forward + backward (need_wgrad = 1) on a stream of its own; returns a Run (res: pooled, dx, g.conv.weight)"""
        d, ws, ptr, G = self.d, self.ws, self._lib.ptr, self.GUARD
        N, mc, P = d.N, self.mc, d.N * d.H * d.W
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        run = Run()
        with torch.cuda.stream(side):
            st = self.F._stream(self.dev)
            run.stream = int(side.cuda_stream)
            E = self._buf(ws.E)
            stats, pooled = self._buf(2 * d.M, G, torch.float64), self._buf(N * mc, G)
            d.need_wgrad = 0
            rc = self.lib.tfnas_head_fwd(C.byref(d), ptr(self.xh), ptr(E), ptr(stats), ptr(self.F._part(ws.part, self.dev)),
                                         ptr(pooled), st)
            run.n_fwd = len(self.hook.calls)
            gw = torch.full_like(self.w, 3.5)
            dp = r.float().contiguous().cuda()
            dEh, cb1 = self._buf(ws.dEh), self._buf(4 * d.M)
            red, dx, dxp = self._buf(2 * d.M, G, torch.float64), self._buf(P * d.ic, G), self._buf(ws.dxp)
            if rc == 0:
                d.g[0].g_expand, d.need_wgrad = gw.data_ptr(), 1
                try:
                    rc = self.lib.tfnas_head_bwd(C.byref(d), ptr(self.xh), ptr(E), ptr(stats), ptr(dp), ptr(dEh), ptr(cb1),
                                                 ptr(red), ptr(self.F._part(ws.part, self.dev)), ptr(dx), ptr(dxp), st)
                finally:
                    d.g[0].g_expand, d.need_wgrad = None, 0
            torch.cuda.synchronize()
        run.rc, run.stats_ptr, run.red_ptr = rc, stats.data_ptr(), red.data_ptr()
        run.guards = {k: bool((t[int(m):] == self.SENTINEL).all())
                      for k, (t, m) in dict(stats=(stats, 2 * d.M), pooled=(pooled, N * mc), red=(red, 2 * d.M), dx=(dx, P * d.ic)).items()}
        run.res = OrderedDict([('pooled', pooled[:N * mc].view(N, mc)),
                               ('dx', dx[:P * d.ic].view(d.N, d.H, d.W, d.ic).permute(0, 3, 1, 2)), ('g.conv.weight', gw)])
        return run
