"""The raw-ABI side of the one-block cell tests (tests/_noexp.py, tests/_fused.py and their suites): descriptors of any block kind
built on ``_lib.describe_block`` -- with overrides, so the refusal tests can still build wrong ones -- their workspaces, and one
launcher for what the Python modules do not expose (route word, GEMM mode, accumulation, guard bands, dx == NULL,
need_wgrad = 0).  Also the activation kinks every suite keeps its seeds clear of."""
import ctypes as C
from collections import OrderedDict

import torch

KINKS = {'relu': (0.0,), 'swish': (), 'relu6': (0.0, 6.0), 'h-swish': (-3.0, 3.0)}
KINK_TAU = 1e-4

_LEAD = {'MBCONV': ('inverted_bottleneck', 'depth_conv'), 'NOEXPAND': ('depth_conv',), 'FUSED': ('fused_conv',)}


def param_names(kind, se):
    """Parameter names of a block of ``kind`` (the modules', the oracle's and the restatement's alike) in hip_params() order."""
    names = [n + '.conv.weight' for n in _LEAD[kind.name] + ('point_linear',)]
    if se:
        names += ['squeeze_excite.conv_%s.%s' % (c, t) for c in ('reduce', 'expand') for t in ('weight', 'bias')]
    return names


def cell_desc(kind, N, H, W, ic, oc, mc, k=3, stride=1, act=0, se=0, flags=None, G=1, mode=0, need_wgrad=0):
    """A descriptor of one block of ``kind``; flags = None: the kind's bit plus whatever k / act need.  ``flags``, ``mode`` and
    ``G`` (every group a copy of the first) override what a well-formed one-block cell would say."""
    d = _lib().describe_block(kind, N, H, W, ic, mc, se, oc, k, stride, act)
    d.G, d.mode, d.need_wgrad = G, mode, need_wgrad
    d.has_res = int(mode == 0 and ic == oc and stride == 1)
    for g in range(1, G):
        d.g[g].mc, d.g[g].k, d.g[g].se = mc, k, se
    if flags is not None:
        d.flags = flags
    return d


def _lib():
    from tfnas_amd import _lib
    return _lib


def ws_of(lib, d):
    ws = _lib().TfnasCellWs()
    assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == 0
    return ws


class RawCell:
    """One search-form block of ``kind`` through tfnas_mixedop_fwd / _bwd with caller-made buffers: ``guard`` sentinel floats
    follow D and dx (``D``, ``out``, ``dx_raw``: the raw buffers); the route word, TFNAS_CELL_ACCUM_WGRAD, need_wgrad and
    dx == NULL are the caller's choice.  Weights: the parameters ``names`` of the CPU block ``o`` (param_names order)."""
    SENTINEL = -777.25

    def __init__(self, o, x, kind, names, guard=64, gemm=None):
        lb = self._lib = _lib()
        self.lib, self.o, self.kind, self.guard, self.names = lb.lib(), o, kind, guard, list(names)
        self.dev = torch.device('cuda')
        N, _, H, W = x.shape
        self.xh = x.permute(0, 2, 3, 1).contiguous().cuda()
        self.d = cell_desc(kind, N, H, W, o.in_channels, o.out_channels, o.mid_channels, o.kernel_size, o.stride,
                           lb.act_id(o.act_func), o.se_channels)
        if gemm is not None:
            self.d.gemm_mode = lb.GEMM_EXPLICIT | lb.GEMM_MODES[gemm]
        lb.check(self.lib.tfnas_cell_plan(C.byref(self.d)), 'tfnas_cell_plan')
        self.ws = ws_of(self.lib, self.d)
        sd = dict(o.named_parameters())
        self.w = [sd[n].detach().float().contiguous().cuda() for n in self.names]
        self.fields = kind.bound(o.se_channels > 0)
        assert len(self.fields) == len(self.w)
        for k, t in zip(self.fields, self.w):
            setattr(self.d.g[0], lb._W_FIELDS[k], t.data_ptr())

    def _buf(self, n, guard=0, dtype=torch.float32):
        t = torch.empty(int(n) + guard, device=self.dev, dtype=dtype)
        if guard:
            t[int(n):] = self.SENTINEL
        return t

    def forward(self, route=0):
        """out [N, oc, Ho, Wo] (a view of ``self.out``)"""
        from tfnas_amd.functions import _part, _stream
        d, ws, ptr = self.d, self.ws, self._lib.ptr
        d.route, d.need_wgrad = route, 0
        self.D = self._buf(ws.D, self.guard)
        self.Pr, self.fsmall = self._buf(ws.Pr), self._buf(ws.fsmall)
        self.stats = self._buf(ws.stats, dtype=torch.float64)
        self.out = self._buf(ws.out)
        part = _part(ws.part, self.dev)
        self._lib.check(self.lib.tfnas_mixedop_fwd(C.byref(d), ptr(self.xh), None, None, ptr(self.D), ptr(self.Pr),
                                                   ptr(self.fsmall), ptr(self.stats), ptr(part), ptr(self.out),
                                                   _stream(self.dev)), 'tfnas_mixedop_fwd')
        torch.cuda.synchronize()
        return self.out.view(d.N, d.Ho, d.Wo, d.oc).permute(0, 3, 1, 2)

    def backward(self, r, route=0, need_wgrad=True, want_dx=True, accum_into=None):
        """returns (rc, dx [N, ic, H, W] or None, {parameter name: gradient} or None); accum_into: the gradients are ADDED to
        copies of these tensors (same order as ``names``).  ``dx_raw``: the dx buffer with its guard band."""
        from tfnas_amd.functions import _part, _stream
        d, ws, ptr = self.d, self.ws, self._lib.ptr
        d.route, d.need_wgrad = route, int(need_wgrad)
        base = d.flags
        grads = None
        if need_wgrad:
            grads = [g.clone() for g in accum_into] if accum_into is not None else [torch.full_like(w, 3.5) for w in self.w]
            for k, t in zip(self.fields, grads):
                setattr(d.g[0], self._lib._G_FIELDS[k], t.data_ptr())
            if accum_into is not None:
                d.flags = base | self._lib.CELL_ACCUM_WGRAD
        rh = r.permute(0, 2, 3, 1).contiguous().cuda()
        P = d.N * d.H * d.W
        dx = self._buf(P * d.ic, self.guard) if want_dx else None
        dZ, dEh, bsmall = self._buf(ws.dZ), self._buf(ws.dEh), self._buf(ws.bsmall)
        red = self._buf(ws.red, dtype=torch.float64)
        part = _part(ws.part * 2, self.dev)
        try:
            rc = self.lib.tfnas_mixedop_bwd(C.byref(d), ptr(self.xh), None, None, ptr(self.D), ptr(self.Pr), ptr(self.fsmall),
                                            ptr(self.stats), ptr(rh), ptr(dZ), ptr(dEh), ptr(bsmall), ptr(red), ptr(part),
                                            ptr(dx), None, None, _stream(self.dev))
            torch.cuda.synchronize()
        finally:
            d.flags, d.need_wgrad = base, 0
            for f in self._lib._G_FIELDS:
                setattr(d.g[0], f, None)
        self.dx_raw = dx
        dxo = None if dx is None else dx[:P * d.ic].view(d.N, d.H, d.W, d.ic).permute(0, 3, 1, 2)
        return rc, dxo, (None if grads is None else OrderedDict(zip(self.names, grads)))

    def guard_ok(self, t, n):
        return bool((t[int(n):] == self.SENTINEL).all())
