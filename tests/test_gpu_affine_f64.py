"""The derived-network ("retrain") path's affine blocks and head at the C ABI against the float64 oracle of tests/_affineref.py:
tfnas_mbconv_fwd/bwd, tfnas_head_fwd/bwd/wgrad, tfnas_head_affine_fwd/bwd, csrc/bn_affine.hip and the Python mirror
(functions._bn_struct, MBConvAffineFn).  Every tensor is held to the cell gate ``2e-5 + 1e-4 max|ref|``, running statistics to
``1e-6 + 1e-5 |ref|`` elementwise; tests/test_affine_refs.py shows on the CPU that the fp32 oracle sits within a quarter of
those gates of the float64 one on every case used here, and that the cases carry the edges they claim (gamma < 0, |beta / gamma|
up to 10, running statistics off their defaults, momentum 0.01, inputs with a per-channel mean).

Through ``layers.MBInvertedResBlock(affine=True)`` where the module can express the case (train, eval, drop-connect, the
sync-stats hook), through raw ctypes where it cannot (the rewritten statistics tables, NULL pointers of TfnasBnAffine,
drop_scale without a residual, the heads with their split backward).

Observed worst err / gate per tensor class on an MI355X (every test prints its own line, ``AFFINE_F64 ...``; 1.0 is the gate):
  blocks (modules and raw)   y 0.011   dx 0.036   conv / SE gradients 0.020   d gamma / d beta 0.058   running statistics 0.010
                             rewritten tables (m_eff, r_eff) 0.007 in train mode, 0 in eval mode
  heads                      pooled 0.025   dx 0.006   g_expand 0.043   d gamma / d beta 0.018   running statistics 0.011
                             rewritten table 0.015
i.e. the kernels sit one to two orders of magnitude inside the gates, the |beta / gamma| = 10 channels included -- about where the
fp32 oracle itself sits (tests/test_affine_refs.py: up to 0.024 of the gate).  Two deliberately wrong builds of
csrc/bn_affine.hip were tried against this file (not kept): without the unbiased-variance factor of k_bn_fwd_fix 13 of the 28
tests fail (every train-mode running_var), with the sign of beta * c flipped in k_bn_bwd_fix 12 fail (dx and the gradients
upstream of an affine site).
"""
import ctypes as C
from collections import OrderedDict

import pytest
import torch

import _affineref as ar
from _rawcell import param_names

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 64


def _report(tag, ratios):
    print('AFFINE_F64 %-26s %s' % (tag, '  '.join('%s %.4f' % kv for kv in ar.classes(ratios).items())))


def _hold(tag, got, ref, only=None):
    """every tensor of ``ref`` (or those named in ``only``) within its gate"""
    if only is not None:
        ref = OrderedDict((k, ref[k]) for k in only)
    ratios = ar.compare(got, ref)
    _report(tag, ratios)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)
    return ratios


# ================================================================================================== through the modules
def _module(case, modes=None):
    from tfnas_amd import functions as F
    from tfnas_amd.layers import MBInvertedResBlock
    ic, mc, se, oc, k, s, act = case.geom[:7]
    m = MBInvertedResBlock(ic, mc, se, oc, k, s, affine=True, act_func=act)
    m.load_state_dict(case.o.state_dict())
    for bn in m.bn_modules():
        bn.momentum = ar.MOMENTUM
    if modes is not None:
        F.adopt_modes(m, modes)
    return m.cuda()


def _run_module(m, case, mode=None, after_forward=None):
    mode = case.mode if mode is None else mode
    m.train(mode != 'eval')
    m.drop_connect_rate, m.drop_u = 0.0, None
    if case.u is not None:
        m.drop_connect_rate, m.drop_u = 1.0 - ar.KEEP, case.u
    xm = case.x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = m(xm)
    if after_forward is not None:
        torch.cuda.synchronize()
        after_forward()
    (y * case.r.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = OrderedDict(y=y.detach(), dx=xm.grad)
    for k, p in m.named_parameters():
        got['g.' + k] = p.grad
    for k, b in m.named_buffers():
        if 'running' in k:
            got['b.' + k] = b.detach().clone()
    return got


@pytest.mark.parametrize('shape,mode', ar.BLOCK_CASES)
def test_affine_block_matches_float64_oracle(shape, mode):
    """y, dx, every conv / SE / BatchNorm parameter gradient and every running buffer; eval: the backward with the statistics as
    constants, running buffers untouched; alldrop: every image dropped -- out IS x, no gradient reaches a parameter, the running
    statistics still move"""
    case = ar.block_case(shape, mode)
    m = _module(case)
    got = _run_module(m, case)
    assert set(got) == {k for k in case.ref if not k.startswith('_')}
    _hold(case.name, got, case.ref)
    for bn in m.bn_modules():
        assert int(bn.num_batches_tracked) == (0 if mode == 'eval' else 1)
    if mode == 'alldrop':
        assert torch.equal(got['y'].cpu(), case.x)
        assert torch.equal(got['dx'].cpu(), case.r)
        for k, v in got.items():
            if k.startswith('g.'):
                assert float(v.abs().max()) <= 2e-5, k               # (the gate of a reference that is exactly 0)
        for k, b in case.o.named_buffers():
            if 'running' in k:
                assert not torch.equal(got['b.' + k].cpu(), b), k
    if mode == 'eval':
        for k, b in case.o.named_buffers():
            if 'running' in k:
                assert torch.equal(got['b.' + k].cpu(), b), k


def test_sync_hook_of_world_two_is_the_doubled_batch():
    """A sync-stats hook that enqueues nothing models two ranks with identical shards (all-reduce, then / world, is the identity):
    y and dx are the first half of the float64 oracle on cat([x, x]), parameter gradients half of its, and running_var carries
    2 cnt / (2 cnt - 1) (launch_bn_fwd_fix: gcnt = cnt * world; at cnt = 70 the one-rank correction misses the gate by 5x).  The
    hook sees the forward's three tables in order -- 2 M, 2 M, 2 oc doubles -- and, in eval mode, none."""
    from tfnas_amd import functions as F
    calls = []

    def hook(_user, _table, n, _stream):
        calls.append(int(n))
        return 0
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)(hook)
    modes = F.HipModes(sync=(C.cast(cb, C.c_void_p).value, None, 2))
    case = ar.block_case('D', 'train')
    ref2 = ar.variant_ref('D', 'train', 'doubled')
    N, oc = case.x.shape[0], case.geom[3]
    m = _module(case, modes)
    fwd_calls = []
    got = _run_module(m, case, after_forward=lambda: fwd_calls.extend(calls))
    M = m._plan.desc(N, case.x.shape[2], case.x.shape[3])[0].M
    assert fwd_calls == [2 * M, 2 * M, 2 * oc], fwd_calls
    assert calls[3:] == [2 * oc, 2 * M, 2 * M], calls           # (the backward's three BatchNorm-backward sum tables)
    want = OrderedDict()
    for k, v in ref2.items():
        if not k.startswith('_'):
            want[k] = v[:N] if k in ('y', 'dx') else 0.5 * v if k.startswith('g.') else v
    _hold('D-train-sync2', got, want)
    # the one-rank correction cnt / (cnt - 1) is NOT what the buffers hold
    one = ar.compare(got, case.ref)
    assert max(v for k, v in one.items() if k.endswith('running_var')) > 1.0
    # eval mode normalises with the running statistics: nothing to reduce in the forward
    ecase = ar.block_case('D', 'eval')
    me = _module(ecase, modes)
    del calls[:]
    seen = []
    got = _run_module(me, ecase, after_forward=lambda: seen.extend(calls))
    assert seen == []
    _hold('D-eval-sync2', got, ecase.ref, only=('y',))
    del cb


# ================================================================================================== raw: tfnas_mbconv_fwd/bwd
class RawBlock:
    """One affine block through tfnas_mbconv_fwd / _bwd with caller-made buffers (as tests/_rawcell.RawCell for the search form):
    guard bands behind out, D, the statistics tables, dx and every running buffer; TfnasBnAffine built by hand."""
    SITES = ('inverted_bottleneck', 'depth_conv', 'point_linear')

    def __init__(self, case, sync=None):
        from tfnas_amd import _lib, functions as F
        self._lib, self.lib, self.F, self.case = _lib, _lib.lib(), F, case
        o = case.o
        self.dev = torch.device('cuda')
        N, _, H, W = case.x.shape
        self.xh = case.x.permute(0, 2, 3, 1).contiguous().cuda()
        d = self.d = _lib.describe_block(_lib.MBCONV, N, H, W, o.in_channels, o.mid_channels, o.se_channels, o.out_channels,
                                         o.kernel_size, o.stride, _lib.act_id(o.act_func))
        F.HipModes(sync=sync).apply(d, _lib.MBCONV)
        _lib.check(self.lib.tfnas_cell_plan(C.byref(d)), 'tfnas_cell_plan')
        self.ws = _lib.TfnasCellWs()
        _lib.check(self.lib.tfnas_cell_ws(C.byref(d), C.byref(self.ws)), 'tfnas_cell_ws')
        self.names = param_names(_lib.MBCONV, o.se_channels > 0)
        sd = dict(o.named_parameters())
        self.w = [sd[n].detach().float().contiguous().cuda() for n in self.names]
        self.fields = _lib.MBCONV.bound(o.se_channels > 0)
        for k, t in zip(self.fields, self.w):
            setattr(d.g[0], _lib._W_FIELDS[k], t.data_ptr())
        bns = [getattr(o, s).bn for s in self.SITES]
        self.nch = [bn.num_features for bn in bns]
        self.gamma = [bn.weight.detach().clone().cuda() for bn in bns]
        self.beta = [bn.bias.detach().clone().cuda() for bn in bns]
        self.rmean0 = [bn.running_mean.detach().clone() for bn in bns]
        self.rvar0 = [bn.running_var.detach().clone() for bn in bns]

    def _buf(self, n, guard=0, dtype=torch.float32):
        t = torch.empty(int(n) + guard, device=self.dev, dtype=dtype)
        if guard:
            t[int(n):] = SENTINEL
        return t

    def _guarded(self, src):
        t = self._buf(src.numel(), GUARD)
        t[:src.numel()] = src.cuda()
        return t

    def guards_intact(self):
        return all(bool((t[int(n):] == SENTINEL).all()) for t, n in self._guards)

    def bn(self, mode, null_affine=(), null_running=False, grads=None, fresh=True):
        """TfnasBnAffine; fresh: the running buffers start over (copies of the case's, guard-banded: self.rmean / self.rvar)"""
        a = self._lib.TfnasBnAffine()
        if fresh:
            self.rmean = [self._guarded(t) for t in self.rmean0]
            self.rvar = [self._guarded(t) for t in self.rvar0]
            self._guards = [(t, n) for ts in (self.rmean, self.rvar) for t, n in zip(ts, self.nch)]
        for i in range(3):
            if i not in null_affine:
                a.weight[i], a.bias[i] = self.gamma[i].data_ptr(), self.beta[i].data_ptr()
            if not null_running:
                a.running_mean[i], a.running_var[i] = self.rmean[i].data_ptr(), self.rvar[i].data_ptr()
            if grads is not None and grads[i] is not None:
                a.g_weight[i], a.g_bias[i] = grads[i][0].data_ptr(), grads[i][1].data_ptr()
        a.momentum, a.eval = ar.MOMENTUM, int(mode == 'eval')
        return a

    def forward(self, bn, drop_scale=None):
        """out [N, oc, Ho, Wo]; keeps what the backward reads"""
        d, ws, ptr = self.d, self.ws, self._lib.ptr
        d.need_wgrad = 0
        self.E, self.D = self._buf(ws.E), self._buf(ws.D, GUARD)
        self.Pr, self.fsmall = self._buf(ws.Pr), self._buf(ws.fsmall)
        self.stats = self._buf(ws.stats, GUARD, torch.float64)
        self.out = self._buf(ws.out, GUARD)
        self._guards += [(self.D, ws.D), (self.stats, ws.stats), (self.out, ws.out)]
        part = self.F._part(ws.part, self.dev)
        self.ds = None if drop_scale is None else drop_scale.float().cuda()
        self._lib.check(self.lib.tfnas_mbconv_fwd(C.byref(d), C.byref(bn), ptr(self.ds), ptr(self.xh), ptr(self.E), ptr(self.D),
                                                  ptr(self.Pr), ptr(self.fsmall), ptr(self.stats), ptr(part), ptr(self.out),
                                                  self.F._stream(self.dev)), 'tfnas_mbconv_fwd')
        torch.cuda.synchronize()
        return self.out[:ws.out].view(d.N, d.Ho, d.Wo, d.oc).permute(0, 3, 1, 2)

    def table(self, site):
        """(m_eff, r_eff) of a site as k_bn_fwd_fix left them"""
        off = (self.ws.off_stats1, self.ws.off_stats2, self.ws.off_stats3)[site]
        t = self.stats[off:off + 2 * self.nch[site]].view(-1, 2)
        return t[:, 0], t[:, 1]

    def backward(self, mode, null_affine=(), null_grads=(), null_running=False):
        """(dx, {'g.<name>': gradient}) as the oracle names them; BatchNorm gradients of the sites not in ``null_grads``"""
        d, ws, ptr = self.d, self.ws, self._lib.ptr
        grads = [torch.full_like(w, 3.5) for w in self.w]
        for k, t in zip(self.fields, grads):
            setattr(d.g[0], self._lib._G_FIELDS[k], t.data_ptr())
        d.need_wgrad = 1
        gbn = [None if (i in null_grads or i in null_affine) else (torch.full((n,), 3.5, device=self.dev),
                                                                    torch.full((n,), 3.5, device=self.dev))
               for i, n in enumerate(self.nch)]
        bn = self.bn(mode, null_affine, null_running, gbn, fresh=False)
        rh = self.case.r.permute(0, 2, 3, 1).contiguous().cuda()
        P = d.N * d.H * d.W
        dx = self._buf(P * d.ic, GUARD)
        self._guards += [(dx, P * d.ic)]
        dZ, dEh, bsmall = self._buf(ws.dZ), self._buf(ws.dEh), self._buf(ws.bsmall)
        red = self._buf(ws.red, dtype=torch.float64)
        part = self.F._part(ws.part * 2, self.dev)
        dxp = self._buf(ws.dxp)
        dout_s = torch.empty_like(rh) if self.ds is not None else None
        try:
            self._lib.check(self.lib.tfnas_mbconv_bwd(C.byref(d), C.byref(bn), ptr(self.ds), ptr(self.xh), ptr(self.E), ptr(self.D),
                                                      ptr(self.Pr), ptr(self.fsmall), ptr(self.stats), ptr(rh), ptr(dout_s),
                                                      ptr(dZ), ptr(dEh), ptr(bsmall), ptr(red), ptr(part), ptr(dx), ptr(dxp),
                                                      self.F._stream(self.dev)), 'tfnas_mbconv_bwd')
            torch.cuda.synchronize()
        finally:
            d.need_wgrad = 0
            for f in self._lib._G_FIELDS:
                setattr(d.g[0], f, None)
        got = OrderedDict(dx=dx[:P * d.ic].view(d.N, d.H, d.W, d.ic).permute(0, 3, 1, 2))
        for n, g in zip(self.names, grads):
            got['g.' + n] = g
        for s, g in zip(self.SITES, gbn):
            if g is not None:
                got['g.%s.bn.weight' % s], got['g.%s.bn.bias' % s] = g
        return got

    def running(self):
        got = OrderedDict()
        for i, s in enumerate(self.SITES):
            got['b.%s.bn.running_mean' % s] = self.rmean[i][:self.nch[i]]
            got['b.%s.bn.running_var' % s] = self.rvar[i][:self.nch[i]]
        return got

    def run(self, mode, drop_scale=None, **kw):
        """forward + backward; everything the oracle's run returns, under its names"""
        fwd_kw = {k: v for k, v in kw.items() if k in ('null_affine', 'null_running')}
        y = self.forward(self.bn(mode, **fwd_kw), drop_scale)
        got = self.backward(mode, kw.get('null_affine', ()), kw.get('null_grads', ()), kw.get('null_running', False))
        got['y'] = y
        if not kw.get('null_running'):
            got.update(self.running())
        return got


@pytest.mark.parametrize('shape,mode', [('A', 'train'), ('B', 'train'), ('A', 'eval'), ('B', 'eval')])
def test_rewritten_statistics_tables_and_bn_gradients(shape, mode):
    """k_bn_fwd_fix leaves (m_eff, r_eff) in the three statistics tables: the map they define against the float64 oracle's
    BatchNorm at mu +- sigma, in train mode (batch statistics) and in eval mode (running statistics); after the backward
    g_weight / g_bias of every site, and the rest of the raw launch with them"""
    case = ar.block_case(shape, mode)
    rb = RawBlock(case)
    got = rb.run(mode)
    taps = case.ref['_taps']
    probes = OrderedDict(('table%d' % i, ar.probe_ratio(*rb.table(i), taps.sites[i])) for i in range(3))
    print('AFFINE_F64 %-26s %s' % (case.name + '-raw', '  '.join('%s %.4f' % kv for kv in probes.items())))
    assert max(probes.values()) <= 1.0, probes
    ratios = _hold(case.name + '-raw', got, case.ref)
    assert sum(1 for k in ratios if k.endswith('.bn.weight') or k.endswith('.bn.bias')) == 6
    assert rb.guards_intact()


def test_site_without_affine_part_is_plain_batchnorm():
    """TfnasBnAffine.weight[1] = bias[1] = NULL (and no gradient destination): the float64 oracle with gamma 1, beta 0 there"""
    case = ar.block_case('A', 'train')
    ref = ar.variant_ref('A', 'train', 'plain_site1')
    rb = RawBlock(case)
    got = rb.run('train', null_affine=(1,))
    only = [k for k in ref if not k.startswith('_') and not k.startswith('g.depth_conv.bn.')]
    assert 'g.depth_conv.bn.weight' not in got
    _hold('A-train-plain_site1', got, ref, only=only)
    m_eff, r_eff = rb.table(1)
    assert ar.probe_ratio(m_eff, r_eff, ref['_taps'].sites[1]) <= 1.0
    assert rb.guards_intact()


def test_null_running_statistics():
    """running_mean = running_var = NULL.  Train mode: batch statistics as ever, nothing is written (the running buffers the
    struct does not name keep their bits, every guard band is intact) and out is bit-identical to the launch that updates them.
    Eval mode: mean 0, variance 1."""
    case = ar.block_case('A', 'train')
    rb = RawBlock(case)
    y_upd = rb.forward(rb.bn('train')).clone()
    y = rb.forward(rb.bn('train', null_running=True))
    assert torch.equal(y, y_upd)
    assert rb.guards_intact()
    for i in range(3):
        assert torch.equal(rb.rmean[i][:rb.nch[i]].cpu(), rb.rmean0[i]) and torch.equal(rb.rvar[i][:rb.nch[i]].cpu(), rb.rvar0[i])
    _hold('A-train-null_running', OrderedDict(y=y), case.ref, only=('y',))
    ecase = ar.block_case('A', 'eval')
    ref = ar.variant_ref('A', 'eval', 'unit_running')
    eb = RawBlock(ecase)
    got = eb.run('eval', null_running=True)
    _hold('A-eval-unit_running', got, ref, only=[k for k in ref if not k.startswith('_') and not ar.is_running(k)])
    assert max(ar.probe_ratio(*eb.table(i), ref['_taps'].sites[i]) for i in range(3)) <= 1.0
    assert eb.guards_intact()


def test_bn_gradient_destinations_are_independent():
    """g_weight / g_bias NULL at one site: every other gradient of the launch keeps its bits"""
    case = ar.block_case('A', 'train')
    rb = RawBlock(case)
    full = rb.run('train')
    for site in range(3):
        part = RawBlock(case).run('train', null_grads=(site,))
        missing = {'g.%s.bn.weight' % RawBlock.SITES[site], 'g.%s.bn.bias' % RawBlock.SITES[site]}
        assert set(full) - set(part) == missing
        for k, v in part.items():
            assert torch.equal(v, full[k]), (site, k)


def test_drop_scale_without_a_residual_is_ignored():
    """shape B (stride 2, no residual): a drop_scale vector changes nothing, forward and backward, bit for bit"""
    case = ar.block_case('B', 'train')
    assert case.o.has_residual is False
    plain = RawBlock(case).run('train')
    scale = torch.floor(ar.KEEP + torch.tensor([0.95, 0.1])) / ar.KEEP
    assert float(scale[0]) > 1.0 and float(scale[1]) == 0.0      # (kept and dropped, were there a residual)
    dropped = RawBlock(case).run('train', drop_scale=scale)
    assert set(plain) == set(dropped)
    for k, v in plain.items():
        assert torch.equal(v, dropped[k]), k


# ================================================================================================== raw: the head
class RawHead:
    """tfnas_head_fwd/bwd/wgrad (form 'search') or tfnas_head_affine_fwd/bwd (forms 'train' / 'eval') with caller-made buffers"""

    def __init__(self, case):
        from tfnas_amd import _lib, functions as F
        self._lib, self.lib, self.F, self.case = _lib, _lib.lib(), F, case
        self.dev = torch.device('cuda')
        ic, mc, N, H, W = case.geom
        assert mc % 4 == 0                                        # (a ragged head is refused by the plan, and never launched)
        self.mc = mc
        d = self.d = _lib.TfnasCellDesc()
        d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, H, W, ic, 4, 1, _lib.act_id('swish'), 1, _lib.MODE_HEAD
        d.has_res, d.eps = 0, _lib.BN_EPS
        d.g[0].mc, d.g[0].k, d.g[0].se = mc, 3, 0
        F.HipModes().apply(d)
        _lib.check(self.lib.tfnas_cell_plan(C.byref(d)), 'tfnas_cell_plan')
        self.ws = _lib.TfnasCellWs()
        _lib.check(self.lib.tfnas_cell_ws(C.byref(d), C.byref(self.ws)), 'tfnas_cell_ws')
        self.xh = case.x.permute(0, 2, 3, 1).contiguous().cuda()
        self.w = case.o.conv.weight.detach().contiguous().cuda()
        d.g[0].w_expand = self.w.data_ptr()
        bn = case.o.bn
        self.gamma, self.beta = bn.weight.detach().clone().cuda(), bn.bias.detach().clone().cuda()
        self.affine = case.form != 'search'

    def _buf(self, n, guard=0, dtype=torch.float32):
        t = torch.empty(int(n) + guard, device=self.dev, dtype=dtype)
        if guard:
            t[int(n):] = SENTINEL
        return t

    def _bn(self, grads=None):
        a = self._lib.TfnasBnAffine()
        a.weight[0], a.bias[0] = self.gamma.data_ptr(), self.beta.data_ptr()
        a.running_mean[0], a.running_var[0] = self.rmean.data_ptr(), self.rvar.data_ptr()
        if grads is not None:
            a.g_weight[0], a.g_bias[0] = grads[0].data_ptr(), grads[1].data_ptr()
        a.momentum, a.eval = ar.MOMENTUM, int(self.case.form == 'eval')
        return a

    def forward(self):
        d, ws, ptr, st = self.d, self.ws, self._lib.ptr, self.F._stream(self.dev)
        d.need_wgrad = 0
        N, mc = d.N, self.mc
        self.E = self._buf(ws.E)
        self.stats = self._buf(2 * d.M, GUARD, torch.float64)
        self.pooled = self._buf(N * mc, GUARD)
        self.rmean, self.rvar = self._buf(mc, GUARD), self._buf(mc, GUARD)
        self.rmean[:mc], self.rvar[:mc] = self.case.o.bn.running_mean.cuda(), self.case.o.bn.running_var.cuda()
        self._guards = [(self.stats, 2 * d.M), (self.pooled, N * mc), (self.rmean, mc), (self.rvar, mc)]
        part = self.F._part(ws.part, self.dev)
        if self.affine:
            bn = self._bn()
            rc = self.lib.tfnas_head_affine_fwd(C.byref(d), C.byref(bn), ptr(self.xh), ptr(self.E), ptr(self.stats), ptr(part),
                                                ptr(self.pooled), st)
        else:
            rc = self.lib.tfnas_head_fwd(C.byref(d), ptr(self.xh), ptr(self.E), ptr(self.stats), ptr(part), ptr(self.pooled), st)
        self._lib.check(rc, 'tfnas_head_fwd')
        torch.cuda.synchronize()
        got = OrderedDict(pooled=self.pooled[:N * mc].view(N, mc))
        if self.affine:
            got['b.bn.running_mean'], got['b.bn.running_var'] = self.rmean[:mc], self.rvar[:mc]
        return got

    def table(self):
        t = self.stats[:2 * self.mc].view(-1, 2)
        return t[:, 0], t[:, 1]

    def backward(self, split=False):
        """dx, g.conv.weight (and g.bn.*); split (search form): tfnas_head_bwd without weight gradient, then tfnas_head_wgrad"""
        d, ws, ptr, st = self.d, self.ws, self._lib.ptr, self.F._stream(self.dev)
        P = d.N * d.H * d.W
        gw = torch.full_like(self.w, 3.5)
        gbn = (torch.full((self.mc,), 3.5, device=self.dev), torch.full((self.mc,), 3.5, device=self.dev))
        dp = self.case.r.contiguous().cuda()
        dEh, cb1 = self._buf(ws.dEh), self._buf(4 * d.M)
        red = self._buf(2 * d.M, dtype=torch.float64)
        dx = self._buf(P * d.ic, GUARD)
        self._guards.append((dx, P * d.ic))
        dxp = self._buf(ws.dxp)
        part = self.F._part(ws.part, self.dev)
        d.g[0].g_expand = gw.data_ptr()
        try:
            if self.affine:
                assert not split
                d.need_wgrad = 1
                bn = self._bn(gbn)
                rc = self.lib.tfnas_head_affine_bwd(C.byref(d), C.byref(bn), ptr(self.xh), ptr(self.E), ptr(self.stats), ptr(dp),
                                                    ptr(dEh), ptr(cb1), ptr(red), ptr(part), ptr(dx), ptr(dxp), st)
            else:
                d.need_wgrad = 0 if split else 1
                rc = self.lib.tfnas_head_bwd(C.byref(d), ptr(self.xh), ptr(self.E), ptr(self.stats), ptr(dp), ptr(dEh), ptr(cb1),
                                             ptr(red), ptr(part), ptr(dx), ptr(dxp), st)
                if split and rc == 0:
                    part2 = self.F._part(ws.part, self.dev)
                    rc = self.lib.tfnas_head_wgrad(C.byref(d), ptr(self.xh), ptr(self.E), ptr(dEh), ptr(cb1), ptr(part2), st)
            self._lib.check(rc, 'tfnas_head_bwd')
            torch.cuda.synchronize()
        finally:
            d.need_wgrad, d.g[0].g_expand = 0, None
        got = OrderedDict(dx=dx[:P * d.ic].view(d.N, d.H, d.W, d.ic).permute(0, 3, 1, 2))
        got['g.conv.weight'] = gw
        if self.affine:
            got['g.bn.weight'], got['g.bn.bias'] = gbn
        return got

    def guards_intact(self):
        return all(bool((t[int(n):] == SENTINEL).all()) for t, n in self._guards)


@pytest.mark.parametrize('idx,form', ar.HEAD_CASES)
def test_head_matches_float64_oracle(idx, form):
    """pooled, dx, g_expand -- and, affine, d gamma / d beta, the running statistics and the rewritten table -- of k_head_pool /
    k_head_bwd at 3 x 3 (fewer pixels than row lanes), 7 x 7 and a 64 -> 192 head at 5 x 9; the search form's split backward
    (tfnas_head_bwd without weight gradient + tfnas_head_wgrad) is bit-identical to the one-call form"""
    case = ar.head_case(idx, form)
    rh = RawHead(case)
    got = rh.forward()
    got.update(rh.backward())
    assert set(got) == {k for k in case.ref if not k.startswith('_')}
    _hold(case.name, got, case.ref)
    if form != 'search':
        p = ar.probe_ratio(*rh.table(), case.ref['_taps'].sites[0])
        print('AFFINE_F64 %-26s table0 %.4f' % (case.name, p))
        assert p <= 1.0
    if form == 'eval':
        assert torch.equal(got['b.bn.running_mean'].cpu(), case.o.bn.running_mean)
        assert torch.equal(got['b.bn.running_var'].cpu(), case.o.bn.running_var)
    assert rh.guards_intact()
    if form == 'search':
        sp = RawHead(case)
        first = sp.forward()
        assert torch.equal(first['pooled'], got['pooled'])
        both = sp.backward(split=True)
        for k, v in both.items():
            assert torch.equal(v, got[k]), k
        assert sp.guards_intact()
