"""Helpers shared by the tests of MBConv blocks WITHOUT an expand convolution (mid_channels <= in_channels:
tests/test_noexp_*.py, tests/test_gpu_noexp*.py) and by the generator of their fixture (tests/golden/make_golden_noexp.py):
the block scenarios of the oracle pin, oracle / HIP block pairs with identical weights, seeds whose float64 pre-activations stay
clear of every activation kink, a raw-ABI launcher for what the Python modules do not expose (route word, accumulation, guard
bands, dx == NULL), and a ``model.config`` whose first stage opens with such a block."""
import ctypes as C
import itertools
from collections import OrderedDict

import torch

import _k7
import tfnas_oracle as orc

# ------------------------------------------------------------------------------------------------ oracle pin (blocks)
# mid x stride x activation x SE at 2 x 16 x 9 x 13, out 16 (residual at stride 1); mid 16 and mid 8 both build the block without
# expand convolution and normalise mid_channels to 16 (models/layers.py:463-482).  Kernel size 3 for mid 16, 5 for mid 8.
PIN_GEOM = dict(N=2, ic=16, oc=16, H=9, W=13, se=8)
PIN_MIDS = (16, 8)
PIN_CASES = [c for c in itertools.product(PIN_MIDS, (1, 2), ('relu', 'swish'), (0, PIN_GEOM['se']))]
PIN_FORMS = ('search', 'derived')
PIN_DROP = _k7.PIN_DROP


def pin_k(case):
    return 3 if case[0] == 16 else 5


def pin_tag(form, case):
    return '%s_m%d_s%d_%s_se%d' % ((form,) + tuple(case))


def pin_oracle_block(form, case):
    """The oracle's block of one pin case (float64) with seeded weights, its input, cotangent and RNG seed."""
    mid, s, act, se = case
    q = PIN_GEOM
    seed = 5000 + 89 * PIN_CASES.index(case) + (0 if form == 'search' else 50)
    torch.manual_seed(seed)
    cls = orc.MBConv if form == 'search' else orc.DerivedBlock
    blk = cls(q['ic'], mid, se, q['oc'], pin_k(case), s, act)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))      # SE biases
    if form == 'derived':
        _k7.randomise_bn(blk, gen)
        blk.drop_connect_rate = PIN_DROP
    blk = blk.double().train()
    x = torch.randn(q['N'], q['ic'], q['H'], q['W'], generator=gen).double()
    r = torch.randn(q['N'], q['oc'], (q['H'] - 1) // s + 1, (q['W'] - 1) // s + 1, generator=gen).double()
    return blk, x, r, seed + 2


pin_run = _k7.pin_run            # forward + backward: out, dx, every parameter gradient, the buffers
pin_record = _k7.pin_record      # what the fixture keeps: the depthwise weight gradient whole, _golden.probe of the rest


# ------------------------------------------------------------------------------------------------ block pairs
def _seed_weights(blk, gen):
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))


def oracle_block(ic, se, oc, k, stride, act, seed, derived=False, mc=None):
    """orc.MBConv / orc.DerivedBlock (float32, train mode) with seeded weights; mc = None: no expand convolution (mid = in)."""
    torch.manual_seed(seed)
    cls = orc.DerivedBlock if derived else orc.MBConv
    blk = cls(ic, ic if mc is None else mc, se, oc, k, stride, act)
    gen = torch.Generator().manual_seed(seed + 1)
    _seed_weights(blk, gen)
    if derived:
        _k7.randomise_bn(blk, gen)
    return blk.train()


def hip_block_like(o, affine=False):
    """The product's MBInvertedResBlock on cuda with the oracle block's geometry, weights and (affine) BatchNorm state."""
    from tfnas_amd.layers import MBInvertedResBlock
    m = MBInvertedResBlock(o.in_channels, o.mid_channels, o.se_channels, o.out_channels, o.kernel_size, o.stride, affine=affine,
                           act_func=o.act_func)
    m.load_state_dict(o.state_dict())
    m.drop_connect_rate = getattr(o, 'drop_connect_rate', 0.0)
    return m.cuda()


# ------------------------------------------------------------------------------------------------ kinks
KINKS = {'relu': (0.0,), 'swish': (), 'relu6': (0.0, 6.0), 'h-swish': (-3.0, 3.0)}
KINK_TAU = 1e-4


def kink_distance(o, x):
    """Smallest distance, in a float64 copy of the search-form oracle block ``o``, of a BN2 output or an SE hidden pre-activation
    from a kink of the block's activation (inf for swish).  Run inside _acts.wrapped_oracle() for relu6 / h-swish."""
    import copy
    import torch.nn.functional as F
    kinks = KINKS[o.act_func]
    if not kinks:
        return float('inf')
    o64 = copy.deepcopy(o).double()
    det = {}
    with torch.no_grad():
        o64(x.double(), det)
        zs = [det['Dh']]
        if o64.squeeze_excite is not None:
            se = o64.squeeze_excite
            zs.append(F.conv2d(det['pooled'], se.conv_reduce.weight, se.conv_reduce.bias))
    return min(float((z - kk).abs().min()) for z in zs for kk in kinks)


# ------------------------------------------------------------------------------------------------ raw ABI
def cell_desc(N, H, W, ic, oc, k=3, stride=1, act=0, se=0, flags=None, mc=None, G=1, mode=0, need_wgrad=0):
    """A descriptor of one block; flags = None: TFNAS_CELL_NOEXPAND plus whatever k / act need."""
    from tfnas_amd import _lib
    d = _lib.TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.G, d.mode = N, H, W, ic, oc, stride, act, G, mode
    d.has_res = int(mode == 0 and ic == oc and stride == 1)
    d.eps, d.need_wgrad = 1e-5, need_wgrad
    for g in range(G):
        d.g[g].mc, d.g[g].k, d.g[g].se = (ic if mc is None else mc), k, se
    d.flags = (_lib.CELL_NOEXPAND | (_lib.CELL_K7 if k == 7 else 0) | _lib.act_flags(act)) if flags is None else flags
    return d


def ws_of(lib, d):
    from tfnas_amd import _lib
    ws = _lib.TfnasCellWs()
    assert lib.tfnas_cell_ws(C.byref(d), C.byref(ws)) == 0
    return ws


class RawCell:
    """One expand-free block through tfnas_mixedop_fwd / _bwd with caller-made buffers: ``guard`` sentinel floats follow D and dx,
    the route word, TFNAS_CELL_ACCUM_WGRAD and dx == NULL are the caller's choice.  Weights come from an oracle block."""
    SENTINEL = -777.25

    def __init__(self, o, x, guard=64):
        from tfnas_amd import _lib
        self.lib, self._lib = _lib.lib(), _lib
        self.o, self.guard = o, guard
        self.dev = torch.device('cuda')
        N, _, H, W = x.shape
        self.xh = x.permute(0, 2, 3, 1).contiguous().cuda()
        self.d = cell_desc(N, H, W, o.in_channels, o.out_channels, o.kernel_size, o.stride, _lib.act_id(o.act_func),
                           o.se_channels)
        _lib.check(self.lib.tfnas_cell_plan(C.byref(self.d)), 'tfnas_cell_plan')
        self.ws = ws_of(self.lib, self.d)
        names = ['dw', 'proj'] + (['se_rw', 'se_rb', 'se_ew', 'se_eb'] if o.se_channels else [])
        op = o.params()
        self.names = names
        self.w = [op[n].detach().float().contiguous().cuda() for n in names]
        for f, t in zip(_lib._W_FIELDS[1:], self.w):
            setattr(self.d.g[0], f, t.data_ptr())

    def _buf(self, n, guard=0, dtype=torch.float32):
        t = torch.empty(int(n) + guard, device=self.dev, dtype=dtype)
        if guard:
            t[int(n):] = self.SENTINEL
        return t

    def forward(self, route=0):
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
        return self.out

    def backward(self, r, route=0, need_wgrad=True, want_dx=True, accum_into=None):
        """returns (rc, dx or None, [weight gradients] or None); accum_into: tensors the gradients are ADDED to"""
        from tfnas_amd.functions import _part, _stream
        d, ws, ptr = self.d, self.ws, self._lib.ptr
        d.route, d.need_wgrad = route, int(need_wgrad)
        base = d.flags
        grads = None
        if need_wgrad:
            grads = [g.clone() for g in accum_into] if accum_into is not None else [torch.full_like(w, 3.5) for w in self.w]
            for f, t in zip(self._lib._G_FIELDS[1:], grads):
                setattr(d.g[0], f, t.data_ptr())
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
        return rc, dx, grads

    def guard_ok(self, t, n):
        return bool((t[int(n):] == self.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ derived network
def noexp_network_config(num_classes=20):
    """A ``model.config`` (parsing.derived_config: two blocks per stage) whose stage1 OPENS with a block without expand
    convolution (16 -> 16 -> 24, stride 2, SE 16) -- recorded as the reference records it, mid_channels == in_channels."""
    from tfnas_amd import geometry as g, parsing
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 2))
                       for i, (st, bl) in enumerate(g.initial_mc_num_dddict().items()))
    cfg = parsing.derived_config(arch, g.initial_mc_num_dddict(), num_classes)
    first = cfg['stage1'][0]
    first['mid_channels'] = first['in_channels']
    first['se_channels'] = 16
    return cfg


def hand_macs_in_M(cfg, size):
    """_k7.hand_macs_in_M with the fork for blocks without expand convolution (no 1 x 1 expand term)."""
    hw = (size - 1) // 2 + 1
    total = 3 * 3 * 3 * 32 * hw * hw
    total += 3 * 3 * 32 * hw * hw + (32 * 8 + 8) + (8 * 32 + 32) + 32 * 16 * hw * hw
    for st in ('stage1', 'stage2', 'stage3', 'stage4', 'stage5', 'stage6'):
        for c in cfg[st]:
            ic, mc, se, oc, k, s = (c[n] for n in ('in_channels', 'mid_channels', 'se_channels', 'out_channels', 'kernel_size',
                                                    'stride'))
            if mc > ic:
                total += ic * mc * hw * hw
            else:
                mc = ic
            hw = (hw - 1) // s + 1
            total += k * k * mc * hw * hw
            if se:
                total += 2 * mc * se + se + mc
            total += mc * oc * hw * hw
    total += 320 * 1280 * hw * hw + 1280 * hw * hw
    ncls = cfg['classifier']['out_features']
    total += 1280 * ncls + ncls
    return total / 1e6
