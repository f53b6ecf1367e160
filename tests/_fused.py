"""Helpers shared by the tests of Fused-MBConv blocks (tests/test_fused_*.py, tests/test_gpu_fused*.py) and by the generator of
their fixture (tests/golden/make_golden_fused.py): a CPU restatement of the block from torch ops in both forms (the reference has
no such block; the fixture pins the restatement to a composition of the reference's own classes), HIP / restatement pairs with
identical weights, seeds whose float64 pre-activations stay clear of every activation kink, a raw-ABI launcher for what the
Python modules do not expose (accumulation, dx == NULL, need_wgrad = 0), and a ``model.config`` whose stage 1 holds a fused block."""
import copy
import itertools
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

import _k7
import _rawcell
from _rawcell import KINKS, KINK_TAU, ws_of  # noqa: F401

BN_EPS = 1e-5


def _act(z, name):
    if name == 'relu':
        return F.relu(z)
    if name == 'swish':
        return z * torch.sigmoid(z)
    if name == 'relu6':
        return F.relu6(z)
    if name == 'h-swish':
        return z * F.relu6(z + 3.0) / 6.0
    raise ValueError(name)


def _seq(**mods):
    return nn.Sequential(OrderedDict(mods))


class FusedRef(nn.Module):
    """z = act(BN_a(conv3x3(x, stride, padding 1)));  [z <- z * sigmoid(W_e act(W_r mean_hw(z) + b_r) + b_e)];
    y = BN_b(conv1x1(z)) [+ x where in == out and stride == 1].
    search form (derived=False): batch statistics, biased variance, eps 1e-5, no affine, no buffers.
    derived form: nn.BatchNorm2d (affine, running statistics with momentum 0.1, unbiased running variance; eval: the running
    statistics), drop-connect on the residual branch in training -- ``drop_u``: injected U[0,1) draws [N] (else torch.rand).
    Parameter names are those of tfnas_amd.layers.FusedMBConvBlock."""

    def __init__(self, ic, mid, se, oc, stride, act, derived=False):
        super().__init__()
        self.in_channels, self.mid_channels, self.se_channels, self.out_channels = ic, mid, se, oc
        self.kernel_size, self.stride, self.act_func, self.derived = 3, stride, act, derived
        self.drop_connect_rate = 0.0
        self.drop_u = None

        def bn(ch):
            return dict(bn=nn.BatchNorm2d(ch)) if derived else {}
        self.fused_conv = _seq(conv=nn.Conv2d(ic, mid, 3, stride, 1, bias=False), **bn(mid))
        self.squeeze_excite = _seq(conv_reduce=nn.Conv2d(mid, se, 1), conv_expand=nn.Conv2d(se, mid, 1)) if se > 0 else None
        self.point_linear = _seq(conv=nn.Conv2d(mid, oc, 1, bias=False), **bn(oc))
        self.has_residual = ic == oc and stride == 1

    def _bn(self, seq, z):
        if self.derived:
            return seq.bn(z)
        return F.batch_norm(z, None, None, None, None, True, 0.0, BN_EPS)

    def forward(self, x, det=None):
        zh = self._bn(self.fused_conv, self.fused_conv.conv(x))
        z = _act(zh, self.act_func)
        if det is not None:
            det['zh'] = zh
        if self.squeeze_excite is not None:
            hpre = self.squeeze_excite.conv_reduce(z.mean((2, 3), keepdim=True))
            if det is not None:
                det['hpre'] = hpre
            z = z * torch.sigmoid(self.squeeze_excite.conv_expand(_act(hpre, self.act_func)))
        y = self._bn(self.point_linear, self.point_linear.conv(z))
        if self.has_residual:
            if self.derived and self.training and self.drop_connect_rate > 0.0:
                keep = 1.0 - self.drop_connect_rate
                u = self.drop_u if self.drop_u is not None else torch.rand(x.size(0))
                y = y.div(keep) * torch.floor(keep + u.to(y.dtype).view(-1, 1, 1, 1))
            y = y + x
        return y


def seed_weights(blk, gen, bn=True):
    """non-trivial SE biases and (derived form) BatchNorm state"""
    with torch.no_grad():
        for k, p in blk.named_parameters():
            if k.startswith('squeeze_excite.') and p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    if bn and blk.derived:
        _k7.randomise_bn(blk, gen)


def ref_block(ic, mid, se, oc, stride, act, seed, derived=False):
    """FusedRef (float32, train mode) with seeded weights."""
    torch.manual_seed(seed)
    blk = FusedRef(ic, mid, se, oc, stride, act, derived)
    seed_weights(blk, torch.Generator().manual_seed(seed + 1))
    return blk.train()


def hip_block_like(o):
    """The product's FusedMBConvBlock on cuda with the restatement's geometry, weights and (derived form) BatchNorm state."""
    from tfnas_amd.layers import FusedMBConvBlock
    m = FusedMBConvBlock(o.in_channels, o.mid_channels, o.se_channels, o.out_channels, 3, o.stride, affine=o.derived,
                         act_func=o.act_func)
    m.load_state_dict(o.state_dict())
    m.drop_connect_rate = o.drop_connect_rate
    return m.cuda()


# ------------------------------------------------------------------------------------------------ kinks and seeds
def kink_distance(o, x):
    """Smallest distance, in a float64 copy of ``o`` (same mode), of a BN_a output or an SE hidden pre-activation from a kink of
    the block's activation (inf for swish).  The copy's buffers move, not ``o``'s."""
    kinks = KINKS[o.act_func]
    if not kinks:
        return float('inf')
    o64 = copy.deepcopy(o).double()
    det = {}
    with torch.no_grad():
        o64(x.double(), det)
    return min(float((z - kk).abs().min()) for z in det.values() for kk in kinks)


def case_data(N, ic, mid, se, oc, H, W, stride, act, derived=False, base=100, eval_mode=False, prep=None):
    """(restatement block, x, cotangent, seed): the first seed from ``base`` up whose float64 pre-activations all stay at least
    KINK_TAU from a kink (ReLU family; swish takes ``base``).  Chosen on the CPU from the restatement alone.  ``prep(o)`` may
    change the block (drop-connect, a negative gamma) before the distance is taken."""
    for seed in range(base, base + 200):
        o = ref_block(ic, mid, se, oc, stride, act, seed, derived)
        if prep is not None:
            prep(o)
        if eval_mode:
            o.eval()
        gen = torch.Generator().manual_seed(seed + 2)
        x = torch.randn(N, ic, H, W, generator=gen)
        r = torch.randn(N, oc, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=gen)
        if kink_distance(o, x) >= KINK_TAU:
            return o, x, r, seed
    raise AssertionError('no seed keeps the pre-activations clear of the kinks')


# the geometries of tests/test_gpu_fused*.py: (N, ic, mid, se, oc, H, W, stride, act); every one is asserted kink-clear on the CPU
# by tests/test_fused_oracle_pin.py
ACTS = ('relu', 'swish', 'relu6', 'h-swish')
SMALL = [(2, 8, 22, se, oc, 7, 9, s, act) for s, (act, se, oc) in itertools.product(
    (1, 2), (('relu', 0, 8), ('swish', 8, 12), ('relu6', 8, 8), ('h-swish', 0, 12)))]
SMALL += [(2, 8, 22, 8, 8, 9, 6, 2, 'relu'), (2, 8, 22, 0, 12, 9, 6, 1, 'swish')]              # an even width
TAP = [(2, 20, 36, 8, 20, 9, 13, 1, 'relu'), (2, 20, 36, 0, 24, 9, 13, 2, 'h-swish')]           # K = 180: tap boundary in a chunk
# 588 rows: four full 128-row tiles and a ragged fifth, the residual gradient in the dgrad store; then 14 -> 7 and 7 -> 4
TILES = [(3, 24, 50, 8, 24, 14, 14, 1, 'relu'), (3, 24, 50, 0, 24, 14, 14, 2, 'swish'), (3, 24, 50, 8, 24, 7, 7, 2, 'relu6')]
GEOMS = SMALL + TAP + TILES
DERIVED_GEOMS = [SMALL[0], SMALL[5], SMALL[2], TAP[1], TILES[0]]
RAW_GEOM = (2, 8, 22, 8, 8, 7, 9, 1, 'relu')          # accumulation, dx == NULL, need_wgrad = 0, GEMM modes


DROP_U = torch.tensor([0.05, 0.9, 0.3])         # floor(0.6 + u): images 0 and 2 are dropped (N <= 3)


def derived_case(geom, mode):
    """case_data of the derived form in 'train' | 'train_drop' (injected draws, rate 0.4) | 'eval' mode, with a negative gamma at
    both BatchNorm sites (the affine fold must not rely on gamma > 0)."""
    def prep(o):
        with torch.no_grad():
            o.fused_conv.bn.weight[0] = -0.7
            o.point_linear.bn.weight[1] = -0.4
        if mode == 'train_drop':
            o.drop_connect_rate = 0.4
            o.drop_u = DROP_U[:geom[0]].clone()
    return case_data(*geom, derived=True, base=500, eval_mode=(mode == 'eval'), prep=prep)


def geom_id(g):
    return 'n%d_ic%d_m%d_se%d_oc%d_%dx%d_s%d_%s' % g


# ------------------------------------------------------------------------------------------------ pin
# stride x activation x SE x form at 2 x 16 x 9 x 13, mid 40, out 16 (residual at stride 1), float64
PIN_GEOM = dict(N=2, ic=16, mid=40, oc=16, H=9, W=13, se=8)
PIN_CASES = list(itertools.product((1, 2), ACTS, (0, PIN_GEOM['se'])))
PIN_FORMS = ('search', 'derived')
PIN_DROP = _k7.PIN_DROP


def pin_tag(form, case):
    return '%s_s%d_%s_se%d' % ((form,) + tuple(case))


def pin_block(form, case):
    """The restatement's block of one pin case (float64, train mode) with seeded weights, its input, cotangent and RNG seed."""
    s, act, se = case
    q = PIN_GEOM
    seed = 7000 + 83 * PIN_CASES.index(case) + (0 if form == 'search' else 41)
    blk = ref_block(q['ic'], q['mid'], se, q['oc'], s, act, seed, derived=(form == 'derived'))
    if form == 'derived':
        blk.drop_connect_rate = PIN_DROP
    blk = blk.double().train()
    gen = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(q['N'], q['ic'], q['H'], q['W'], generator=gen).double()
    r = torch.randn(q['N'], q['oc'], (q['H'] - 1) // s + 1, (q['W'] - 1) // s + 1, generator=gen).double()
    return blk, x, r, seed + 3


pin_run = _k7.pin_run            # forward + backward: out, dx, every parameter gradient, the buffers


def pin_record(res):
    """What the fixture keeps of pin_run's result: _golden.probe of every tensor, and the four corner taps and the centre tap of
    the dense weight gradient's first six output channels whole."""
    import numpy as np
    import _golden
    out = OrderedDict()
    for k, v in res.items():
        out[k] = _golden.probe(torch.from_numpy(np.asarray(v)))
        if k == 'g.fused_conv.conv.weight':
            a = np.asarray(v)
            out[k + '.taps'] = a[:6].reshape(6, a.shape[1], 9)[:, :, ::2].copy()
    return out


# ------------------------------------------------------------------------------------------------ comparison
def compare(o, m, x, r):
    """{name: (max abs error, max |reference|)} of out, dx, every parameter gradient and every buffer of one forward + backward
    of the restatement ``o`` (CPU float32) and the product block ``m`` (cuda)."""
    import _hipcheck as hc
    for p in list(o.parameters()) + list(m.parameters()):
        p.grad = None
    xo = x.clone().requires_grad_(True)
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    yo, ym = o(xo), m(xm)
    res = OrderedDict(out=hc.err(ym, yo))
    (yo * r).sum().backward()
    (ym * r.cuda()).sum().backward()
    res['dx'] = hc.err(xm.grad, xo.grad)
    po, pm = dict(o.named_parameters()), dict(m.named_parameters())
    assert list(po) == list(pm)
    for k in po:
        assert pm[k].grad is not None, k
        res['g.' + k] = hc.err(pm[k].grad, po[k].grad)
    bo, bm = dict(o.named_buffers()), dict(m.named_buffers())
    assert list(bo) == list(bm)
    for k in bo:
        res['b.' + k] = hc.err(bm[k].float(), bo[k].float())
    return res


# ------------------------------------------------------------------------------------------------ raw ABI
def cell_desc(N, H, W, ic, oc, mc, stride=1, act=0, se=0, flags=None, k=3, G=1, mode=0, need_wgrad=0):
    """_rawcell.cell_desc of a Fused-MBConv block"""
    from tfnas_amd import _lib
    return _rawcell.cell_desc(_lib.FUSED, N, H, W, ic, oc, mc, k, stride, act, se, flags, G, mode, need_wgrad)


def raw_cell(o, x, gemm=None):
    """_rawcell.RawCell of a search-form FusedRef"""
    from tfnas_amd import _lib
    return _rawcell.RawCell(o, x, _lib.FUSED, _rawcell.param_names(_lib.FUSED, o.se_channels), gemm=gemm)


def ref_grads(o, x, r):
    """out, dx and {name: gradient} of one forward + backward of the restatement"""
    for p in o.parameters():
        p.grad = None
    xs = x.clone().requires_grad_(True)
    y = o(xs)
    (y * r).sum().backward()
    return y.detach(), xs.grad, OrderedDict((k, p.grad.clone()) for k, p in o.named_parameters())


# ------------------------------------------------------------------------------------------------ derived network
def fused_network_config(num_classes=20):
    """_k7.base_network_config whose stage1 holds Fused-MBConv blocks: 16 -> 48 -> 24 at stride 2 with SE 16, then 24 -> 50 -> 24
    (ragged width, residual) without."""
    cfg = _k7.base_network_config(num_classes)
    a, b = cfg['stage1']
    a.update(name='FusedMBConvBlock', kernel_size=3, mid_channels=48, se_channels=16)
    b.update(name='FusedMBConvBlock', kernel_size=3, mid_channels=50, se_channels=0)
    return cfg


def hand_counts(cfg, size):
    """(MACs in millions at ``size`` x ``size``, parameters in millions): the hand counters of every block kind"""
    return _k7.hand_macs_in_M(cfg, size), _k7.hand_params_in_MB(cfg)
