"""Helpers shared by the tests of MBConv blocks WITHOUT an expand convolution (mid_channels <= in_channels:
tests/test_noexp_*.py, tests/test_gpu_noexp*.py) and by the generator of their fixture (tests/golden/make_golden_noexp.py):
the block scenarios of the oracle pin, oracle / HIP block pairs with identical weights, seeds whose float64 pre-activations stay
clear of every activation kink, a raw-ABI launcher for what the Python modules do not expose (route word, accumulation, guard
bands, dx == NULL), and a ``model.config`` whose first stage opens with such a block."""
import itertools

import torch

import _k7
import _rawcell
import tfnas_oracle as orc
from _k7 import hand_macs_in_M  # noqa: F401  (one hand counter for every block kind)
from _rawcell import KINKS, KINK_TAU, ws_of  # noqa: F401

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
    """_rawcell.cell_desc of an expand-free block (mc = None: ic)"""
    from tfnas_amd import _lib
    return _rawcell.cell_desc(_lib.NOEXPAND, N, H, W, ic, oc, ic if mc is None else mc, k, stride, act, se, flags, G, mode,
                              need_wgrad)


def raw_cell(o, x):
    """_rawcell.RawCell of an oracle block without expand convolution"""
    from tfnas_amd import _lib
    return _rawcell.RawCell(o, x, _lib.NOEXPAND, _rawcell.param_names(_lib.NOEXPAND, o.se_channels))


# ------------------------------------------------------------------------------------------------ derived network
def noexp_network_config(num_classes=20):
    """_k7.base_network_config whose stage1 OPENS with a block without expand convolution (16 -> 16 -> 24, stride 2, SE 16) --
    recorded as the reference records it, mid_channels == in_channels."""
    cfg = _k7.base_network_config(num_classes)
    first = cfg['stage1'][0]
    first['mid_channels'] = first['in_channels']
    first['se_channels'] = 16
    return cfg
