"""Helpers shared by the ReLU6 / hard-swish tests (tests/test_act_*.py, tests/test_gpu_acts*.py) and by the generator of their
fixture (tests/golden/make_golden_act.py).

The CPU oracle's ``_act`` knows 'relu' and 'swish' and raises on anything else; it is not edited.  ``wrapped_oracle()`` installs a
wrapper over ``tfnas_oracle._act`` for the duration of a test (mbconv_forward, DerivedBlock and the rest call it through the
module global):
  'relu6'    the oracle's own 'relu' followed by clamp(max=6) -- so oracle.RELU_HOOK keeps replaying the lower kink;
  'h-swish'  x * relu6(x + 3) / 6, written as the reference writes it (models/layers.py:38-47);
  anything else is delegated to the original."""
import contextlib
import itertools
from collections import OrderedDict

import torch
import torch.nn.functional as F

import _hipcheck as hc
import _k7
import tfnas_oracle as orc

NEW_ACTS = ('relu6', 'h-swish')
UPPER_KINKS = {'relu6': (6.0,), 'h-swish': (-3.0, 3.0)}     # where a flipped decision is an O(1) gradient difference
BRANCH_EDGES = {'relu6': (0.0, 6.0), 'h-swish': (-3.0, 3.0)}


@contextlib.contextmanager
def wrapped_oracle():
    orig = orc._act

    def _act(x, act):
        if act == 'relu6':
            return orig(x, 'relu').clamp(max=6.0)
        if act == 'h-swish':
            return x * F.relu6(x + 3.0) / 6.0
        return orig(x, act)
    orc._act = _act
    try:
        yield
    finally:
        orc._act = orig


# ------------------------------------------------------------------------------------------------ oracle pin (blocks)
# activation x stride x SE x kernel size at the geometry of the 7 x 7 pin
PIN_GEOM = _k7.PIN_GEOM
PIN_CASES = [c for c in itertools.product(NEW_ACTS, (1, 2), (0, PIN_GEOM['se']), (3, 5))]
PIN_FORMS = ('search', 'derived')


def pin_tag(form, case):
    return '%s_%s_s%d_se%d_k%d' % ((form,) + tuple(case))


def pin_oracle_block(form, case):
    """The oracle's block of one pin case (float64; run it inside wrapped_oracle()), its input, cotangent and RNG seed.  The
    input is scaled by 3 so that BatchNorm outputs pass both kinks of either activation (the derived form's BatchNorms get
    gamma ~ 2)."""
    act, s, se, k = case
    q = PIN_GEOM
    seed = 3000 + 101 * PIN_CASES.index(case) + (0 if form == 'search' else 50)
    torch.manual_seed(seed)
    cls = orc.MBConv if form == 'search' else orc.DerivedBlock
    blk = cls(q['ic'], q['mc'], se, q['oc'], k, s, act)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))      # SE biases
    if form == 'derived':
        _k7.randomise_bn(blk, gen)
        with torch.no_grad():
            for m in (blk.inverted_bottleneck.bn, blk.depth_conv.bn):
                m.weight.mul_(2.5)
                m.bias.add_(1.0)
        blk.drop_connect_rate = _k7.PIN_DROP
    blk = blk.double().train()
    x = spiked_input((q['N'], q['ic'], q['H'], q['W']), gen).double()
    r = torch.randn(q['N'], q['oc'], (q['H'] - 1) // s + 1, (q['W'] - 1) // s + 1, generator=gen).double()
    return blk, x, r, seed + 2


# ------------------------------------------------------------------------------------------------ inputs and branches
def spiked_input(shape, gen, p=0.02, gain=11.0):
    """randn * (1 + gain * s), s ~ Bernoulli(p) per pixel and shared over channels: with plain randn input a batch-normalised
    pre-activation essentially never exceeds 6 and ReLU6 would be tested as ReLU."""
    N, C, H, W = shape
    x = torch.randn(N, C, H, W, generator=gen)
    s = (torch.rand(N, 1, H, W, generator=gen) < p).float()
    return x * (1.0 + gain * s)


def branch_fractions(z, act):
    """fractions of the pre-activations ``z`` below, between and above the two kinks of ``act``"""
    lo, hi = BRANCH_EDGES[act]
    z = z.detach()
    n = float(z.numel())
    return (float((z <= lo).sum()) / n, float(((z > lo) & (z < hi)).sum()) / n, float((z >= hi).sum()) / n)


def near_upper_kink(z, act, tau=2e-5):
    """number of pre-activations within ``tau`` of an upper kink (6 for ReLU6, -3 and 3 for hard-swish)"""
    z = z.detach()
    return sum(int(((z - k).abs() < tau).sum()) for k in UPPER_KINKS[act])


def assert_branches(zs, act, least, sites='all'):
    """every branch of ``act`` holds at least ``least`` of the pre-activations ``zs`` (a list of tensors, pooled), and none of
    them lies within 2e-5 of an upper kink.  sites='lower': the branch above the upper kink is not required (ReLU6 after BN2 of
    a search cell: the depthwise input is bounded by 6)."""
    z = torch.cat([t.detach().reshape(-1) for t in zs])
    fr = branch_fractions(z, act)
    need = fr[:2] if sites == 'lower' else fr
    assert min(need) >= least, (act, fr)
    assert near_upper_kink(z, act) == 0, (act, near_upper_kink(z, act))
    return fr


# ------------------------------------------------------------------------------------------------ cells
class _AnyLut(dict):
    """every key -> {mid: deterministic latency}"""

    def __init__(self, mids):
        super().__init__()
        self.mids = [int(m) for m in mids]

    def __missing__(self, key):
        v = self[key] = {m: 0.25 + 0.11 * i + 0.003 * (sum(map(ord, key)) % 97) for i, m in enumerate(self.mids)}
        return v


def make_oracle_cell(ic, oc, stride, act, mids, ks=None, seed=0, T=2.5):
    """The oracle's MixedOP (CPU) with activation ``act``, seeded weights, non-trivial SE biases and log_alphas and a synthetic
    LUT; ks: the candidates' kernel sizes (None: the search space's 3 / 3 / 5 / 5 / 3 / 3 / 5 / 5)."""
    torch.manual_seed(seed)
    mc = OrderedDict((i, int(m)) for i, m in enumerate(mids))
    o = orc.MixedOP(ic, oc, stride, act, mc, _AnyLut(mids))
    with torch.no_grad():
        for p in o.parameters():
            if p.dim() == 1 and p.numel() != 8:
                p.copy_(torch.randn(p.shape) * 0.1)
        o.log_alphas.copy_(torch.log_softmax(torch.randn(8) * 0.5, -1))
    if ks is not None:
        _k7.replace_oracle_ops(o, ks, seed)
    o.set_temperature(T)
    return o


def make_cell_pair(ic, oc, stride, act, mids, ks=None, seed=0):
    """(oracle MixedOP on the CPU, product MixedOP on cuda) with activation ``act`` and identical parameters"""
    o = make_oracle_cell(ic, oc, stride, act, mids, ks, seed)
    return o, _k7.hip_cell_like(o)


def compare_cell(o, m, x, r, e, idxs, need_wgrad, flip_tau=2e-5, least=1e-3):
    """_hipcheck.compare_cell for a cell with a new activation (that routine keys its ReLU replay on act_func == 'relu'): every
    tensor of every stage of groups ``idxs`` against the wrapped oracle, {name: (abs err, max |ref|)} for _hipcheck.worst.
    The HIP launch runs first; for ReLU6 its lower-kink decisions -- rebuilt from the E and D it saved (hip_relu_masks: E is
    always materialised on this route) -- are replayed in the oracle through RELU_HOOK, never exempted, and may differ from the
    oracle's own only within ``flip_tau`` of 0.  Asserted on the oracle's side: every branch of the activation holds at least
    ``least`` of the BN1 pre-activations (BN2: both branches below ReLU6's clamp, all three of hard-swish), none within 2e-5 of an
    upper kink."""
    from tfnas_amd import _lib
    from tfnas_amd.functions import MixedOpFn
    import ctypes as C
    act = o.m_ops[idxs[0]].act_func
    assert act in NEW_ACTS
    soft = len(idxs) > 1
    res = OrderedDict()
    w_o = None
    if soft:
        w_o = orc.gumbel_softmax(o.log_alphas, o.T, e)
        w_o.retain_grad()
    xm = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    plan = m._plan(tuple(idxs))
    params = plan.params()
    for p in params:
        p.requires_grad_(need_wgrad)
        p.grad = None
    w_m = w_o.detach().cuda().requires_grad_(True) if soft else None
    MixedOpFn.debug_sink, MixedOpFn.fwd_sink = [], []
    try:
        out_m = MixedOpFn.apply(plan, xm, w_m, *params)
        saved = out_m.grad_fn.saved_tensors        # xh, wmix, E, D, Pr, fsmall, stats, *params
        (out_m * r.cuda()).sum().backward()
        torch.cuda.synchronize()
        dbg, frec = MixedOpFn.debug_sink[0], MixedOpFn.fwd_sink[0]
    finally:
        MixedOpFn.debug_sink = MixedOpFn.fwd_sink = None
    d, ws = dbg['d'], dbg['ws']
    assert d.flags & _lib.CELL_ACTS
    assert not _lib.lib().tfnas_fx_supported(C.byref(d)) and not _lib.lib().tfnas_efree_supported(C.byref(d))
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    M, Ho, Wo = d.M, d.Ho, d.Wo
    assert saved[2] is not None                    # E is always materialised
    E = saved[2].view(N, H, W, M)
    D = saved[3].view(N, Ho, Wo, M)
    Pr = saved[4].view(len(idxs), N, Ho, Wo, m.out_channels)
    gate = saved[5][ws.off_gate:ws.off_gate + N * M].view(N, M)
    dZ = dbg['dZ'].view(N, Ho, Wo, M)
    dEh = dbg['dEh'].view(N, H, W, M)
    inj = None
    if act == 'relu6':
        frec['fx'] = False
        masks = []
        for gi, (m1, m2) in zip(idxs, hc.hip_relu_masks(frec)):
            masks += [m1, m2] + ([None] if o.m_ops[gi].se_channels else [])      # (SE hidden layer: the oracle's own)
        inj = hc.ReluInjector(masks)
    xo = x.clone().requires_grad_(True)
    details, ys = [], []
    orc.RELU_HOOK = inj
    try:
        with wrapped_oracle():
            for i in idxs:
                det = {}
                ys.append(o.m_ops[i](xo, det))
                for k in ('Eh', 'Z'):
                    det[k].retain_grad()
                details.append(det)
    finally:
        orc.RELU_HOOK = None
    if inj is not None:
        inj.done()
        res['relu_flips'] = (0.0, float(inj.flips))                       # informational (never "worst")
        res['relu_flip_max_abs'] = (max(0.0, inj.max_abs_at_flip - flip_tau), 0.0)   # > 0 -> a flip far from the kink: worst()
    res['_branches1'] = assert_branches([det['Eh'] for det in details], act, least)
    res['_branches2'] = assert_branches([det['Dh'] for det in details], act, least, 'lower' if act == 'relu6' else 'all')
    out_o = sum(w_o[i] * y for i, y in zip(idxs, ys)) if soft else ys[0]
    (out_o * r).sum().backward()
    for g, (i, det) in enumerate(zip(idxs, details)):
        off, mc = d.g[g].off, d.g[g].mc
        tag = 'g%d.' % i
        res[tag + 'E'] = hc.err(E[..., off:off + mc], hc.nhwc(det['E']))
        res[tag + 'D'] = hc.err(D[..., off:off + mc], hc.nhwc(det['D']))
        if 'gate' in det:
            res[tag + 'gate'] = hc.err(gate[:, off:off + mc], det['gate'].flatten(1))
        res[tag + 'Pr'] = hc.err(Pr[g], hc.nhwc(det['P']))
        res[tag + 'dZ'] = hc.err(dZ[..., off:off + mc], hc.nhwc(det['Z'].grad))
        res[tag + 'dEh'] = hc.err(dEh[..., off:off + mc], hc.nhwc(det['Eh'].grad))
    res['out'] = hc.err(out_m, out_o)
    res['dx'] = hc.err(xm.grad, xo.grad)
    if soft:
        res['dwmix'] = hc.err(w_m.grad, w_o.grad)
    if need_wgrad:
        k = 0
        for i in idxs:
            names = ['expand', 'dw', 'proj'] + (['se_rw', 'se_rb', 'se_ew', 'se_eb'] if o.m_ops[i].se_channels else [])
            op = o.m_ops[i].params()
            for nme in names:
                res['g%d.grad_%s' % (i, nme)] = hc.err(params[k].grad, op[nme].grad)
                k += 1
    for p in params:
        p.grad = None
    o.zero_grad()
    return res


def check_cell(o, m, x, r, e, idxs, need_wgrad):
    """compare_cell + the project's standing gate on every tensor: abs err <= 2e-5 + 1e-4 * max|ref| (_hipcheck.worst)"""
    res = compare_cell(o, m, x, r, e, idxs, need_wgrad)
    bad = hc.worst(res)
    assert not bad, bad
    return res


# ------------------------------------------------------------------------------------------------ derived blocks
def strong_bn(blk, gen):
    """BN1 and BN2 of a derived block with gamma ~ 3 (some entries negative) and beta ~ 2, so that the affine output passes both
    kinks of either activation at both sites; non-trivial running statistics everywhere."""
    _k7.randomise_bn(blk, gen)
    with torch.no_grad():
        for m in (blk.inverted_bottleneck.bn, blk.depth_conv.bn):
            m.weight.copy_(3.0 + 0.3 * torch.randn(m.weight.shape, generator=gen))
            m.weight[::5].neg_()
            m.bias.copy_(2.0 + 0.2 * torch.randn(m.bias.shape, generator=gen))


def derived_preacts(o, x):
    """the affine BN1 / BN2 outputs of the oracle's DerivedBlock ``o`` on ``x`` in its current mode, without moving its running
    statistics"""
    import copy
    c = copy.deepcopy(o)
    with torch.no_grad(), wrapped_oracle():
        z1 = c.inverted_bottleneck.bn(c.inverted_bottleneck.conv(x))
        z2 = c.depth_conv.bn(c.depth_conv.conv(orc._act(z1, c.act_func)))
    return z1, z2


def act_network_config(num_classes=50):
    """A ``model.config`` (parsing.derived_config: two blocks per stage, SE and plain candidates) whose blocks name 'relu6' and
    'h-swish' in turn."""
    from tfnas_amd import geometry as g, parsing
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 2))
                       for i, (st, bl) in enumerate(g.initial_mc_num_dddict().items()))
    cfg = parsing.derived_config(arch, g.initial_mc_num_dddict(), num_classes)
    n = 0
    for i in range(1, 7):
        for blk in cfg['stage%d' % i]:
            blk['act_func'] = NEW_ACTS[n % 2]
            n += 1
    return cfg, arch, g.initial_mc_num_dddict()
