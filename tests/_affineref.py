"""The float64 reference of the derived-network ("retrain") path's affine blocks and head, shared by tests/test_affine_refs.py
(CPU: what makes the reference and its gates meaningful) and tests/test_gpu_affine_f64.py (the HIP kernels at the C ABI).

The reference is the project's own oracle run in float64 -- ``copy.deepcopy(orc.DerivedBlock(...)).double()``; for the head
``orc._ConvBN(ic, mc, 1, 1, act)`` followed by ``adaptive_avg_pool2d``, and for the search-form head the same convolution under
``F.batch_norm`` without weight or bias on batch statistics.  The oracle is pinned to the reference implementation's
model_eval.py by tests/test_oracle_vs_reference.py.

Every case is built from ``torch.Generator`` seeds alone.  BatchNorm parameters are those of ``_randomise`` in
tests/test_gpu_derived.py with four edge channels on top (EDGES), running statistics off their defaults, momentum 0.01 and inputs
with a per-channel mean.  |beta / gamma| <= 10 on every channel: the affine fold (csrc/bn_affine.hip) loses a factor |beta / gamma|
of fp32 precision by construction, 10 costs under 1e-5 relative -- an order below the gate -- so any correct implementation passes.

Gates: ``gate(ref) = 2e-5 + 1e-4 max|ref|`` per tensor (tests/_hipcheck.worst: the cell gate) and, for running statistics,
``1e-6 + 1e-5 |ref|`` elementwise (one fp32 multiply-add on values good to ~1e-7; a missing unbiased-variance correction moves
running_var by momentum * var / (cnt - 1): 2.3e-4 var at momentum 0.01 and the smallest head's cnt = 45, 1.4e-4 var at block D's
cnt = 70)."""
import copy
import functools
from collections import OrderedDict

import torch
import torch.nn.functional as F

import tfnas_oracle as orc
from _rawcell import KINK_TAU

# (ic, mc, se, oc, k, stride, act, N, H, W)
BLOCKS = OrderedDict([
    ('A', (24, 72, 24, 24, 3, 1, 'swish', 3, 9, 11)),      # residual, SE, ragged image
    ('B', (40, 131, 0, 80, 5, 2, 'swish', 2, 13, 9)),      # mc % 4 != 0, stride 2, no SE
    ('C', (32, 96, 32, 32, 5, 1, 'swish', 5, 7, 7)),       # residual: drop-connect and eval
    ('D', (16, 48, 16, 16, 3, 1, 'relu', 2, 5, 7)),        # ReLU: kink-clear seed
])
# (ic, mc, N, H, W), all swish
HEADS = [(320, 1280, 5, 3, 3), (320, 1280, 3, 7, 7), (64, 192, 2, 5, 9)]
# (gamma, beta) of channels 0..3 of every BatchNorm; None: as _randomise left it
EDGES = ((-0.7, None), (0.05, 0.5), (-0.05, 0.5), (2.5, -1.5))
MAX_BETA_OVER_GAMMA = 10.0
MOMENTUM = 0.01
KEEP = 0.6                                                 # drop-connect keep probability (rate 0.4)
DROP_U = (0.05, 0.95, 0.5, 0.61, 0.3)                      # floor(KEEP + u): dropped, kept, kept, kept, dropped
DROP_U_ALL = 0.1                                           # every image dropped
BLOCK_CASES = [('A', 'train'), ('B', 'train'), ('C', 'train'), ('D', 'train'), ('C', 'drop'), ('C', 'alldrop'),
               ('A', 'eval'), ('B', 'eval'), ('C', 'eval'), ('D', 'eval')]
HEAD_CASES = [(i, form) for i in range(len(HEADS)) for form in ('search', 'train', 'eval')]


def gate(ref):
    return 2e-5 + 1e-4 * float(ref.abs().max())


def ratio(got, ref):
    """max|got - ref| / gate(ref)"""
    return float((got.detach().cpu().double() - ref.double()).abs().max()) / gate(ref)


def running_ratio(got, ref):
    """max over elements of |got - ref| / (1e-6 + 1e-5 |ref|)"""
    ref = ref.double()
    return float(((got.detach().cpu().double() - ref).abs() / (1e-6 + 1e-5 * ref.abs())).max())


def is_running(key):
    return key.startswith('b.')


def compare(got, ref, scale=1.0):
    """{key: err / gate} over every tensor of ``ref`` (keys with '_' in front are not tensors to compare): running statistics
    ('b.*') under the elementwise gate, everything else under gate(); scale < 1 tightens both."""
    out = OrderedDict()
    for k, want in ref.items():
        if k.startswith('_'):
            continue
        assert got[k].shape == want.shape, (k, tuple(got[k].shape), tuple(want.shape))
        out[k] = (running_ratio if is_running(k) else ratio)(got[k], want) / scale
    return out


def classes(ratios):
    """worst err / gate per tensor class: y, dx, conv / SE gradients, BatchNorm gradients, running statistics"""
    out = OrderedDict()
    for k, v in ratios.items():
        c = ('running' if is_running(k) else 'g_bn' if (k.startswith('g.') and '.bn.' in k) else 'g_conv' if k.startswith('g.')
             else k)
        out[c] = max(out.get(c, 0.0), v)
    return out


# ---------------------------------------------------------------------------------------------------------------- builders
def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def randomise(mod, gen):
    """Every parameter and buffer of ``mod`` from ``gen``: convolutions ~ N(0, 1 / fan_in), their biases ~ 0.1 N(0, 1); BatchNorms
    as tests/test_gpu_derived._randomise, then EDGES on channels 0..3, momentum MOMENTUM."""
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan_in = m.weight[0].numel()
                m.weight.copy_(_randn(gen, *m.weight.shape) * fan_in ** -0.5)
                if m.bias is not None:
                    m.bias.copy_(0.1 * _randn(gen, *m.bias.shape))
            elif isinstance(m, torch.nn.BatchNorm2d):
                n = m.weight.numel()
                m.weight.copy_(1.0 + 0.3 * _randn(gen, n))
                m.bias.copy_(0.2 * _randn(gen, n))
                m.running_mean.copy_(0.1 * _randn(gen, n))
                m.running_var.copy_(1.0 + 0.2 * torch.rand(n, generator=gen))
                for c, (g, b) in enumerate(EDGES):
                    m.weight[c] = g
                    if b is not None:
                        m.bias[c] = b
                m.momentum = MOMENTUM


def batchnorms(mod):
    return [m for m in mod.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def worst_beta_over_gamma(mod):
    return max(float((m.bias.detach().double() / m.weight.detach().double()).abs().max()) for m in batchnorms(mod))


def conditioned(mod):
    """|beta / gamma| <= 10 on every channel (the edge channels sit AT 10 up to the rounding of 0.05 to fp32)"""
    return worst_beta_over_gamma(mod) <= MAX_BETA_OVER_GAMMA * (1.0 + 1e-6)


def inputs(gen, N, ic, H, W, out_shape):
    """x with a per-channel mean (retrain-path activations are not zero-mean) and the upstream gradient r"""
    x = _randn(gen, N, ic, H, W) + 2.0 * _randn(gen, 1, ic, 1, 1)
    return x, _randn(gen, *out_shape)


class _Taps:
    """What the BatchNorms of one oracle run saw: per site the statistics it normalised with (mean, biased variance; in eval
    mode the running ones) and the smallest |output| (kink distance of the activation that follows)."""

    def __init__(self, mod, extra=()):
        self.sites, self.kink, self.pre_kink = [], [], []
        self._h = [m.register_forward_hook(self._bn) for m in batchnorms(mod)]
        self._h += [m.register_forward_hook(self._pre) for m in extra]

    def _bn(self, m, inp, out):
        v = inp[0].detach()
        if m.training:
            mean, var = v.mean((0, 2, 3)), v.var((0, 2, 3), unbiased=False)
        else:
            mean, var = m.running_mean.detach().clone(), m.running_var.detach().clone()
        self.sites.append(dict(mean=mean, var=var, gamma=m.weight.detach().clone(), beta=m.bias.detach().clone(), eps=m.eps))
        self.kink.append(float(out.detach().abs().min()))

    def _pre(self, m, inp, out):
        self.pre_kink.append(float(out.detach().abs().min()))

    def close(self):
        for h in self._h:
            h.remove()


def run_block(o, x, r, mode='train', u=None):
    """One forward + backward of ``o`` (loss = sum(y * r)); ``o`` is used up (its running statistics move).  Returns y, dx, 'g.<name>'
    of every parameter, 'b.<name>' of every running buffer, and '_taps'."""
    o.train(mode != 'eval')
    o.drop_connect_rate, o.drop_u = 0.0, None
    if u is not None:
        o.drop_connect_rate, o.drop_u = 1.0 - KEEP, u.to(x.dtype)
    # (the activations that follow a BatchNorm: sites 0 and 1; the SE hidden layer's follows conv_reduce)
    taps = _Taps(o, extra=[o.squeeze_excite.conv_reduce] if o.squeeze_excite is not None else [])
    x = x.clone().requires_grad_(True)
    y = o(x)
    (y * r).sum().backward()
    taps.close()
    out = OrderedDict(y=y.detach(), dx=x.grad)
    for k, p in o.named_parameters():
        out['g.' + k] = p.grad
    for k, b in o.named_buffers():
        if 'running' in k:
            out['b.' + k] = b.detach().clone()
    out['_taps'] = taps
    return out


def kink_clear(taps, act, n_bn_act):
    """no pre-activation of a ReLU (the first ``n_bn_act`` BatchNorm outputs and the SE hidden layer) within KINK_TAU of 0"""
    if act != 'relu':
        return True
    return min(taps.kink[:n_bn_act] + taps.pre_kink) >= KINK_TAU


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def drop_u(mode, N):
    if mode == 'drop':
        assert N == len(DROP_U)
        return torch.tensor(DROP_U)
    if mode == 'alldrop':
        return torch.full((N,), DROP_U_ALL)
    return None


def _build_block(shape, mode, seed):
    ic, mc, se, oc, k, s, act, N, H, W = BLOCKS[shape]
    gen = torch.Generator().manual_seed(seed)
    o = orc.DerivedBlock(ic, mc, se, oc, k, s, act)
    randomise(o, gen)
    x, r = inputs(gen, N, ic, H, W, (N, oc, (H - 1) // s + 1, (W - 1) // s + 1))
    return Case(name='%s-%s' % (shape, mode), shape=shape, geom=BLOCKS[shape], mode=mode, seed=seed, o=o, x=x, r=r, u=drop_u(mode, N))


def reference(case, dtype=torch.float64, x=None, r=None, u=None, edit=None):
    """The oracle in ``dtype`` on the case (optionally on other inputs, or after ``edit(module)``)."""
    o = copy.deepcopy(case.o).to(dtype)
    if edit is not None:
        with torch.no_grad():
            edit(o)
    x = case.x if x is None else x
    r = case.r if r is None else r
    u = case.u if u is None else u
    return run_block(o, x.to(dtype), r.to(dtype), case.mode, None if u is None else u.to(dtype))


def plain_site1(o):
    """BatchNorm site 1 without affine part (TfnasBnAffine.weight[1] = bias[1] = NULL): gamma 1, beta 0"""
    o.depth_conv.bn.weight.fill_(1.0)
    o.depth_conv.bn.bias.fill_(0.0)


def unit_running(o):
    """no running statistics in eval mode (TfnasBnAffine.running_* = NULL): mean 0, variance 1"""
    for m in batchnorms(o):
        m.running_mean.fill_(0.0)
        m.running_var.fill_(1.0)


def doubled(case):
    """two ranks with identical shards: the global batch"""
    return dict(x=torch.cat([case.x, case.x]), r=torch.cat([case.r, case.r]))


# the variants of a case the GPU tests compare against, beyond the case's own ``ref``: (shape, mode, name) -> keyword arguments
VARIANTS = OrderedDict([
    (('A', 'train', 'plain_site1'), lambda c: dict(edit=plain_site1)),
    (('A', 'eval', 'unit_running'), lambda c: dict(edit=unit_running)),
    (('D', 'train', 'doubled'), doubled),
])


@functools.lru_cache(maxsize=None)
def block_case(shape, mode):
    """The case of BLOCKS[shape] in ``mode`` (train | drop | alldrop | eval) with its float64 reference ``ref``: the first seed
    0, 1, 2, ... whose parameters are conditioned and -- ReLU -- whose float64 run is kink-clear."""
    for seed in range(64):
        case = _build_block(shape, mode, seed)
        if not conditioned(case.o):
            continue
        case.ref = reference(case)
        if kink_clear(case.ref['_taps'], case.geom[6], 2):
            return case
    raise AssertionError('no qualifying seed for %s / %s' % (shape, mode))


@functools.lru_cache(maxsize=None)
def variant_ref(shape, mode, name):
    case = block_case(shape, mode)
    return reference(case, **VARIANTS[(shape, mode, name)](case))


# ---------------------------------------------------------------------------------------------------------------- the head
def head_forward(cb, x, affine=True):
    """feature-mix layer + global average pool: ``cb`` an orc._ConvBN; affine=False: the search form (BatchNorm on batch
    statistics, no weight, no bias, no running statistics)."""
    if affine:
        y = cb(x)
    else:
        y = orc._act(F.batch_norm(cb.conv(x), None, None, None, None, True, 0.0, cb.bn.eps), cb.act)
    return F.adaptive_avg_pool2d(y, 1).flatten(1)


def run_head(cb, x, r, form):
    """form: search | train | eval.  Returns pooled, dx, g.conv.weight and, in the affine forms, g.bn.weight / g.bn.bias and the
    running buffers."""
    cb.train(form != 'eval')
    taps = _Taps(cb)
    x = x.clone().requires_grad_(True)
    pooled = head_forward(cb, x, form != 'search')
    (pooled * r).sum().backward()
    taps.close()
    out = OrderedDict(pooled=pooled.detach(), dx=x.grad)
    out['g.conv.weight'] = cb.conv.weight.grad
    if form != 'search':
        out['g.bn.weight'], out['g.bn.bias'] = cb.bn.weight.grad, cb.bn.bias.grad
        out['b.bn.running_mean'], out['b.bn.running_var'] = cb.bn.running_mean.detach().clone(), cb.bn.running_var.detach().clone()
    out['_taps'] = taps
    return out


@functools.lru_cache(maxsize=None)
def head_case(idx, form):
    ic, mc, N, H, W = HEADS[idx]
    for seed in range(64):
        gen = torch.Generator().manual_seed(seed)
        cb = orc._ConvBN(ic, mc, 1, 1, 'swish')
        randomise(cb, gen)
        if conditioned(cb):
            break
    else:
        raise AssertionError('no conditioned seed for head %d' % idx)
    x, r = inputs(gen, N, ic, H, W, (N, mc))
    case = Case(name='head%d-%s' % (idx, form), geom=HEADS[idx], form=form, seed=seed, o=cb, x=x, r=r)
    case.ref = head_reference(case)
    return case


def head_reference(case, dtype=torch.float64):
    return run_head(copy.deepcopy(case.o).to(dtype), case.x.to(dtype), case.r.to(dtype), case.form)


# ---------------------------------------------------------------------------------------------------------------- tables
def probe_ratio(m_eff, r_eff, site):
    """The statistics table of one BatchNorm site after k_bn_fwd_fix, (m_eff, r_eff) per channel, against the float64 oracle's
    site record (_Taps.sites[i]).  m_eff is legitimately huge where r_eff is small, so the MAP the pair defines is compared, not
    the raw numbers: y(v) = (v - m_eff) r_eff at v = mu64 +- sigma64 against gamma (v - mu) / sqrt(var + eps) + beta, under gate()."""
    mu, var = site['mean'].double(), site['var'].double()
    sig = var.sqrt()
    m_eff, r_eff = m_eff.detach().cpu().double(), r_eff.detach().cpu().double()
    got, want = [], []
    for v in (mu - sig, mu + sig):
        got.append((v - m_eff) * r_eff)
        want.append(site['gamma'].double() * (v - mu) / (var + site['eps']).sqrt() + site['beta'].double())
    return ratio(torch.stack(got), torch.stack(want))
