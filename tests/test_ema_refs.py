"""CPU: the float64 restatement of the weight EMA (tests/_emaref.py) against torch.lerp and the textbook form; the warm-up
schedule; model_eval.WeightEma on a CPU derived network (the ``torch._foreach_lerp_`` route: no arena, no launch); the host-side
refusals of tfnas_sgd_clip_ema_step / tfnas_ema_lerp; and run_retrain's checkpoint keys with and without an EMA.

Bound of the torch route.  torch's fp32 lerp evaluates ``e + a (w - e)`` for a < 0.5 and ``w - (w - e)(1 - a)`` otherwise; the second
form rounds 1 - a and carries the difference at full size, so its error is not scaled by a: per update
4 * 2^-24 * (|e'| + |w - e|) covers both (difference, 1 - a, product, sum: four roundings, each of a term no larger than that sum).
Errors of earlier updates only shrink (factor 1 - a), so the bounds of the updates add up."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _emaref as er
import _smallref as sr

EINVAL, ENULL, ERANGE = -1, -2, -3


def test_restatement_is_torch_lerp_and_the_textbook_form_in_float64():
    g = torch.Generator().manual_seed(7)
    e = torch.randn(4096, generator=g, dtype=torch.float64)
    w = e + torch.randn(4096, generator=g, dtype=torch.float64) * torch.logspace(-8, 1, 4096, dtype=torch.float64)
    for alpha in (1e-4, 0.1, 0.4736842105263158, 0.9, 1.0, 0.0):
        ref = er.lerp_ref(e, w, alpha)
        scale = np.abs(sr.d64(e)) + np.abs(sr.d64(w))
        assert np.all(np.abs(ref - torch.lerp(e, w, alpha).numpy()) <= 4 * 2.0 ** -53 * scale)
        decay = 1.0 - alpha
        book = decay * sr.d64(e) + (1.0 - decay) * sr.d64(w)
        assert np.all(np.abs(ref - book) <= 1e-15 * scale)
    assert np.array_equal(er.lerp_ref(e, w, 0.0), sr.d64(e))
    # sgd_ema_ref: the SGD part is _smallref's, the EMA moves towards the NEW weights, only inside the ranges
    w32, g32, m32, e32 = (torch.randn(64, generator=g) for _ in range(4))
    ranges = [(8, 16), (40, 4)]
    w2, g2, m2, tot, e2 = er.sgd_ema_ref(w32, g32, m32, e32, ranges, None, 5.0, 0.05, 0.9, 1e-5, 1.0, 0.25)
    ws, gs, ms, ts = sr.sgd_clip_ref(w32, g32, m32, ranges, None, 5.0, 0.05, 0.9, 1e-5, 1.0)
    assert np.array_equal(w2, ws) and np.array_equal(g2, gs) and np.array_equal(m2, ms) and tot == ts
    inside = np.zeros(64, dtype=bool)
    for o, n in ranges:
        inside[o:o + n] = True
    assert np.array_equal(e2[~inside], sr.d64(e32)[~inside])
    assert np.array_equal(e2[inside], (sr.d64(e32) + 0.25 * (w2 - sr.d64(e32)))[inside])


def test_warmup_schedule():
    from tfnas_amd import model_eval as me
    assert er.alpha_ref(0, 0.9999) == 0.9
    assert er.alpha_ref(9, 0.9999) == 1 - 10 / 19
    assert er.alpha_ref(0, 0.9999, warmup=False) == er.alpha_ref(10 ** 6, 0.9999, warmup=False) == 1 - 0.9999
    for decay in (0.9, 0.999, 0.9999):
        first = next(t for t in range(10 ** 6) if (1.0 + t) / (10.0 + t) >= decay)
        assert first > 0 and er.alpha_ref(first - 1, decay) > 1 - decay
        for t in (first, first + 1, first + 7, 10 * first, 10 ** 7):
            assert er.alpha_ref(t, decay) == 1 - decay                    # exactly, from there on
        prev = 1.0
        for t in range(first + 2):                                        # never increasing on the way
            assert er.alpha_ref(t, decay) <= prev
            prev = er.alpha_ref(t, decay)

    class _M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(3))
    for decay, warm in ((0.9999, True), (0.9, True), (0.9, False)):
        e = me.WeightEma(_M(), decay, warm)
        for t in (0, 1, 9, 80, 81, 100000):
            assert e.alpha(t) == er.alpha_ref(t, decay, warm)
        assert e.alpha() == e.alpha(0)
    with pytest.raises(ValueError):
        me.WeightEma(_M(), 1.5)


def _arch():
    from tfnas_amd import geometry as g
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 2))
                       for i, (st, bl) in enumerate(g.initial_mc_num_dddict().items()))
    return arch, g.initial_mc_num_dddict()


def _net(seed, classes=10):
    from tfnas_amd import model_eval as me
    arch, mc = _arch()
    torch.manual_seed(seed)
    m = me.Network(classes, arch, mc, None, 0.0, 0.0)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=gen))
                mod.running_var.copy_(1.0 + 0.2 * torch.rand(mod.running_var.shape, generator=gen))
    return m


def _perturb(m, gen, step):
    """What a training step leaves behind, without one: every parameter and running statistic moves, the batch counters count."""
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen))
        for k, b in m.named_buffers():
            if b.is_floating_point():
                b.mul_(0.9).add_(0.1 * torch.rand(b.shape, generator=gen))
            else:
                b.fill_(step)


@pytest.mark.parametrize('warmup', [True, False])
def test_weight_ema_on_a_cpu_network_follows_the_restatement(warmup):
    from tfnas_amd import model_eval as me
    m = _net(3)
    ema = me.WeightEma(m, 0.9, warmup)
    assert ema.updates == 0
    sd0 = ema.state_dict()
    assert list(sd0.keys()) == list(m.state_dict().keys())
    for k, v in m.state_dict().items():
        assert torch.equal(sd0[k], v) and sd0[k].data_ptr() != v.data_ptr()           # starts as a copy
    ref = {k: sr.d64(v) for k, v in m.state_dict().items()}
    lim = {k: np.zeros(v.shape) for k, v in ref.items()}
    gen = torch.Generator().manual_seed(9)
    worst = 0.0
    for t in range(3):
        _perturb(m, gen, t + 1)
        alpha = er.alpha_ref(t, 0.9, warmup)
        assert ema.alpha() == alpha
        ema.update(m)
        assert ema.updates == t + 1
        got = ema.state_dict()
        for k, v in m.state_dict().items():
            if not v.is_floating_point():
                assert torch.equal(got[k], v) and int(got[k]) == t + 1                 # integer buffers: copied, not averaged
                continue
            new = er.lerp_ref(ref[k], v, alpha)
            lim[k] = lim[k] + 4 * er.U * (np.abs(new) + np.abs(sr.d64(v) - ref[k]))
            ref[k] = new
            err = np.abs(sr.d64(got[k]) - new)
            assert np.all(err <= lim[k]), (k, t, float(err.max()))
            nz = lim[k] > 0
            if nz.any():
                worst = max(worst, float((err[nz] / lim[k][nz]).max()))
    print('WeightEma cpu warmup=%s: worst error / bound %.3f' % (warmup, worst))
    assert worst > 0.0                                                                  # (the EMA did move)


def test_state_dict_round_trip_copy_to_and_swapped():
    import io
    from tfnas_amd import model_eval as me
    m = _net(5)
    ema = me.WeightEma(m, 0.9)
    gen = torch.Generator().manual_seed(2)
    for t in range(2):
        _perturb(m, gen, t + 1)
        ema.update(m)
    sd = ema.state_dict()
    assert list(sd.keys()) == list(m.state_dict().keys())
    assert any(not torch.equal(sd[k], v) for k, v in m.state_dict().items())
    # straight into a fresh NetworkCfg, strict: no tensor key was added for the count ...
    m2 = me.NetworkCfg(10, m.config)
    res = m2.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k])
    # ... which survives torch.save / torch.load and comes back through load_state_dict
    assert me.WeightEma.COUNT_KEY not in set(m.state_dict()._metadata)
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    back = torch.load(f, weights_only=False)
    e2 = me.WeightEma(m2, 0.9)
    assert e2.updates == 0
    e2.load_state_dict(back)
    assert e2.updates == 2 and e2.alpha() == ema.alpha()
    for k, v in e2.state_dict().items():
        assert torch.equal(v, sd[k])
    e2.load_state_dict({k: v for k, v in sd.items()}, updates=7)                       # a plain dict + the count beside it
    assert e2.updates == 7
    with pytest.raises(KeyError):
        e2.load_state_dict({k: v for k, v in list(sd.items())[1:]})
    # swapped: the model holds the average inside and is restored bit for bit -- also when the body raises
    live = {k: v.clone() for k, v in m.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in m.state_dict().items()}
    with ema.swapped(m) as inner:
        assert inner is m
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k])
    with pytest.raises(ZeroDivisionError):
        with ema.swapped(m):
            assert torch.equal(next(iter(m.state_dict().values())), next(iter(sd.values())))
            1 / 0
    for k, v in m.state_dict().items():
        assert torch.equal(v, live[k]) and v.data_ptr() == ptrs[k], k
    for k, v in ema.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # copy_to
    m3 = _net(11)
    me.WeightEma(m3, 0.5).copy_to(m3)                                                   # (its own copy: a no-op)
    ema.copy_to(m)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k])


def test_ema_entry_points_refuse_on_the_host():
    """As test_capi_symbols.py::test_error_codes: every refusal comes before any launch, so no GPU (and no real buffer) is needed."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    w, g, m, e, sc = (C.c_void_p(4096 * (i + 1)) for i in range(5))
    u64 = lambda v: (C.c_uint64 * len(v))(*v)
    good = ([64, 512, 1024], [64, 128, 512])

    def step(ema=e, alpha=0.1, off=good[0], ln=good[1], nr=None, ww=w, gg=g, mm=m):
        return lib.tfnas_sgd_clip_ema_step(ww, gg, mm, len(off) if nr is None else nr, u64(off), None, u64(ln), 5.0, 0.025, 0.9,
                                           1e-5, 1.0, ema, alpha, sc, 8, None, None)

    def lerp(ema=e, src=w, alpha=0.1, off=good[0], ln=good[1], nr=None):
        return lib.tfnas_ema_lerp(ema, src, len(off) if nr is None else nr, u64(off), u64(ln), alpha, None)

    assert step(ema=None) == ENULL and lerp(ema=None) == ENULL and lerp(src=None) == ENULL
    assert step(ww=None) == ENULL and step(gg=None) == ENULL and step(mm=None) == ENULL
    for bad in (-0.1, 1.5, float('nan'), float('inf'), -float('inf')):
        assert step(alpha=bad) == EINVAL, bad
        assert lerp(alpha=bad) == EINVAL, bad
    assert step(off=[64, 100, 1024]) == EINVAL and lerp(off=[64, 100, 1024]) == EINVAL           # [64,128) and [100,228) overlap
    assert step(off=[64, 512, 512]) == EINVAL and lerp(off=[64, 512, 512]) == EINVAL             # the same range twice
    assert step(ema=w) == EINVAL and step(ema=g) == EINVAL and step(ema=m) == EINVAL             # aliasing
    assert lerp(ema=w, src=w) == EINVAL
    assert step(off=[64, 514, 1024]) == EINVAL and lerp(off=[64, 514, 1024]) == EINVAL           # what fill_ranges refuses: alignment,
    assert step(ln=[64, 0, 512]) == EINVAL and lerp(ln=[64, 126, 512]) == EINVAL                 # empty / ragged lengths,
    assert step(nr=0) == ERANGE and lerp(nr=0) == ERANGE                                         # the range count
    many = ([4 * i for i in range(65)], [4] * 65)
    assert step(off=many[0], ln=many[1]) == ERANGE and lerp(off=many[0], ln=many[1]) == ERANGE
    assert lib.tfnas_sgd_clip_ema_step(w, g, m, 1, u64([0]), None, u64([8192 + 4]), 5.0, 0.025, 0.9, 1e-5, 1.0, e, 0.1, sc, 1,
                                       None, None) == ERANGE                                     # scratch one double short


def test_run_retrain_checkpoint_keys_with_and_without_an_ema(tmp_path):
    """On the CPU nothing can be fused and no batch can run (the blocks have no CPU implementation): empty queues, one epoch --
    what is pinned here is what the checkpoint holds.  ema_decay=None: exactly the reference's five keys."""
    from tfnas_amd import model_eval as me
    m = _net(2)
    h = me.run_retrain(str(tmp_path / 'a'), m, lambda e: [], lambda e: [], epochs=1, lr=0.1, device='cpu', log=lambda s: None)
    ck = torch.load(tmp_path / 'a' / 'checkpoint.pth.tar', weights_only=False)
    assert set(ck) == {'epoch', 'state_dict', 'best_acc_top1', 'best_acc_top5', 'optimizer'}
    assert set(h[0]) == {'epoch', 'lr', 'train_acc', 'train_obj', 'val_top1', 'val_top5', 'val_obj'}
    lines = []
    h = me.run_retrain(str(tmp_path / 'b'), m, lambda e: [], lambda e: [], epochs=1, lr=0.1, device='cpu', log=lines.append,
                       ema_decay=0.9)
    ck = torch.load(tmp_path / 'b' / 'checkpoint.pth.tar', weights_only=False)
    assert set(ck) == {'epoch', 'state_dict', 'best_acc_top1', 'best_acc_top5', 'optimizer', 'state_dict_ema', 'ema_updates'}
    assert ck['ema_updates'] == 0 and list(ck['state_dict_ema']) == list(ck['state_dict'])
    assert all(k.startswith('module.') for k in ck['state_dict_ema'])
    for k, v in ck['state_dict'].items():
        assert torch.equal(ck['state_dict_ema'][k], v)                                  # no update yet: still the copy
    assert {'val_top1_ema', 'val_top5_ema', 'val_obj_ema'} <= set(h[0]) and 'ema_top1' in lines[0]
