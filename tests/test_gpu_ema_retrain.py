"""GPU, end to end: model_eval.WeightEma through train_step / validate / run_retrain on the derived network of
test_gpu_derived.py::_arch (8 x 3 x 64 x 64 inputs, drop rates 0, three steps, lr 0.05, decay 0.9, warm-up both ways).

(a) attaching an EMA changes no bit of the training itself; (b) the EMA is the float64 recurrence (tests/_emaref.py) over the
per-step snapshots of weights and buffers, within _emaref.lerp_bound summed over the steps (an earlier step's error only shrinks,
by 1 - alpha); (c) the gaps of the flat shadows are zero; (d) fused route and torch route + ``update`` agree as closely as their
weights do; (e) ``validate(..., ema=)`` is ``validate`` of a fresh network loaded from ``ema.state_dict()`` and restores the model;
(f) the EMA survives a rebuilt arena; (g) run_retrain: history, best checkpoint, bit-identical resume, resume of an EMA-less
snapshot."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _emaref as er
import _smallref as sr

pytestmark = pytest.mark.gpu

STEPS, LR, DECAY, CLASSES = 3, 0.05, 0.9, 10


def _arch():
    from tfnas_amd import geometry as g
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 2))
                       for i, (st, bl) in enumerate(g.initial_mc_num_dddict().items()))
    return arch, g.initial_mc_num_dddict()


def _model(seed=5):
    from tfnas_amd import model_eval as me
    arch, mc = _arch()
    torch.manual_seed(seed)
    return me.Network(CLASSES, arch, mc, None, 0.0, 0.0)


def _batches(n, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(8, 3, 64, 64, generator=gen), torch.randint(0, CLASSES, (8,), generator=gen)) for _ in range(n)]


def _cpu(sd):
    return OrderedDict((k, v.detach().cpu().clone()) for k, v in sd.items())


_runs = {}


def _run(warmup, fused=True, roundtrip=False):
    """Three training steps; ``warmup`` None: no EMA.  Returns per-step CPU snapshots (computed once per configuration)."""
    key = (warmup, fused, roundtrip)
    if key in _runs:
        return _runs[key]
    from tfnas_amd import model_eval as me
    m = _model().cuda()
    opt = torch.optim.SGD(m.parameters(), LR, momentum=0.9, weight_decay=4e-5)
    crit = me.CrossEntropyLabelSmooth(CLASSES, 0.1)
    ema = None if warmup is None else me.WeightEma(m, DECAY, warmup)
    out = dict(model=m, ema=ema, opt=opt, init=_cpu(m.state_dict()), snaps=[], emas=[], losses=[], arenas=[])
    for t, (x, y) in enumerate(_batches(STEPS)):
        if roundtrip and t == 1:
            before = _cpu(ema.state_dict())
            m.to('cpu').to('cuda')
            out['kept'] = (before, _cpu(ema.state_dict()))
        loss, _ = me.train_step(m, x.cuda(), y.cuda(), crit, opt, 5.0, fused=fused, ema=ema)
        torch.cuda.synchronize()
        out['losses'].append(loss.cpu().clone())
        out['snaps'].append(_cpu(m.state_dict()))
        out['arenas'].append(getattr(m, '_retrain_state', None))
        if ema is not None:
            out['emas'].append(_cpu(ema.state_dict()))
            assert ema.updates == t + 1
    out['mom'] = [opt.state[p]['momentum_buffer'].detach().cpu().clone() for p in m.parameters()]
    _runs[key] = out
    return out


def _recurrence(init, snaps, warmup):
    """[(ref, bound)] per step: the float64 EMA over the snapshots, starting as a copy of ``init``."""
    ref = {k: sr.d64(v) for k, v in init.items() if v.is_floating_point()}
    lim = {k: np.zeros(v.shape) for k, v in ref.items()}
    steps = []
    for t, snap in enumerate(snaps):
        a = sr.f32(er.alpha_ref(t, DECAY, warmup))
        for k in ref:
            new = er.lerp_ref(ref[k], snap[k], a)
            lim[k] = lim[k] + er.lerp_bound(new, snap[k], ref[k], a)
            ref[k] = new
        steps.append(({k: v.copy() for k, v in ref.items()}, {k: v.copy() for k, v in lim.items()}))
    return steps


@pytest.mark.parametrize('warmup', [True, False])
def test_an_ema_changes_no_bit_of_the_training(warmup):
    """(a)"""
    base, with_ema = _run(None), _run(warmup)
    assert with_ema['ema']._pflat is not None and with_ema['ema']._bflat is not None       # (the flat routes were taken)
    for t in range(STEPS):
        assert torch.equal(base['losses'][t], with_ema['losses'][t]), t
        for k, v in base['snaps'][t].items():
            assert torch.equal(v, with_ema['snaps'][t][k]), (t, k)                        # parameters, running statistics, counters
    for a, b in zip(base['mom'], with_ema['mom']):
        assert torch.equal(a, b)


@pytest.mark.parametrize('warmup', [True, False])
def test_the_ema_is_the_float64_recurrence_over_the_snapshots(warmup):
    """(b) and (c)"""
    r = _run(warmup)
    worst = 0.0
    moved = False
    for t, (ref, lim) in enumerate(_recurrence(r['init'], r['snaps'], warmup)):
        got = r['emas'][t]
        assert list(got.keys()) == list(r['snaps'][t].keys())
        for k, v in got.items():
            if not v.is_floating_point():
                assert torch.equal(v, r['snaps'][t][k]), k                                # integer buffers: the live value
                continue
            err = np.abs(sr.d64(v) - ref[k])
            assert np.all(err <= lim[k]), 'step %d %s: err %.3e, %.3f of the bound' % (
                t, k, float(err.max()), float((err / np.maximum(lim[k], 1e-300)).max()))
            nz = lim[k] > 0
            if nz.any():
                worst = max(worst, float((err[nz] / lim[k][nz]).max()))
            moved = moved or not torch.equal(v, r['init'][k])
    print('ema recurrence warmup=%s: worst error / bound %.3f' % (warmup, worst))
    assert moved
    # (c) the aligning gaps of both flat shadows are zero
    ema, m = r['ema'], r['model']
    arena, ba = m._retrain_state.arena, m._buffer_arena
    assert ema._arena is arena and ema._barena is ba and ema._pflat.numel() == arena.total and ema._bflat.numel() == ba.total
    for flat, slots in ((ema._pflat, [arena.slot[id(p)] for p in arena.params]), (ema._bflat, list(ba.slot.values()))):
        used = torch.zeros(flat.numel(), dtype=torch.bool)
        for o, n in slots:
            used[o:o + n] = True
        assert int((~used).sum()) > 0 and bool((flat.cpu()[~used] == 0).all())
        assert bool((flat.cpu()[used] != 0).any())


def test_fused_route_and_torch_route_agree_as_their_weights_do():
    """(d) An EMA is a convex combination of the weight snapshots, so the two routes' EMAs differ by at most the largest
    difference of their weights (measured here, per tensor, over the steps) plus the rounding of the EMA arithmetic itself: the
    fused route's bound and the torch route's (torch's fp32 lerp: 4 * 2^-24 * (|e'| + |w - e|) per update, test_ema_refs.py)."""
    f, s = _run(True), _run(True, fused=False)
    assert s['arenas'][-1] is None and s['ema']._pflat is None and s['ema']._bflat is not None
    rec = _recurrence(f['init'], f['snaps'], True)
    worst = 0.0
    for k, v in f['emas'][-1].items():
        if not v.is_floating_point():
            assert torch.equal(v, s['emas'][-1][k])
            continue
        dw = max(float((f['snaps'][t][k] - s['snaps'][t][k]).abs().max()) for t in range(STEPS))
        rounding = float(rec[-1][1][k].max()) + sum(
            4 * er.U * float((s['emas'][t][k].abs() + (s['snaps'][t][k] - (s['emas'][t - 1][k] if t else s['init'][k])).abs()).max())
            for t in range(STEPS))
        de = float((v - s['emas'][-1][k]).abs().max())
        assert de <= dw + rounding, (k, de, dw, rounding)
        worst = max(worst, de / (dw + rounding))
    print('fused vs torch route: worst ema difference / (weight difference + rounding) %.3f' % worst)


def test_validate_with_an_ema_is_validate_of_the_deployed_network():
    """(e)"""
    from tfnas_amd import model_eval as me
    r = _run(True)
    m, ema = r['model'], r['ema']
    q = _batches(2, seed=23)
    live = _cpu(m.state_dict())
    shadow = _cpu(ema.state_dict())
    got = me.validate(m, q, ema=ema)
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), live[k]), k
    for k, v in ema.state_dict().items():
        assert torch.equal(v.cpu(), shadow[k]), k
    fresh = me.NetworkCfg(CLASSES, m.config, None, 0.0, 0.0)
    fresh.load_state_dict(ema.state_dict(), strict=True)
    want = me.validate(fresh.cuda(), q)
    assert got == want, (got, want)
    raw = me.validate(m, q)
    assert raw[2] != got[2]                                                               # (the average is not the raw network)


def test_the_ema_survives_a_rebuilt_arena():
    """(f) model.to('cpu').to('cuda') between steps: a new arena, the same EMA values, and the updates after it are those of the
    uninterrupted run, bit for bit."""
    straight, r = _run(True), _run(True, roundtrip=True)
    assert r['arenas'][0] is not r['arenas'][1] and r['arenas'][1] is r['arenas'][2]
    assert r['ema']._arena is r['arenas'][2].arena and r['ema']._barena is r['model']._buffer_arena
    before, after = r['kept']
    for k in before:
        assert torch.equal(before[k], after[k]) and torch.equal(before[k], r['emas'][0][k]), k
    for t in range(STEPS):
        for k, v in straight['snaps'][t].items():
            assert torch.equal(v, r['snaps'][t][k]), (t, k)
        for k, v in straight['emas'][t].items():
            assert torch.equal(v, r['emas'][t][k]), (t, k)


def _queues(n):
    return lambda e: _batches(n, seed=100 + e)


def test_run_retrain_with_an_ema(tmp_path, monkeypatch):
    """(g)"""
    from tfnas_amd import model_eval as me
    kw = dict(lr=LR, log=lambda s: None, ema_decay=DECAY)
    h = me.run_retrain(str(tmp_path / 'straight'), _model(), _queues(2), _queues(2), epochs=2, **kw)
    a = torch.load(tmp_path / 'straight' / 'checkpoint.pth.tar', weights_only=False)
    assert set(a) == {'epoch', 'state_dict', 'best_acc_top1', 'best_acc_top5', 'optimizer', 'state_dict_ema', 'ema_updates'}
    assert a['ema_updates'] == 4 and list(a['state_dict_ema']) == list(a['state_dict'])
    assert any(not torch.equal(v, a['state_dict'][k]) for k, v in a['state_dict_ema'].items())
    for row in h:
        assert {'val_top1', 'val_top5', 'val_obj', 'val_top1_ema', 'val_top5_ema', 'val_obj_ema'} <= set(row)
        assert 0.0 <= row['val_top1_ema'] <= row['val_top5_ema'] <= 100.0 and np.isfinite(row['val_obj_ema'])
    assert a['best_acc_top1'] == max(0.0, max(row['val_top1_ema'] for row in h))
    # one epoch, then the second from the snapshot (epoch 0 has the same rate under either schedule length)
    me.run_retrain(str(tmp_path / 'first'), _model(), _queues(2), _queues(2), epochs=1, **kw)
    h2 = me.run_retrain(str(tmp_path / 'resumed'), _model(seed=77), _queues(2), _queues(2), epochs=2,
                        snapshot=str(tmp_path / 'first' / 'checkpoint.pth.tar'), **kw)
    b = torch.load(tmp_path / 'resumed' / 'checkpoint.pth.tar', weights_only=False)
    assert [row['epoch'] for row in h2] == [1] and b['ema_updates'] == a['ema_updates']
    for k, v in a['state_dict_ema'].items():
        assert torch.equal(v, b['state_dict_ema'][k]), k
    for k, v in a['state_dict'].items():
        assert torch.equal(v, b['state_dict'][k]), k
    assert h2[0]['val_top1_ema'] == h[1]['val_top1_ema'] and h2[0]['val_obj_ema'] == h[1]['val_obj_ema']
    # a snapshot written without an EMA resumes with one: the average starts from the loaded weights
    me.run_retrain(str(tmp_path / 'plain'), _model(), _queues(2), _queues(2), epochs=1, lr=LR, log=lambda s: None)
    p = torch.load(tmp_path / 'plain' / 'checkpoint.pth.tar', weights_only=False)
    assert set(p) == {'epoch', 'state_dict', 'best_acc_top1', 'best_acc_top5', 'optimizer'}
    # ... and model_best follows the EMA's top-1: validate is wrapped so that the two are told apart for certain
    real = me.validate
    seen = []

    def fake(model, q, criterion=None, ema=None):
        t1, t5, obj = real(model, q, criterion, ema=ema)
        seen.append(ema is not None)
        return (40.0, 60.0, obj) if ema is not None else (90.0, 95.0, obj)
    monkeypatch.setattr(me, 'validate', fake)
    h3 = me.run_retrain(str(tmp_path / 'late'), _model(seed=77), _queues(2), _queues(2), epochs=2,
                        snapshot=str(tmp_path / 'plain' / 'checkpoint.pth.tar'), **kw)
    monkeypatch.setattr(me, 'validate', real)
    c = torch.load(tmp_path / 'late' / 'checkpoint.pth.tar', weights_only=False)
    assert seen == [False, True] and c['ema_updates'] == 2
    assert (c['best_acc_top1'], c['best_acc_top5']) == (40.0, 60.0) and h3[0]['val_top1'] == 90.0 and h3[0]['val_top1_ema'] == 40.0
    best = torch.load(tmp_path / 'late' / 'model_best.pth.tar', weights_only=False)
    assert best['best_acc_top1'] == 40.0 and best['ema_updates'] == 2
    # the late EMA: two updates from the snapshot's weights -- it lies strictly between them and the final weights somewhere
    assert any(not torch.equal(v, c['state_dict'][k]) for k, v in c['state_dict_ema'].items())
    assert all(torch.isfinite(v.float()).all() for v in c['state_dict_ema'].values())
    assert os.path.exists(tmp_path / 'late' / 'model.config')


def test_the_fused_route_adds_one_launch_per_step():
    """The library's own count (tfnas_prof_collect) of one training step: the EMA of the parameters rides in the SGD pass, the
    buffers' is the one launch more."""
    import ctypes as C
    from tfnas_amd import _lib, model_eval as me
    lib = _lib.lib()
    nfam = lib.tfnas_prof_count()
    (x, y), = _batches(1)
    counts = []
    for with_ema in (False, True):
        m = _model().cuda()
        opt = torch.optim.SGD(m.parameters(), LR, momentum=0.9, weight_decay=4e-5)
        crit = me.CrossEntropyLabelSmooth(CLASSES, 0.1)
        ema = me.WeightEma(m, DECAY) if with_ema else None
        me.train_step(m, x.cuda(), y.cuda(), crit, opt, 5.0, ema=ema)              # (plans, arenas and layouts are built here)
        torch.cuda.synchronize()
        lib.tfnas_prof_enable((1 << nfam) - 1)
        try:
            me.train_step(m, x.cuda(), y.cuda(), crit, opt, 5.0, ema=ema)
            torch.cuda.synchronize()
            total = 0
            for i in range(nfam):
                cnt, ms = C.c_uint64(0), C.c_double(0.0)
                _lib.check(lib.tfnas_prof_collect(i, C.byref(cnt), C.byref(ms)), 'tfnas_prof_collect')
                total += cnt.value
        finally:
            lib.tfnas_prof_enable(0)
        counts.append(total)
    print('library launches per step: without EMA %d, with %d' % tuple(counts))
    assert counts[1] == counts[0] + 1
