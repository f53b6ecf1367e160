"""GPU, end to end: the 'groups' plan of model_eval.RetrainState (tfnas_opt_groups_step) on the derived network of
test_gpu_derived.py::_arch (8 x 3 x 64 x 64 inputs, 10 classes, drop rates 0) with the two parameter groups of
optim.param_groups and differing rates per group.

(a) teacher-forced step: gradients by begin / forward / backward / end, a snapshot of the arenas, ``st.step``, and the float64
restatement of tests/_optref.py on the snapshot within the kernel's bounds -- group membership derived here from the parameter
NAMES, not from the optimizer; (b) optimizer state: views of the arenas, an ordinary state_dict, step counters; (c) a changed
learning rate is honoured by the next step; (d) a one-group plain SGD still makes the tfnas_sgd_clip_step call, bit for bit; (e) an
EMA on the 'groups' plan is the float64 recurrence over the weight snapshots (the bound of test_gpu_ema_retrain.py (b)); (f) the
library's own launch count; (g) run_retrain with 'rmsprop-tf', two groups and an EMA writes loadable checkpoints and resumes."""
import ctypes as C
import io
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _emaref as er
import _optref as oref
import _smallref as sr

pytestmark = pytest.mark.gpu

CLASSES, WD, CLIP = 10, 4e-5, 5.0
OPTS = ['sgd', 'nesterov', 'rmsprop', 'rmsprop0', 'rmsprop-tf']
KIND = {'sgd': (oref.SGD, False), 'nesterov': (oref.SGD, True), 'rmsprop': (oref.RMSPROP, False), 'rmsprop0': (oref.RMSPROP, False),
        'rmsprop-tf': (oref.RMSPROP_TF, False)}
ALPHA, EPS = 0.9, 1e-3


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


def _opt(name, m):
    """Two groups with their own rates: (decayed, rate r) and (BatchNorm + biases, rate 2 r)."""
    from tfnas_amd import optim
    r = 0.05 if name in ('sgd', 'nesterov') else 0.004
    groups = optim.param_groups(m, WD)
    groups[0]['lr'], groups[1]['lr'] = r, 2 * r
    if name in ('sgd', 'nesterov'):
        return torch.optim.SGD(groups, r, momentum=0.9, nesterov=name == 'nesterov')
    if name in ('rmsprop', 'rmsprop0'):
        return torch.optim.RMSprop(groups, r, alpha=ALPHA, eps=EPS, momentum=0.9 if name == 'rmsprop' else 0.0)
    return optim.RMSpropTF(groups, r, alpha=ALPHA, eps=EPS, momentum=0.9)


def _no_decay(name):
    """Membership of the second group from the parameter's name alone: BatchNorm modules are called ``bn`` everywhere in the
    derived network, biases ``bias``."""
    return '.bn.' in name or name.endswith('.bias')


def _name_map(arena):
    gmap = np.full(arena.total // 64, 255, dtype=np.uint8)
    for name, p in zip(arena.names, arena.params):
        o, n = arena.slot[id(p)]
        assert o % 64 == 0
        gmap[o // 64:(o + n + 63) // 64] = int(_no_decay(name))
    assert not (gmap == 255).any() and (gmap == 1).any() and (gmap == 0).any()
    return gmap


def _forced(m, opt, st, x, y, ema=None):
    """One teacher-forced step: (arena snapshot before the step, arenas after it, the norm the kernel wrote)."""
    from tfnas_amd import model_eval as me
    crit = me.CrossEntropyLabelSmooth(CLASSES, 0.1)
    a = st.arena
    m.train()
    st.begin()
    try:
        crit(m(x.cuda()), y.cuda()).backward()
    finally:
        st.end()
    torch.cuda.synchronize()
    take = lambda: dict(w=a.w.cpu().clone(), g=a.g.cpu().clone(), m=a.m.cpu().clone(), v=None if st._v is None else st._v.cpu().clone())
    before = take()
    st.step(opt, CLIP, ema=ema)
    torch.cuda.synchronize()
    return before, take(), float(st._gnorm[0])


def _compare(name, opt, st, before, after, norm, lrs, worst):
    kind, nesterov = KIND[name]
    mom = opt.param_groups[0]['momentum']
    hp = dict(lr=[sr.f32(v) for v in lrs], wd=[sr.f32(WD), 0.0], mom=sr.f32(mom), alpha=sr.f32(ALPHA), eps=sr.f32(EPS),
              max_norm=sr.f32(CLIP), grad_scale=1.0, nesterov=nesterov)
    vin = before['v'] if kind != oref.SGD else None
    gmap = _name_map(st.arena)
    ref = oref.groups_ref(kind, before['w'], before['g'], before['m'], vin, gmap, **hp)
    lim = oref.groups_bounds(kind, ref, before['w'], before['m'], vin, hp['mom'], hp['alpha'], hp['eps'], nesterov)
    for k in ('w', 'g', 'm') + (('v',) if kind != oref.SGD else ()):
        if k == 'm' and name == 'rmsprop0':
            assert torch.equal(after['m'], before['m'])                          # momentum 0: m is not touched
            continue
        err = np.abs(sr.d64(after[k]) - ref[k])
        bad = np.nonzero(err > lim[k])[0]
        assert bad.size == 0, '%s %s[%d]: err %.3e > bound %.3e (%d elements)' % (name, k, bad[0], err[bad[0]], lim[k][bad[0]], bad.size)
        nz = lim[k] > 0
        worst[k] = max(worst.get(k, 0.0), float((err[nz] / lim[k][nz]).max()))
    assert abs(norm - ref['total']) <= 4 * sr.U * ref['total']
    assert not torch.equal(after['w'], before['w'])
    return ref


_runs = {}


def _run(name):
    """train_step (binds state, builds the map), then two teacher-forced steps with a rate change in between."""
    if name in _runs:
        return _runs[name]
    from tfnas_amd import model_eval as me
    m = _model().cuda()
    opt = _opt(name, m)
    assert me.RetrainState.plan(opt, m) == 'groups' and not me.RetrainState.fusable(opt, m)
    (x0, y0), (x1, y1), (x2, y2) = _batches(3)
    me.train_step(m, x0.cuda(), y0.cuda(), me.CrossEntropyLabelSmooth(CLASSES, 0.1), opt, CLIP)
    st = m._retrain_state
    out = dict(model=m, opt=opt, st=st, steps=[])
    lrs = [g['lr'] for g in opt.param_groups]
    out['steps'].append((lrs, _forced(m, opt, st, x1, y1)))
    opt.param_groups[1]['lr'] = lrs[1] * 0.25                                    # what a scheduler does
    lrs = [g['lr'] for g in opt.param_groups]
    out['steps'].append((lrs, _forced(m, opt, st, x2, y2)))
    _runs[name] = out
    return out


@pytest.mark.parametrize('name', OPTS)
def test_teacher_forced_steps_match_float64_and_honour_a_changed_rate(name):
    """(a) and (c)"""
    r = _run(name)
    worst = {}
    for lrs, (before, after, norm) in r['steps']:
        _compare(name, r['opt'], r['st'], before, after, norm, lrs, worst)
    # (c) not vacuous: with the OLD rate of group 1 the second step leaves the bounds
    lrs, (before, after, norm) = r['steps'][1]
    with pytest.raises(AssertionError):
        _compare(name, r['opt'], r['st'], before, after, norm, r['steps'][0][0], {})
    print('groups plan %s: worst error / bound %s' % (name, {k: round(v, 3) for k, v in worst.items()}))
    # the gaps of every arena are still zero
    a = r['st'].arena
    used = torch.zeros(a.total, dtype=torch.bool)
    for p in a.params:
        o, n = a.slot[id(p)]
        used[o:o + n] = True
    for k, t in after.items():
        assert t is None or bool((t[~used] == 0).all()), k


@pytest.mark.parametrize('name', OPTS)
def test_optimizer_state_lives_in_the_arenas_and_checkpoints(name):
    """(b) after train_step + two forced steps: three fused steps."""
    r = _run(name)
    m, opt, st = r['model'], r['opt'], r['st']
    a = st.arena
    kind, _ = KIND[name]
    for p in a.params:
        o, n = a.slot[id(p)]
        s = opt.state[p]
        if name != 'rmsprop0':
            assert s['momentum_buffer'].data_ptr() == a.m.data_ptr() + 4 * o and s['momentum_buffer'].shape == p.shape
        else:
            assert 'momentum_buffer' not in s
        if kind != oref.SGD:
            assert s['square_avg'].data_ptr() == st._v.data_ptr() + 4 * o and s['square_avg'].shape == p.shape
            assert int(s['step']) == 3
        else:
            assert 'step' not in s
    assert opt._step_count == 3 if hasattr(opt, '_step_count') else True
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=False)
    m2 = _model(seed=9).cuda()
    fresh = _opt(name, m2)
    fresh.load_state_dict(sd)
    assert [g['lr'] for g in fresh.param_groups] == [g['lr'] for g in opt.param_groups]
    for p, q in zip(m.parameters(), m2.parameters()):
        for k, v in opt.state[p].items():
            w = fresh.state[q][k]
            assert torch.equal(torch.as_tensor(w).cpu(), torch.as_tensor(v).cpu()), k
    # ... and the fresh optimizer steps on, fused, from the loaded state: its tensors are copied into the new model's arenas
    from tfnas_amd import model_eval as me
    x, y = _batches(1, seed=3)[0]
    me.train_step(m2, x.cuda(), y.cuda(), me.CrossEntropyLabelSmooth(CLASSES, 0.1), fresh, CLIP)
    torch.cuda.synchronize()
    p0 = next(m2.parameters())
    if kind != oref.SGD:
        assert int(fresh.state[p0]['step']) == 4
        assert fresh.state[p0]['square_avg'].data_ptr() == m2._retrain_state._v.data_ptr()
    assert all(torch.isfinite(p).all() for p in m2.parameters())


def test_one_group_plain_sgd_still_makes_the_sgd_clip_step_call(monkeypatch):
    """(d) the call is the old one, and three steps are, bit for bit, three hand-made steps of begin / forward / backward / end +
    tfnas_sgd_clip_step over the whole arena -- what the step has always been."""
    from tfnas_amd import _lib, model_eval as me
    lib = _lib.lib()
    calls = []
    real_sgd, real_groups = lib.tfnas_sgd_clip_step, lib.tfnas_opt_groups_step
    monkeypatch.setattr(lib, 'tfnas_sgd_clip_step', lambda *a: (calls.append('sgd'), real_sgd(*a))[1])
    monkeypatch.setattr(lib, 'tfnas_opt_groups_step', lambda *a: (calls.append('groups'), real_groups(*a))[1])
    monkeypatch.setattr(me, 'FUSED_TAIL', False)       # (classifier + loss by torch on both sides: the hand-made step calls them so)
    crit = me.CrossEntropyLabelSmooth(CLASSES, 0.1)
    m = _model().cuda()
    opt = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=WD)
    assert me.RetrainState.plan(opt, m) == 'sgd'
    for x, y in _batches(3):
        me.train_step(m, x.cuda(), y.cuda(), crit, opt, CLIP)
    torch.cuda.synchronize()
    assert calls == ['sgd'] * 3
    h = _model().cuda()
    st = me.RetrainState(h)
    a = st.arena
    scratch = torch.empty(4096, dtype=torch.float64, device='cuda')
    h.train()
    for x, y in _batches(3):
        st.begin()
        crit(h(x.cuda()), y.cuda()).backward()
        st.end()
        _lib.check(lib.tfnas_sgd_clip_step(_lib.ptr(a.w), _lib.ptr(a.g), _lib.ptr(a.m), 1, (C.c_uint64 * 1)(0), None,
                                           (C.c_uint64 * 1)(a.total), CLIP, 0.05, 0.9, WD, 1.0, _lib.ptr(scratch), scratch.numel(), None,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'tfnas_sgd_clip_step')
    torch.cuda.synchronize()
    assert torch.equal(m._retrain_state.arena.w, a.w) and torch.equal(m._retrain_state.arena.m, a.m)
    # and a two-group optimizer on the same model takes the new call
    m2 = _model().cuda()
    calls.clear()
    x, y = _batches(1)[0]
    me.train_step(m2, x.cuda(), y.cuda(), crit, _opt('sgd', m2), CLIP)
    assert calls == ['groups']


def test_an_ema_on_the_groups_plan_is_the_float64_recurrence():
    """(e) three steps of RMSpropTF with two groups and a WeightEma (decay 0.9, warm-up): every shadow within the summed
    _emaref.lerp_bound of the recurrence over the per-step snapshots, as in test_gpu_ema_retrain.py (b)."""
    from tfnas_amd import model_eval as me
    m = _model().cuda()
    opt = _opt('rmsprop-tf', m)
    ema = me.WeightEma(m, 0.9, True)
    crit = me.CrossEntropyLabelSmooth(CLASSES, 0.1)
    cpu = lambda sd: OrderedDict((k, v.detach().cpu().clone()) for k, v in sd.items())
    init = cpu(m.state_dict())
    ref = {k: sr.d64(v) for k, v in init.items() if v.is_floating_point()}
    lim = {k: np.zeros(v.shape) for k, v in ref.items()}
    worst, moved = 0.0, False
    for t, (x, y) in enumerate(_batches(3)):
        me.train_step(m, x.cuda(), y.cuda(), crit, opt, CLIP, ema=ema)
        torch.cuda.synchronize()
        assert ema.updates == t + 1 and ema._pflat is not None and ema._arena is m._retrain_state.arena
        snap, got = cpu(m.state_dict()), cpu(ema.state_dict())
        a = sr.f32(er.alpha_ref(t, 0.9, True))
        for k in ref:
            new = er.lerp_ref(ref[k], snap[k], a)
            lim[k] = lim[k] + er.lerp_bound(new, snap[k], ref[k], a)
            ref[k] = new
            err = np.abs(sr.d64(got[k]) - ref[k])
            assert np.all(err <= lim[k]), 'step %d %s: err %.3e' % (t, k, float(err.max()))
            nz = lim[k] > 0
            if nz.any():
                worst = max(worst, float((err[nz] / lim[k][nz]).max()))
            moved = moved or not torch.equal(got[k], init[k])
    assert moved
    print('ema on the groups plan: worst error / bound %.3f' % worst)


def _launches(lib, fn):
    from tfnas_amd import _lib
    nfam = lib.tfnas_prof_count()
    lib.tfnas_prof_enable((1 << nfam) - 1)
    try:
        fn()
        torch.cuda.synchronize()
        total = 0
        for i in range(nfam):
            cnt, ms = C.c_uint64(0), C.c_double(0.0)
            _lib.check(lib.tfnas_prof_collect(i, C.byref(cnt), C.byref(ms)), 'tfnas_prof_collect')
            total += cnt.value
    finally:
        lib.tfnas_prof_enable(0)
    return total


def test_launch_counts_of_the_groups_plan():
    """(f) tfnas_prof_collect counts one entry per kernel of tfnas_opt_groups_step (two), and one for the pair of
    tfnas_sgd_clip_step: a 'groups' step counts one more than an 'sgd' step, an EMA one more again (the buffers' lerp)."""
    from tfnas_amd import _lib, model_eval as me
    lib = _lib.lib()
    crit = me.CrossEntropyLabelSmooth(CLASSES, 0.1)
    (x, y), = _batches(1)
    counts = {}
    for key in ('sgd', 'groups', 'groups+ema'):
        m = _model().cuda()
        opt = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=WD) if key == 'sgd' else _opt('rmsprop', m)
        ema = me.WeightEma(m, 0.9) if key.endswith('ema') else None
        step = lambda: me.train_step(m, x.cuda(), y.cuda(), crit, opt, CLIP, ema=ema)
        step()                                                                   # (plans, arenas, map and layouts are built here)
        torch.cuda.synchronize()
        counts[key] = _launches(lib, step)
        if key == 'groups':
            st = m._retrain_state
            st.begin()
            st.end()
            counts['tail'] = _launches(lib, lambda: st.step(opt, CLIP))
    print('library launches per step: %r' % (counts,))
    assert counts['tail'] == 2                                                   # the optimizer's two launches, nothing else
    assert counts['groups'] == counts['sgd'] + 1
    assert counts['groups+ema'] == counts['groups'] + 1


def test_run_retrain_with_rmsprop_tf_two_groups_and_an_ema(tmp_path):
    """(g)"""
    from tfnas_amd import model_eval as me
    from tfnas_amd.optim import RMSpropTF
    q = lambda n: (lambda e: _batches(n, seed=100 + e))
    seen = []
    kw = dict(lr=0.004, log=lambda s: None, ema_decay=0.9, optimizer='rmsprop-tf', no_decay=('bn', 'bias'),
              lr_at=lambda e: seen.append(e) or 0.004 * 0.5 ** e)
    h = me.run_retrain(str(tmp_path / 'straight'), _model(), q(2), q(2), epochs=2, **kw)
    assert seen == [0, 1] and [row['lr'] for row in h] == [0.004, 0.002]
    a = torch.load(tmp_path / 'straight' / 'checkpoint.pth.tar', weights_only=False)
    assert set(a) == {'epoch', 'state_dict', 'best_acc_top1', 'best_acc_top5', 'optimizer', 'state_dict_ema', 'ema_updates'}
    assert a['ema_updates'] == 4 and len(a['optimizer']['param_groups']) == 2
    assert [g['weight_decay'] for g in a['optimizer']['param_groups']] == [4e-5, 0.0]
    st0 = a['optimizer']['state'][0]
    assert set(st0) == {'step', 'square_avg', 'momentum_buffer'} and st0['step'] == 4
    for v in list(a['state_dict'].values()) + list(a['state_dict_ema'].values()):
        assert torch.isfinite(v.float()).all()
    # loadable: a fresh network and a fresh optimizer of the same class take them
    fresh = me.NetworkCfg(CLASSES, _model().config, None, 0.0, 0.0)
    fresh.load_state_dict({k[len('module.'):]: v for k, v in a['state_dict'].items()}, strict=True)
    from tfnas_amd.optim import param_groups
    RMSpropTF(param_groups(fresh, 4e-5), 0.004).load_state_dict(a['optimizer'])
    # one epoch, then the second from the snapshot: the same bits
    me.run_retrain(str(tmp_path / 'first'), _model(), q(2), q(2), epochs=1, **kw)
    h2 = me.run_retrain(str(tmp_path / 'resumed'), _model(seed=77), q(2), q(2), epochs=2,
                        snapshot=str(tmp_path / 'first' / 'checkpoint.pth.tar'), **kw)
    b = torch.load(tmp_path / 'resumed' / 'checkpoint.pth.tar', weights_only=False)
    assert [row['epoch'] for row in h2] == [1] and b['ema_updates'] == 4
    for k, v in a['state_dict'].items():
        assert torch.equal(v, b['state_dict'][k]), k
    for k, v in a['state_dict_ema'].items():
        assert torch.equal(v, b['state_dict_ema'][k]), k
    # the keywords left alone: the optimizer and the checkpoint keys of ever
    me.run_retrain(str(tmp_path / 'plain'), _model(), q(1), q(1), epochs=1, lr=0.05, log=lambda s: None)
    p = torch.load(tmp_path / 'plain' / 'checkpoint.pth.tar', weights_only=False)
    assert set(p) == {'epoch', 'state_dict', 'best_acc_top1', 'best_acc_top5', 'optimizer'}
    g0, = p['optimizer']['param_groups']
    assert (g0['lr'], g0['momentum'], g0['weight_decay'], g0['nesterov'], g0['dampening']) == (0.05, 0.9, 4e-5, False, 0)
    with pytest.raises(ValueError):
        me.run_retrain(str(tmp_path / 'bad'), _model(), q(1), q(1), epochs=1, optimizer='adam')
