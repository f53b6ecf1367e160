"""CPU: the float64 restatements of tests/_optref.py against torch's own optimizers in float64 (two parameter groups, three
steps, clip_grad_norm_ in between), and the error bounds against a float32 emulation of the kernel's operation order (not
hollow) and against three wrong formulas (not slack).

Tolerance of the float64 comparisons: 1e-12 of (|old value| + |new value|) per element -- both sides are float64 and differ
only in the order of their operations; measuring against the operands keeps an element whose update happens to cancel from
turning a 1e-16 rounding into a large relative number."""
import numpy as np
import pytest
import torch

import _optref as oref
import _smallref as sr

SIZES = [100, 64, 30, 200, 7, 128]          # parameter i belongs to group i % 2; slots padded to 64 floats, like the weight arena
LR, WD = [0.05, 0.2], [4e-5, 0.0]


def _layout():
    off, pos = [], 0
    for n in SIZES:
        off.append(pos)
        pos += (n + 63) // 64 * 64
    gmap = np.full(pos // 64, 255, dtype=np.uint8)
    for i, (o, n) in enumerate(zip(off, SIZES)):
        gmap[o // 64:(o + n + 63) // 64] = i % 2
    return off, pos, gmap


def _flat(tensors, off, total, fill=0.0):
    out = np.zeros(total)
    for t, o, n in zip(tensors, off, SIZES):
        out[o:o + n] = fill if t is None else t.detach().numpy().reshape(-1)
    return out


def _make(name, params, mom):
    from tfnas_amd.optim import RMSpropTF
    groups = [{'params': params[0::2], 'lr': LR[0], 'weight_decay': WD[0]}, {'params': params[1::2], 'lr': LR[1], 'weight_decay': WD[1]}]
    if name == 'sgd':
        return torch.optim.SGD(groups, lr=0.1, momentum=mom), oref.SGD
    if name == 'nesterov':
        return torch.optim.SGD(groups, lr=0.1, momentum=mom, nesterov=True), oref.SGD
    if name == 'rmsprop':
        return torch.optim.RMSprop(groups, lr=0.1, alpha=oref.ALPHA, eps=oref.EPS, momentum=mom), oref.RMSPROP
    return RMSpropTF(groups, lr=0.1, alpha=oref.ALPHA, eps=oref.EPS, momentum=mom), oref.RMSPROP_TF


@pytest.mark.parametrize('name,kind,nesterov,mom', oref.KINDS)
def test_restatements_match_torch_float64(name, kind, nesterov, mom):
    off, total, gmap = _layout()
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64)) for n in SIZES]
    opt, kind2 = _make(name, params, mom)
    assert kind2 == kind
    w = _flat(params, off, total)
    m = np.zeros(total)
    v = _flat([None] * len(SIZES), off, total, fill=1.0 if kind == oref.RMSPROP_TF else 0.0)     # each optimizer's own start
    for step in range(3):
        grads = [torch.randn(n, generator=gen, dtype=torch.float64) * (0.3 + step) for n in SIZES]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        g = _flat(grads, off, total)
        max_norm = 0.5 * float(np.sqrt(np.sum(g ** 2))) if step != 1 else 1e3          # clipping, not clipping, clipping
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        ref = oref.groups_ref(kind, w, g, m, v, gmap, LR, WD, mom, oref.ALPHA, oref.EPS, max_norm, 1.0, nesterov)
        got = dict(w=_flat(params, off, total), g=_flat([p.grad for p in params], off, total))
        st = [opt.state[p] for p in params]
        if 'momentum_buffer' in st[0] and st[0]['momentum_buffer'] is not None:
            got['m'] = _flat([s['momentum_buffer'] for s in st], off, total)
        if 'square_avg' in st[0]:
            got['v'] = _flat([s['square_avg'] for s in st], off, total)
        assert set(got) >= ({'w', 'g'} | ({'v'} if kind != oref.SGD else set()) | ({'m'} if mom > 0 else set()))
        old = dict(w=w, g=g, m=m, v=v)
        for k, val in got.items():
            err = np.abs(val - ref[k])
            lim = 1e-12 * (np.abs(old[k]) + np.abs(ref[k]))
            assert np.all(err <= lim), (name, step, k, float(err.max()))
        w, m, v = ref['w'], ref['m'], ref['v']
        assert np.all(ref['w'][~ref['live']] == 0) and np.all(ref['v'][~ref['live']] == 0)       # the gaps stay zero


def _inputs(kind_row, mname, clip, gs, seed=7):
    name, kind, nesterov, mom = kind_row
    w, g, m, v, ema, gap = oref.make_state(oref.TOTAL, seed)
    gmap, ng = oref.maps()[mname]
    n0 = float(g.double().norm()) * sr.f32(gs)
    hp = dict(lr=[sr.f32(x) for x in LR[:ng]], wd=[sr.f32(x) for x in WD[:ng]], mom=sr.f32(mom), alpha=sr.f32(oref.ALPHA),
              eps=sr.f32(oref.EPS), max_norm=sr.f32(clip * n0), grad_scale=sr.f32(gs), nesterov=nesterov)
    return kind, (w, g, m, v if kind != oref.SGD else None), ema, gmap, hp


@pytest.mark.parametrize('row', oref.KINDS, ids=lambda r: '%s-%g' % (r[0], r[3]))
def test_bounds_hold_a_float32_emulation(row):
    """Not hollow: the kernel's operation order in numpy float32 stays inside the bounds, every element, on the GPU tests' inputs."""
    worst = {}
    for mname in ('interleaved', 'single', 'zero'):
        for clip, gs in ((0.5, 1.0), (2.0, 0.5)):
            kind, (w, g, m, v), ema, gmap, hp = _inputs(row, mname, clip, gs)
            ref = oref.groups_ref(kind, w, g, m, v, gmap, ema=ema, ema_alpha=sr.f32(0.01), **hp)
            lim = oref.groups_bounds(kind, ref, w, m, v, hp['mom'], hp['alpha'], hp['eps'], hp['nesterov'], ema, sr.f32(0.01))
            emu = oref.groups_emul32(kind, w, g, m, v, gmap, ema=ema, ema_alpha=sr.f32(0.01), **hp)
            for k in ('w', 'g', 'm', 'v', 'ema'):
                err = np.abs(emu[k].astype(np.float64) - ref[k])
                assert np.all(err <= lim[k]), (row, mname, k, int(np.argmax(err - lim[k])))
                nz = lim[k] > 0
                if nz.any():
                    worst[k] = max(worst.get(k, 0.0), float((err[nz] / lim[k][nz]).max()))
            assert abs(emu['total'] - ref['total']) <= 4 * sr.U * ref['total']
    print('emulation %s: worst error / bound %s' % (row[0], {k: round(x, 3) for k, x in worst.items()}))


@pytest.mark.parametrize('row,wrong', [(oref.KINDS[3], 'eps'), (oref.KINDS[4], 'eps'), (oref.KINDS[5], 'eps'),
                                       (oref.KINDS[2], 'lookahead'), (oref.KINDS[5], 'rate')])
def test_bounds_reject_wrong_formulas(row, wrong):
    """Not slack: eps on the wrong side of the root, Nesterov without its look-ahead and the TF form with the rate outside the
    momentum each leave the bounds of w' (on most elements, in fact)."""
    kind, (w, g, m, v), ema, gmap, hp = _inputs(row, 'interleaved', 0.5, 1.0)
    ref = oref.groups_ref(kind, w, g, m, v, gmap, **hp)
    lim = oref.groups_bounds(kind, ref, w, m, v, hp['mom'], hp['alpha'], hp['eps'], hp['nesterov'])
    bad = oref.groups_ref(kind, w, g, m, v, gmap, wrong=wrong, **hp)
    out = np.abs(bad['w'] - ref['w']) > lim['w']
    assert out.any()
    print('%s / %s: %.1f%% of the elements leave the bound' % (row[0], wrong, 100.0 * out.mean()))
    assert out.mean() > 0.5
