"""CPU: the float64 restatements of tests/_smallref.py against torch's own float64 CPU path (clip_grad_norm_ + torch.optim.SGD /
Adam + F.log_softmax, the oracle's gumbel_softmax under autograd, the oracle's MixedOP.forward for sampled positions), to 1e-12
relative and exactly for positions -- so that the GPU tests of the optimizer / architecture / sink kernels compare against
something that is itself pinned.  Also here, before any GPU is involved: the exclusion cap of the sampling cases, the tie rules,
and torch's fp32 SGD against the error bound the GPU test applies to the kernel (a bound torch's own fp32 misses would be wrong)."""
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _smallref as sr
import tfnas_oracle as orc

RTOL = 1e-12


def _close64(a, b, what):
    a, b = sr.d64(a), sr.d64(b)
    err = np.abs(a - b).max() if a.size else 0.0
    lim = RTOL * max(np.abs(b).max() if b.size else 0.0, 1e-300)
    assert err <= lim, '%s: %.3e > %.3e' % (what, err, lim)


def _sgd_inputs(seed, n=3000):
    g = torch.Generator().manual_seed(seed)
    w, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.3, torch.randn(n, generator=g) * 0.1
    ranges = [(2000, 400), (8, 4), (100, 1024), (1500, 256)]
    return w, gr, m, ranges


def _torch_sgd(w, gr, m, ranges, max_norm, lr, mom, wd, grad_scale, dtype):
    ps = [w[o:o + n].to(dtype).clone().requires_grad_(True) for o, n in ranges]
    for p, (o, n) in zip(ps, ranges):
        p.grad = gr[o:o + n].to(dtype) * grad_scale
    opt = torch.optim.SGD(ps, lr=lr, momentum=mom, weight_decay=wd)
    if mom:
        for p, (o, n) in zip(ps, ranges):
            opt.state[p]['momentum_buffer'] = m[o:o + n].to(dtype).clone()
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm)) if max_norm > 0 else None
    opt.step()
    return ps, opt, total


@pytest.mark.parametrize('hp', [(0.025, 0.9, 1e-5), (0.2, 0.0, 0.0)])
@pytest.mark.parametrize('grad_scale', [1.0, 0.5, 1.0 / 3.0])
@pytest.mark.parametrize('clip', [0.5, 2.0, 1.001, 0.999, 0.0, -1.0])
def test_sgd_clip_ref_equals_torch_float64(hp, grad_scale, clip):
    lr, mom, wd = hp
    w, gr, m, ranges = _sgd_inputs(1)
    n0 = float(np.sqrt(sum(float((gr[o:o + n].double() ** 2).sum()) for o, n in ranges))) * grad_scale
    max_norm = clip * n0 if clip > 0 else clip
    ps, opt, total = _torch_sgd(w, gr, m, ranges, max_norm, lr, mom, wd, grad_scale, torch.float64)
    w2, g2, m2, tot = sr.sgd_clip_ref(w, gr, m, ranges, None, max_norm, lr, mom, wd, grad_scale)
    if total is not None:
        assert abs(tot - total) <= RTOL * total
    assert abs(tot - n0) <= RTOL * n0
    touched = np.zeros(len(w), dtype=bool)
    for p, (o, n) in zip(ps, ranges):
        _close64(w2[o:o + n], p.detach(), 'w')
        _close64(g2[o:o + n], p.grad, 'clipped g')
        if mom:
            _close64(m2[o:o + n], opt.state[p]['momentum_buffer'], 'momentum')
        else:                                   # (torch keeps no buffer at momentum 0; the kernel's m becomes the step direction)
            _close64(m2[o:o + n], p.grad + wd * w[o:o + n].double(), 'momentum 0')
        touched[o:o + n] = True
    for new, old in ((w2, w), (g2, gr), (m2, m)):
        assert np.array_equal(new[~touched], sr.d64(old)[~touched])


def test_sgd_clip_ref_packed_gradient_equals_in_place():
    w, gr, m, ranges = _sgd_inputs(2)
    goff, pos = [], 12
    for o, n in ranges:
        goff.append(pos)
        pos += n + 4
    msg = torch.full((pos,), -5.0)
    for q, (o, n) in zip(goff, ranges):
        msg[q:q + n] = gr[o:o + n]
    a = sr.sgd_clip_ref(w, gr, m, ranges, None, 1.0, 0.025, 0.9, 1e-5, 0.5)
    b = sr.sgd_clip_ref(w, msg, m, ranges, goff, 1.0, 0.025, 0.9, 1e-5, 0.5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    for q, (o, n) in zip(goff, ranges):
        assert np.array_equal(b[1][q:q + n], a[1][o:o + n])
    untouched = np.ones(pos, dtype=bool)
    for q, (o, n) in zip(goff, ranges):
        untouched[q:q + n] = False
    assert np.all(b[1][untouched] == -5.0)


@pytest.mark.parametrize('hp', [(0.025, 0.9, 1e-5), (0.2, 0.0, 0.0)])
@pytest.mark.parametrize('clip', [0.5, 2.0, 0.0])
def test_torch_fp32_sgd_meets_the_bound_the_kernel_is_held_to(hp, clip):
    """The GPU test's element-wise bound (sgd_bounds) applied to torch's own fp32 CPU clip_grad_norm_ + SGD on inputs of the GPU
    test's kind: if torch's fp32 missed it, the bound would be wrong.  Worst ratio seen here: 0.49 of the bound (the final rounding of w')."""
    lr, mom, wd = hp
    g = torch.Generator().manual_seed(3)
    n = 40000
    w, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.3, torch.randn(n, generator=g) * 0.1
    ranges = [(24000, 8196), (0, 8192), (9000, 4), (10000, 8188)]
    for grad_scale in (1.0, 1.0 / 3.0):
        gs = sr.f32(grad_scale)
        n0 = float(np.sqrt(sum(float((gr[o:o + k].double() ** 2).sum()) for o, k in ranges))) * gs
        max_norm = sr.f32(clip * n0)
        ps, opt, _ = _torch_sgd(w, gr, m, ranges, max_norm, sr.f32(lr), sr.f32(mom), sr.f32(wd), gs, torch.float32)
        w2, g2, m2, _ = sr.sgd_clip_ref(w, gr, m, ranges, None, max_norm, sr.f32(lr), sr.f32(mom), sr.f32(wd), gs)
        bm, bw = sr.sgd_bounds(w, g2, m, w2, ranges, None, sr.f32(lr), sr.f32(mom), sr.f32(wd))
        worst = 0.0
        for p, (o, k) in zip(ps, ranges):
            errs = [(np.abs(sr.d64(p.detach()) - w2[o:o + k]), bw[o:o + k]), (np.abs(sr.d64(p.grad) - g2[o:o + k]), bm[o:o + k])]
            if mom:                             # (torch keeps no buffer at momentum 0)
                errs.append((np.abs(sr.d64(opt.state[p]['momentum_buffer']) - m2[o:o + k]), bm[o:o + k]))
            for err, lim in errs:
                assert np.all(err <= lim)
                worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        print('torch fp32 SGD: worst error / bound = %.3f' % worst)


_ADAM = dict(lr=0.01, b1=0.5, b2=0.999, eps=1e-8)


@pytest.mark.parametrize('wd', [5e-4, 0.0])
@pytest.mark.parametrize('grad_scale', [1.0, 1.0 / 3.0])
@pytest.mark.parametrize('clip', [0.5, 2.0, 0.0])
def test_adam_project_ref_equals_torch_float64_for_three_chained_steps(wd, grad_scale, clip):
    g = torch.Generator().manual_seed(5)
    lens = [8] * 18 + [2, 3, 4, 4, 4, 1, 5, 6, 7]
    ps = [F.log_softmax(torch.randn(k, generator=g), -1).double().requires_grad_(True) for k in lens]
    opt = torch.optim.Adam(ps, lr=_ADAM['lr'], betas=(_ADAM['b1'], _ADAM['b2']), eps=_ADAM['eps'], weight_decay=wd)
    m, v = np.zeros((len(lens), 8)), np.zeros((len(lens), 8))
    mine = [p.detach().clone() for p in ps]
    for step in (1, 2, 3):
        grads = [torch.randn(k, generator=g) * 0.2 for k in lens]
        grads[5][2] = 0.0
        n0 = float(torch.cat(grads).double().norm()) * grad_scale
        max_norm = clip * n0
        for p, gr in zip(ps, grads):
            p.grad = gr.double() * grad_scale
        if max_norm > 0:
            total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        opt.step()
        with torch.no_grad():
            for p in ps:
                p.copy_(F.log_softmax(p, dim=-1))                 # train_search.py:421-422
        mine, m, v, tot, _ = sr.adam_project_ref(mine, grads, m, v, max_norm, _ADAM['lr'], _ADAM['b1'], _ADAM['b2'], _ADAM['eps'],
                                                 wd, step, grad_scale)
        assert abs(tot - n0) <= RTOL * n0
        for i, (p, q) in enumerate(zip(ps, mine)):
            _close64(q, p.detach(), 'p step %d' % step)
            _close64(m[i, :lens[i]], opt.state[p]['exp_avg'], 'exp_avg step %d' % step)
            _close64(v[i, :lens[i]], opt.state[p]['exp_avg_sq'], 'exp_avg_sq step %d' % step)
            assert abs(float(np.log(np.sum(np.exp(q))))) < 1e-14
        assert np.all(m[-4, 1:] == 0) and np.all(v[-4, 1:] == 0)  # the length-1 row: its padding stays
    assert mine[-4][0] == 0.0                                     # a length-1 tensor projects to exactly 0


@pytest.mark.parametrize('T', [5.0, 1.0, 0.1])
def test_gumbel_and_its_backward_equal_the_oracle_in_double(T):
    g = torch.Generator().manual_seed(7)
    ncell = 18
    la = F.log_softmax(torch.randn(ncell, 8, generator=g), -1)
    e = torch.empty(ncell, 8).exponential_(generator=g)
    e[0, 3], e[1, 0], e[2, 5] = 1e-30, 50.0, 1e-30
    lat = torch.rand(ncell, 8, generator=g) * 2
    dw, dcl = torch.randn(ncell, 8, generator=g), torch.randn(ncell, generator=g)
    la64 = la.double().requires_grad_(True)
    w = torch.stack([orc.gumbel_softmax(la64[c], T, e[c].double()) for c in range(ncell)])
    cl = (w * lat.double()).sum(1)
    w_ref, cl_ref = sr.gumbel_ref(la, e, T, lat)
    _close64(w_ref, w.detach(), 'w')
    _close64(cl_ref, cl.detach(), 'cell_lat')
    for use_dw, use_dcl, use_lat in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1)):
        obj = w.sum() * 0
        if use_dw:
            obj = obj + (w * dw.double()).sum()
        if use_dcl and use_lat:
            obj = obj + (cl * dcl.double()).sum()
        gr, = torch.autograd.grad(obj, la64, retain_graph=True)
        ref = sr.arch_bwd_ref(w.detach(), lat if use_lat else None, dw if use_dw else None, dcl if use_dcl else None, T)
        err = np.abs(ref - gr.numpy()).max()
        assert err <= 1e-12 * max(np.abs(gr.numpy()).max(), 1.0), (use_dw, use_dcl, use_lat, err)


def _oracle_cell():
    mids = [20, 24, 28, 32, 36, 40, 44, 48]

    class AnyLut(dict):
        def __missing__(self, key):
            v = self[key] = {m: 1.0 for m in mids}
            return v
    torch.manual_seed(0)
    return orc.MixedOP(16, 16, 1, 'relu', OrderedDict(enumerate(mids)), AnyLut()).double()


def test_sample_ref_equals_oracle_mixedop_positions():
    """Every 11th call of the GPU test's case list (all modes, both temperatures, partial masks), first cell: the oracle's
    MixedOP.forward in double picks the same position.  'gumbel_2' is the oracle's mode 0 under partial masks."""
    o = _oracle_cell()
    x = torch.zeros(1, 16, 2, 2, dtype=torch.float64)
    names = {0: 'gumbel_2', 1: 'min_alphas', 2: 'max_alphas'}
    checked = 0
    for case in sr.sample_cases()[::11]:
        pos, _ = sr.sample_ref(case['la'], case['mask'], case['e'], case['T'], case['mode'])
        for c in range(min(case['ncell'], 3)):
            sw = [bool(b) for b in case['mask'][c]]
            with torch.no_grad():
                o.log_alphas.copy_(case['la'][c].double())
            o.switches = sw[:]
            o.set_temperature(case['T'])
            o(x, True, names[case['mode']], exp_noise=case['e'][c][:sum(sw)].double())
            assert [i for i, s in enumerate(sw) if s].index(o.last_idx) == pos[c], (case['mode'], case['T'], c)
            checked += 1
    assert checked >= 30


def test_sampling_cases_cover_what_they_claim_and_stay_under_the_exclusion_cap():
    cases = sr.sample_cases()
    for mode in (0, 1, 2):
        mine = [c for c in cases if c['mode'] == mode]
        assert len(mine) >= 60 and {c['ncell'] for c in mine} == {1, 18, 32} and {c['T'] for c in mine} == {5.0, 0.1}
        on = torch.cat([c['mask'].sum(1) for c in mine])
        assert set(on.tolist()) == set(range(1, 9))
        assert any(c['ncell'] > 1 and int((c['mask'][1:].sum(1) < 8).sum()) > 0 for c in mine)      # knocked-out candidates at c > 0
    cells = left_out = 0
    min_gap = np.inf
    for c in cases:
        if c['mode'] == 0:
            pos, gap = sr.sample_ref(c['la'], c['mask'], c['e'], c['T'], 0)
            one = c['mask'].sum(1).numpy() == 1
            assert np.all(pos[one] == 0)
            cells += len(gap)
            left_out += int((gap < sr.SAMPLE_GAP).sum())
            min_gap = min(min_gap, float(gap.min()))
    print('mode-0 cells %d, left out %d, smallest top-two gap %.3e' % (cells, left_out, min_gap))
    assert left_out <= sr.SAMPLE_CAP * cells


def test_ties_give_the_first_position_like_torch_cpu():
    for la, mask in sr.tie_cases():
        for mode, fn in ((1, torch.argmin), (2, torch.argmax)):
            pos, gap = sr.sample_ref(la, mask, None, 1.0, mode)
            for c in range(len(la)):
                assert pos[c] == int(fn(la[c][mask[c]])) and gap[c] == np.inf
    eq, m_eq = sr.tie_cases()[0]
    assert sr.sample_ref(eq, m_eq, None, 1.0, 1)[0].tolist() == [0, 0, 0] == sr.sample_ref(eq, m_eq, None, 1.0, 2)[0].tolist()
    dup, m_dup = sr.tie_cases()[1]
    assert sr.sample_ref(dup, m_dup, None, 1.0, 2)[0].tolist() == [1, 1, 1]      # third row: candidates 0, 3, 4.. -> -1 first at 1
    assert sr.sample_ref(dup, m_dup, None, 1.0, 1)[0].tolist() == [2, 0, 3]


@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_sink_ref_equals_torch_float64(K):
    g = torch.Generator().manual_seed(K)
    betas, cl = torch.randn(K, generator=g), torch.rand(K, generator=g)
    res = [torch.randn(36, generator=g) for _ in range(K)]
    dout = torch.randn(36, generator=g)
    b = betas.double().requires_grad_(True)
    c = cl.double().requires_grad_(True)
    rs = [r.double().requires_grad_(True) for r in res]
    bw = F.softmax(b, -1)
    out = sum(wk * r for wk, r in zip(bw, rs))
    lat = sum(wk * ck for wk, ck in zip(bw, torch.cumsum(c, 0)))
    ((out * dout.double()).sum() + 1.7 * lat).backward()
    r = sr.sink_ref(betas, res, cl, dout, 1.7)
    _close64(r['out'], out.detach(), 'out')
    assert abs(r['out_lat'] - float(lat.detach())) <= RTOL * abs(float(lat.detach()))
    _close64(r['dbetas'], b.grad, 'dbetas') if K > 1 else None
    _close64(r['dcell_lat'], c.grad, 'dcell_lat')
    # closed forms of the header: dres[k] = bw[k] dout, dcell_lat[j] = dlat sum_{k>=j} bw[k]
    for k in range(K):
        _close64(r['dres'][k], r['bw'][k] * sr.d64(dout), 'dres')
        _close64(r['dcell_lat'][k], 1.7 * r['bw'][k:].sum(), 'dcell_lat closed form')
    r0 = sr.sink_ref(betas, res, None, dout, None)
    assert r0['out_lat'] == 0.0 and np.all(r0['dcell_lat'] == 0)
