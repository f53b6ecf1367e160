"""GPU: the fused tail of the derived network's retrain path (csrc/cls_kernels.hip: k_cls_ce_ex / k_cls_reduce through tfnas_cls_ce_ex /
tfnas_cls_reduce; tail.RetrainTailFn / DeviceMeter; model_eval.train_step / validate / run_retrain with FUSED_TAIL).

Reference arithmetic: the classifier of models/model_eval.py + CrossEntropyLabelSmooth(num_classes, 0.1) (train_eval.py:72-85,126)
and the loops of train_eval.py:228-293.  The kernels are compared with torch's own fp32 ops on the GPU (F.linear +
F.cross_entropy(label_smoothing=eps) through autograd), the top-k counts with search.accuracy, a whole training step with the CPU
oracle (oracle.DerivedNetwork + oracle.label_smooth_loss) and with the same step on the torch tail.

Tolerances are the project's own: 1e-5 + 1e-4 * max|ref| (tests/test_gpu_tail.py), 1e-5 + 1e-5 * |ref| on a loss scalar, and for a
whole training step tests/test_gpu_derived.py's |d loss| < 1e-4 and 1e-5 + 2e-3 * max|ref| on the state.  Counts are exact."""
import ctypes as C
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import tfnas_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(8, 1280, 100), (5, 64, 7), (128, 1280, 100), (3, 260, 1000), (256, 1280, 1000)]


def _close(a, b, what, rtol=1e-4, atol=1e-5):
    err = float((a - b).abs().max())
    lim = atol + rtol * float(b.abs().max())
    print('%s: max err %.3e (limit %.3e)' % (what, err, lim))
    assert err <= lim, '%s: max err %.3e > %.3e' % (what, err, lim)


def _loss_close(a, b, what='loss'):
    a, b = float(a), float(b)
    print('%s: %.8f vs %.8f' % (what, a, b))
    assert abs(a - b) <= 1e-5 + 1e-5 * abs(b), (what, a, b)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _problem(N, Cf, K, seed=None):
    """W, b, x on the GPU and targets that make the counts non-trivial: rows 0, 3, 6, ... take the argmax class of the reference
    logits, rows 1, 4, 7, ... the third-ranked class, the rest are random."""
    g = torch.Generator().manual_seed(N + K if seed is None else seed)
    W = (torch.randn(K, Cf, generator=g) * 0.05).cuda()
    b = (torch.randn(K, generator=g) * 0.1).cuda()
    x = torch.randn(N, Cf, generator=g).cuda()
    t = torch.randint(0, K, (N,), generator=g).cuda()
    order = F.linear(x, W, b).argsort(dim=1, descending=True)
    t[0::3] = order[0::3, 0]
    t[1::3] = order[1::3, 2]
    return W, b, x, t


def _ce_ex(x, W, b, t, eps, grads=True):
    from tfnas_amd import _lib
    N, Cf = x.shape
    K = W.shape[0]
    logits = torch.empty(N, K, device='cuda')
    loss_n = torch.empty(N, device='cuda')
    rank = torch.empty(N, device='cuda', dtype=torch.int32)
    dlog = torch.empty(N, K, device='cuda') if grads else None
    dpool = torch.empty(N, Cf, device='cuda') if grads else None
    rc = _lib.lib().tfnas_cls_ce_ex(N, Cf, K, _lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(t), 1.0 / N, eps, _lib.ptr(logits),
                                    _lib.ptr(loss_n), _lib.ptr(rank), _lib.ptr(dlog), _lib.ptr(dpool), _stream())
    assert rc == 0
    return logits, loss_n, rank, dlog, dpool


def _reduce(x, dlog, loss_n, rank, K, gscale=None, acc=0, dW=None, db=None, out=None, meter=None):
    from tfnas_amd import _lib
    N, Cf = x.shape
    rc = _lib.lib().tfnas_cls_reduce(N, Cf, K, _lib.ptr(x), _lib.ptr(dlog), _lib.ptr(loss_n), _lib.ptr(rank), _lib.ptr(gscale), acc,
                                     _lib.ptr(dW), _lib.ptr(db), _lib.ptr(out), _lib.ptr(meter), _stream())
    assert rc == 0


def _no_ties_with_target(logits, t):
    lt = logits.gather(1, t.view(-1, 1))
    return int((logits == lt).sum()) == logits.size(0)


def _counts(logits, t):
    from tfnas_amd import search
    n = t.numel()
    p1, p5 = search.accuracy(logits, t, (1, 5))
    return round(float(p1) * n / 100.0), round(float(p5) * n / 100.0)


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('N,Cf,K', SHAPES)
def test_kernels_match_torch(N, Cf, K, eps):
    """Logits, per-image loss, d logits, d pooled, dW, db and the loss scalar against F.linear + F.cross_entropy(label_smoothing)
    through autograd; top-1 / top-5 counts from ``rank`` against search.accuracy on the logits the ranks were taken from (no logit
    ties with its row's target logit, in the reference's logits or the kernel's, so no tie rule is involved: exact)."""
    W, b, x, t = _problem(N, Cf, K)
    Wr, br, xr = (v.clone().requires_grad_(True) for v in (W, b, x))
    ref = F.linear(xr, Wr, br)
    ref.retain_grad()
    assert _no_ties_with_target(ref.detach(), t)
    loss_ref = F.cross_entropy(ref, t, label_smoothing=eps)
    loss_ref.backward()
    loss_n_ref = F.cross_entropy(ref.detach(), t, label_smoothing=eps, reduction='none')
    logits, loss_n, rank, dlog, dpool = _ce_ex(x, W, b, t, eps)
    dW, db, out = torch.empty_like(W), torch.empty_like(b), torch.empty(4, device='cuda')
    _reduce(x, dlog, loss_n, rank, K, dW=dW, db=db, out=out)
    torch.cuda.synchronize()
    _close(logits, ref.detach(), 'logits')
    _close(loss_n, loss_n_ref, 'loss_n')
    _close(dlog, ref.grad, 'd logits')
    _close(dpool, xr.grad, 'd pooled')
    _close(dW, Wr.grad, 'dW')
    _close(db, br.grad, 'db')
    _loss_close(out[0], loss_ref)
    assert _no_ties_with_target(logits, t)
    c1, c5 = _counts(logits, t)
    print('top-1 %d top-5 %d of %d' % (c1, c5, N))
    assert c1 >= (N + 2) // 3 and c5 >= c1 + (N + 1) // 3            # (the constructed rows: non-trivial counts)
    assert int((rank == 0).sum()) == c1 and int(((rank >= 0) & (rank < 5)).sum()) == c5
    assert out.tolist()[1:] == [float(c1), float(c5), 0.0]


def test_tie_rule_lower_class_index_ranks_first():
    """Hand-made rows (pooled = 0, so logits = bias): rank = #greater + #equal with a lower class index, independent of torch."""
    K, Cf = 8, 4
    x = torch.zeros(6, Cf, device='cuda')
    W = torch.randn(K, Cf, device='cuda')
    rows = [([1.0] * 8, 3, 3), ([1.0] * 8, 0, 0), ([1.0] * 8, 5, 5), ([2.0, 1.0, 1.0, 0.0, 1.0, 3.0, 1.0, 1.0], 2, 3),
            ([2.0, 1.0, 1.0, 0.0, 1.0, 3.0, 1.0, 1.0], 7, 6), ([0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5], 7, 2)]
    for bias, t, want in rows:
        b = torch.tensor(bias, device='cuda')
        tt = torch.full((6,), t, device='cuda', dtype=torch.int64)
        logits, _, rank, _, _ = _ce_ex(x, W, b, tt, 0.1)
        torch.cuda.synchronize()
        assert torch.equal(logits[0], b)
        assert rank.tolist() == [want] * 6, (bias, t, rank.tolist())
    # exactly one class of an all-equal row has rank 0
    b = torch.ones(K, device='cuda')
    ranks = []
    for t in range(K):
        ranks.append(int(_ce_ex(x, W, b, torch.full((6,), t, device='cuda', dtype=torch.int64), 0.0)[2][0]))
    assert ranks == list(range(K))


@pytest.mark.parametrize('N,Cf,K', [(8, 1280, 100), (5, 64, 7), (256, 1280, 1000)])
def test_eps0_bit_identical_to_tfnas_cls_ce(N, Cf, K):
    from tfnas_amd import _lib
    W, b, x, t = _problem(N, Cf, K)
    base = [torch.empty(N, K, device='cuda'), torch.empty(N, device='cuda'), torch.empty(N, K, device='cuda'),
            torch.empty(N, Cf, device='cuda')]
    rc = _lib.lib().tfnas_cls_ce(N, Cf, K, _lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(t), 1.0 / N, *[_lib.ptr(v) for v in base],
                                 _stream())
    assert rc == 0
    logits, loss_n, rank, dlog, dpool = _ce_ex(x, W, b, t, 0.0)
    torch.cuda.synchronize()
    for name, a, r in zip(('logits', 'loss_n', 'dlogits', 'dpooled'), (logits, loss_n, dlog, dpool), base):
        assert torch.equal(a, r), name


@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_forward_only_and_deterministic(eps):
    N, Cf, K = 128, 1280, 1000
    W, b, x, t = _problem(N, Cf, K)
    full = _ce_ex(x, W, b, t, eps)
    fwd = _ce_ex(x, W, b, t, eps, grads=False)
    again = _ce_ex(x, W, b, t, eps)
    torch.cuda.synchronize()
    for i, name in enumerate(('logits', 'loss_n', 'rank')):
        assert torch.equal(full[i], fwd[i]), name
    for i, name in enumerate(('logits', 'loss_n', 'rank', 'dlogits', 'dpooled')):
        assert torch.equal(full[i], again[i]), name
    outs = []
    for _ in range(2):
        dW, db, out = torch.empty_like(W), torch.empty_like(b), torch.empty(4, device='cuda')
        _reduce(x, full[3], full[1], full[2], K, dW=dW, db=db, out=out)
        outs.append((dW, db, out))
    torch.cuda.synchronize()
    for a, r in zip(*outs):
        assert torch.equal(a, r)


def test_gscale_and_accumulate_in_the_reduction():
    N, Cf, K = 16, 260, 37
    W, b, x, t = _problem(N, Cf, K)
    logits, loss_n, rank, dlog, dpool = _ce_ex(x, W, b, t, 0.1)
    dW0, db0, out0 = torch.empty_like(W), torch.empty_like(b), torch.empty(4, device='cuda')
    _reduce(x, dlog, loss_n, rank, K, dW=dW0, db=db0, out=out0)
    # a device-resident upstream gradient
    gs = torch.tensor(0.5, device='cuda')
    dW1, db1 = torch.empty_like(W), torch.empty_like(b)
    _reduce(x, dlog, loss_n, rank, K, gscale=gs, dW=dW1, db=db1)
    # accumulate into pre-filled destinations
    g = torch.Generator().manual_seed(4)
    preW, preb = torch.randn(K, Cf, generator=g).cuda(), torch.randn(K, generator=g).cuda()
    dW2, db2 = preW.clone(), preb.clone()
    _reduce(x, dlog, loss_n, rank, K, gscale=gs, acc=1, dW=dW2, db=db2)
    # metrics only: no pooled / d logits / destinations
    out3 = torch.empty(4, device='cuda')
    from tfnas_amd import _lib
    assert _lib.lib().tfnas_cls_reduce(N, Cf, K, None, None, _lib.ptr(loss_n), _lib.ptr(rank), None, 0, None, None, _lib.ptr(out3), None,
                                       _stream()) == 0
    torch.cuda.synchronize()
    _close(dW1, 0.5 * dW0, 'dW * gscale')
    _close(db1, 0.5 * db0, 'db * gscale')
    _close(dW2, preW + 0.5 * dW0, 'dW accumulated')
    _close(db2, preb + 0.5 * db0, 'db accumulated')
    assert torch.equal(out3, out0)
    _loss_close(out0[0], loss_n.double().mean())


def test_invalid_targets_are_flagged_not_trained():
    """Targets -1 and K in a batch of 8: NaN loss_n, rank -1, zero gradient rows, invalid count 2; the other six rows are what a
    run without the bad rows gives (scale 1 / 8 in both).  The kernel never indexes by an out-of-range target (cls_kernels.hip:
    ``lt`` is read only under ``tok``, the one-hot compares against t = -1)."""
    from tfnas_amd import _lib
    N, Cf, K = 8, 64, 10
    W, b, x, t = _problem(N, Cf, K, seed=17)
    bad = [2, 5]
    t[2], t[5] = -1, K
    logits, loss_n, rank, dlog, dpool = _ce_ex(x, W, b, t, 0.1)
    out, meter = torch.empty(4, device='cuda'), torch.zeros(5, device='cuda', dtype=torch.float64)
    dW, db = torch.empty_like(W), torch.empty_like(b)
    _reduce(x, dlog, loss_n, rank, K, dW=dW, db=db, out=out, meter=meter)
    good = [i for i in range(N) if i not in bad]
    xg, tg = x[good].contiguous(), t[good].contiguous()
    lg = torch.empty(6, K, device='cuda')
    ln, rk = torch.empty(6, device='cuda'), torch.empty(6, device='cuda', dtype=torch.int32)
    dl, dp = torch.empty(6, K, device='cuda'), torch.empty(6, Cf, device='cuda')
    assert _lib.lib().tfnas_cls_ce_ex(6, Cf, K, _lib.ptr(xg), _lib.ptr(W), _lib.ptr(b), _lib.ptr(tg), 1.0 / N, 0.1, _lib.ptr(lg), _lib.ptr(ln),
                                      _lib.ptr(rk), _lib.ptr(dl), _lib.ptr(dp), _stream()) == 0
    dWg, dbg = torch.empty_like(W), torch.empty_like(b)
    _reduce(xg, dl, ln, rk, K, dW=dWg, db=dbg)
    torch.cuda.synchronize()
    assert torch.isnan(loss_n[bad]).all() and rank[bad].tolist() == [-1, -1]
    assert float(dlog[bad].abs().max()) == 0.0 and float(dpool[bad].abs().max()) == 0.0
    assert torch.isfinite(logits).all()
    for name, a, r in (('logits', logits[good], lg), ('loss_n', loss_n[good], ln), ('dlogits', dlog[good], dl), ('dpooled', dpool[good], dp)):
        assert torch.equal(a, r), name
    assert torch.equal(rank[good], rk)
    _close(dW, dWg, 'dW without the bad rows')
    _close(db, dbg, 'db without the bad rows')
    o = out.tolist()
    assert o[0] != o[0] and o[3] == 2.0                                  # the mean is NaN: loud
    assert o[1] == float((rk == 0).sum()) and o[2] == float((rk < 5).sum())
    m = meter.tolist()
    assert m[0] != m[0] and m[3:] == [8.0, 2.0]


def test_meter_accumulates_across_steps():
    from tfnas_amd.tail import DeviceMeter
    meter = DeviceMeter(torch.device('cuda'))
    tot = [0.0, 0, 0, 0]
    for step, (N, Cf, K) in enumerate([(8, 1280, 100), (128, 1280, 100), (5, 64, 7)]):
        W, b, x, t = _problem(N, Cf, K, seed=step)
        logits, loss_n, rank, _, _ = _ce_ex(x, W, b, t, 0.1, grads=False)
        _reduce(x, None, loss_n, rank, K, meter=meter.buf)
        c1, c5 = _counts(logits, t)
        assert _no_ties_with_target(logits, t)
        tot = [tot[0] + float(loss_n.double().sum()), tot[1] + c1, tot[2] + c5, tot[3] + N]
    avg, p1, p5, cnt, bad = meter.read()
    raw = meter.buf.tolist()
    assert raw[1:] == [float(tot[1]), float(tot[2]), float(tot[3]), 0.0]
    _loss_close(raw[0], tot[0], 'sum of losses')
    assert (cnt, bad) == (tot[3], 0) and p1 == 100.0 * tot[1] / cnt and p5 == 100.0 * tot[2] / cnt
    _loss_close(avg, tot[0] / cnt, 'loss average')
    meter.reset()
    assert meter.read() == (0.0, 0.0, 0.0, 0, 0)


@pytest.mark.parametrize('route', ['autograd', 'direct', 'direct_lazy'])
def test_retrain_tail_fn_under_an_upstream_gradient(route):
    """(loss * 0.5).backward() through tail.RetrainTailFn against torch autograd of the same expression: d pooled, dW, db; with
    ``direct_grads`` the weight gradients are written into the .grad views (and, with ``lazy_join``, on the side stream)."""
    from tfnas_amd import functions
    from tfnas_amd.tail import DeviceMeter, RetrainTailFn
    N, Cf, K, eps = 16, 1280, 100, 0.1
    W, b, x, t = _problem(N, Cf, K)
    Wr, br, xr = (v.clone().requires_grad_(True) for v in (W, b, x))
    lr = F.cross_entropy(F.linear(xr, Wr, br), t, label_smoothing=eps)
    (lr * 0.5).backward()
    Wm, bm, xm = (v.clone().requires_grad_(True) for v in (W, b, x))
    modes = functions.HipModes(direct_grads=route != 'autograd', lazy_join=route == 'direct_lazy')
    if route != 'autograd':
        Wm.grad, bm.grad = torch.zeros_like(Wm), torch.zeros_like(bm)
    meter = DeviceMeter(x.device)
    loss, logits, rank = RetrainTailFn.apply(xm, Wm, bm, t, eps, modes, meter)
    assert not logits.requires_grad and not rank.requires_grad and loss.requires_grad and loss.dim() == 0
    gw_ptr = None if Wm.grad is None else Wm.grad.data_ptr()
    (loss * 0.5).backward()
    if route == 'direct_lazy':
        functions.retrain_join(x.device)
    torch.cuda.synchronize()
    if gw_ptr is not None:
        assert Wm.grad.data_ptr() == gw_ptr                              # written in place
    _loss_close(loss, lr)
    _close(logits, F.linear(x, W, b), 'logits')
    _close(xm.grad, xr.grad, 'd pooled')
    _close(Wm.grad, Wr.grad, 'dW')
    _close(bm.grad, br.grad, 'db')
    c1, c5 = _counts(logits, t)
    assert meter.read()[3:] == (N, 0) and meter.buf.tolist()[1:3] == [float(c1), float(c5)]


# ---------------------------------------------------------------------------------------------------------------- model level
def _arch():
    from tfnas_amd import geometry as g
    arch = OrderedDict((st, OrderedDict((b, (i * 3 + j) % 8) for j, b in enumerate(bl) if j < 2))
                       for i, (st, bl) in enumerate(g.initial_mc_num_dddict().items()))
    return arch, g.initial_mc_num_dddict()


def _randomise(mod, gen):
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(1.0 + 0.2 * torch.rand(m.running_var.shape, generator=gen))


def _blocks(m):
    return [m.second_stem] + [b for st in m._stages() for b in st]


def _state_close(ref, got):
    for (k, a), (_, b) in zip(ref.items(), got.items()):
        err, mx = float((b.cpu().float() - a.cpu().float()).abs().max()), float(a.float().abs().max())
        assert err <= 1e-5 + 2e-3 * mx, (k, err, mx)


def test_train_step_with_fused_tail_matches_oracle(monkeypatch):
    """As tests/test_gpu_derived.py::test_derived_network_train_step_and_eval_match_oracle, with the fused tail switched on
    explicitly and the criterion confirmed eligible."""
    from tfnas_amd import model_eval as me
    monkeypatch.setattr(me, 'FUSED_TAIL', True)
    arch, mc = _arch()
    torch.manual_seed(3)
    o = orc.DerivedNetwork(50, arch, mc, 0.0, 0.2)
    _randomise(o, torch.Generator().manual_seed(1))
    m = me.Network(50, arch, mc, None, 0.0, 0.2)
    m.load_state_dict(o.state_dict())
    m = m.cuda()
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(8, 3, 96, 96, generator=gen)
    y = torch.randint(0, 50, (8,), generator=gen)
    for bo, bm in zip([o.second_stem] + o.blocks(), _blocks(m)):
        u = torch.rand(8, generator=gen)
        bo.drop_u, bm.drop_u = u, u
    oo = torch.optim.SGD(o.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
    mo = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
    o.train()
    logits_o = o(x)
    lo = orc.label_smooth_loss(logits_o, y, 50, 0.1)
    oo.zero_grad(); lo.backward()
    torch.nn.utils.clip_grad_norm_(o.parameters(), 5.0); oo.step()
    crit = me.CrossEntropyLabelSmooth(50, 0.1)
    assert me.fused_tail_eligible(m, crit)
    lm, logits_m = me.train_step(m, x.cuda(), y.cuda(), crit, mo, 5.0)
    print('loss oracle %.7f fused %.7f' % (float(lo), float(lm)))
    assert abs(float(lo) - float(lm)) < 1e-4
    assert logits_m.shape == (8, 50) and not logits_m.requires_grad
    # (the returned logits: the bar tests/test_gpu_derived.py holds the network's logits to against the oracle)
    assert torch.allclose(logits_m.cpu(), logits_o.detach(), atol=1e-3, rtol=1e-3), float((logits_m.cpu() - logits_o).abs().max())
    _state_close(o.state_dict(), m.state_dict())


def test_train_step_fused_tail_equals_torch_tail_with_dropout(monkeypatch):
    """dropout_rate = 0.2: dropout stays the torch op at the same point of the RNG stream, so under one torch.manual_seed the masks of
    the two routes agree; loss and state after one step within the training-step bars."""
    from tfnas_amd import model_eval as me
    arch, mc = _arch()
    torch.manual_seed(8)
    base = me.Network(50, arch, mc, None, 0.2, 0.2)
    _randomise(base, torch.Generator().manual_seed(6))
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(8, 3, 96, 96, generator=gen).cuda()
    y = torch.randint(0, 50, (8,), generator=gen).cuda()
    us = [torch.rand(8, generator=gen) for _ in range(64)]
    res = []
    for on in (False, True):
        monkeypatch.setattr(me, 'FUSED_TAIL', on)
        m = me.Network(50, arch, mc, None, 0.2, 0.2)
        m.load_state_dict(base.state_dict())
        m = m.cuda()
        for blk, u in zip(_blocks(m), us):
            blk.drop_u = u
        opt = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
        torch.manual_seed(31)
        loss, _ = me.train_step(m, x, y, me.CrossEntropyLabelSmooth(50, 0.1), opt, 5.0)
        torch.cuda.synchronize()
        res.append((float(loss), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    print('loss torch tail %.7f fused tail %.7f' % (res[0][0], res[1][0]))
    assert abs(res[0][0] - res[1][0]) < 1e-4
    _state_close(res[0][1], res[1][1])


def test_direct_lazy_routes_bit_identical_with_fused_tail(monkeypatch):
    """Three steps with the fused tail over the four DIRECT_GRADS / LAZY_JOIN combinations: in-place classifier gradients and the
    side-stream launch are plumbing only -- bit-identical parameters, momentum and running statistics."""
    from tfnas_amd import model_eval as me
    monkeypatch.setattr(me, 'FUSED_TAIL', True)
    arch, mc = _arch()

    def run(direct, lazy):
        monkeypatch.setattr(me, 'DIRECT_GRADS', direct)
        monkeypatch.setattr(me, 'LAZY_JOIN', lazy)
        torch.manual_seed(5)
        m = me.Network(50, arch, mc, None, 0.0, 0.2).cuda()
        opt = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
        crit = me.CrossEntropyLabelSmooth(50, 0.1)
        assert me.fused_tail_eligible(m, crit)
        gen = torch.Generator().manual_seed(11)
        for _ in range(3):
            x = torch.randn(16, 3, 128, 128, generator=gen).cuda()
            y = torch.randint(0, 50, (16,), generator=gen).cuda()
            for b in _blocks(m):
                b.drop_u = torch.rand(16, generator=gen)
            me.train_step(m, x, y, crit, opt, 5.0)
        torch.cuda.synchronize()
        out = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        out.update({'mom%d' % i: opt.state[p]['momentum_buffer'].detach().cpu().clone() for i, p in enumerate(m.parameters())})
        return out

    base = run(False, False)
    for direct, lazy in ((True, False), (False, True), (True, True)):
        other = run(direct, lazy)
        assert base.keys() == other.keys()
        for k in base:
            assert torch.equal(base[k], other[k]), (direct, lazy, k)


def test_validate_routes_agree(monkeypatch, tmp_path):
    """model_eval.validate on the forward-only kernel against the torch route: top-1 / top-5 equal as counts, loss within the loss
    tolerance, for the default criterion and for a label-smoothed nn.CrossEntropyLoss; run_retrain over a training queue with an
    out-of-range label raises ValueError naming the count (fused route: the label is flagged by the kernel, never indexed)."""
    from tfnas_amd import model_eval as me
    arch, mc = _arch()
    torch.manual_seed(13)
    m = me.Network(50, arch, mc, None, 0.2, 0.2)
    _randomise(m, torch.Generator().manual_seed(2))
    m = m.cuda()
    gen = torch.Generator().manual_seed(7)
    queue = [(torch.randn(n, 3, 96, 96, generator=gen), torch.randint(0, 50, (n,), generator=gen)) for n in (8, 8, 5)]
    # make some hits: the labels of the first batch are the eval-mode argmax / third-ranked classes
    m.eval()
    with torch.no_grad():
        order = m(queue[0][0].cuda()).argsort(dim=1, descending=True).cpu()
    queue[0][1][0::2] = order[0::2, 0]
    queue[0][1][1::2] = order[1::2, 2]
    total = 21
    for crit in (None, torch.nn.CrossEntropyLoss(label_smoothing=0.1)):
        got = []
        for on in (False, True):
            monkeypatch.setattr(me, 'FUSED_TAIL', on)
            assert me.fused_tail_eligible(m, crit, validating=True)
            got.append(me.validate(m, queue, crit))
        (t1a, t5a, la), (t1b, t5b, lb) = got
        print('torch route', got[0], 'fused route', got[1])
        assert round(t1a * total / 100.0) == round(t1b * total / 100.0) >= 4
        assert round(t5a * total / 100.0) == round(t5b * total / 100.0) >= 8
        _loss_close(lb, la, 'validation loss')
    # frozen classifier: still the fused route in validate
    for p in m.classifier.parameters():
        p.requires_grad_(False)
    assert me.fused_tail_eligible(m, None, validating=True) and not me.fused_tail_eligible(m, me.CrossEntropyLabelSmooth(50, 0.1))
    t1c, t5c, lc = me.validate(m, queue)
    assert (t1c, t5c) == got[1][:2]
    for p in m.classifier.parameters():
        p.requires_grad_(True)

    monkeypatch.setattr(me, 'FUSED_TAIL', True)
    m2 = me.Network(10, arch, mc, None, 0.1, 0.1)
    assert me.fused_tail_eligible(m2.cuda(), me.CrossEntropyLabelSmooth(10, 0.1))
    g2 = torch.Generator().manual_seed(1)
    labels = torch.randint(0, 10, (8,), generator=g2)
    labels[3] = 10

    def train_queue(epoch):
        return [(torch.randn(8, 3, 64, 64, generator=g2), torch.randint(0, 10, (8,), generator=g2)),
                (torch.randn(8, 3, 64, 64, generator=g2), labels)]
    with pytest.raises(ValueError, match=r'\b1 training target'):
        me.run_retrain(str(tmp_path / 'rt'), m2, train_queue, lambda e: [], epochs=1, lr=0.05, log=lambda s: None)


def test_ineligible_criteria_and_frozen_classifier_take_the_torch_route(monkeypatch):
    from tfnas_amd import model_eval as me
    from tfnas_amd import tail
    monkeypatch.setattr(me, 'FUSED_TAIL', True)
    arch, mc = _arch()
    torch.manual_seed(21)
    m = me.Network(50, arch, mc, None, 0.0, 0.0).cuda()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(8, 3, 96, 96, generator=gen).cuda()
    y = torch.randint(0, 50, (8,), generator=gen).cuda()
    calls = []
    real = tail.RetrainTailFn.apply
    monkeypatch.setattr(tail.RetrainTailFn, 'apply', staticmethod(lambda *a: (calls.append(1), real(*a))[1]))
    good = [me.CrossEntropyLabelSmooth(50, 0.1), torch.nn.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(label_smoothing=0.2)]
    bad = [torch.nn.CrossEntropyLoss(weight=torch.ones(50, device='cuda')), torch.nn.CrossEntropyLoss(reduction='sum'),
           torch.nn.CrossEntropyLoss(ignore_index=3), me.CrossEntropyLabelSmooth(51, 0.1), F.cross_entropy,
           lambda lg, t: F.cross_entropy(lg, t)]
    opt = torch.optim.SGD(m.parameters(), 0.01, momentum=0.9)
    for crit in good:
        assert me.fused_tail_eligible(m, crit)
    loss, _ = me.train_step(m, x, y, good[0], opt, 5.0)
    assert len(calls) == 1 and torch.isfinite(loss)
    for crit in bad:
        assert not me.fused_tail_eligible(m, crit), crit
        loss, logits = me.train_step(m, x, y, crit, opt, 5.0)
        assert torch.isfinite(loss) and logits.shape == (8, 50)
    assert len(calls) == 1                                               # none of them went through the fused tail
    assert not me.fused_tail_eligible(torch.nn.Sequential(m), good[0])    # a wrapper with a forward of its own
    assert me.fused_tail_eligible(torch.nn.DataParallel(m, device_ids=[0]), good[0])
    m.classifier.linear.weight.requires_grad_(False)
    assert not me.fused_tail_eligible(m, good[0]) and not me.fused_tail_eligible(m, None, validating=True)
    sub = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], 0.01, momentum=0.9)
    before = m.classifier.linear.weight.detach().clone()
    loss, _ = me.train_step(m, x, y, good[0], sub, 5.0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and len(calls) == 1 and torch.equal(m.classifier.linear.weight, before)
