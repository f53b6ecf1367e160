"""GPU: the search loop's device-side meters -- tfnas_cls_wgrad_ex (csrc/cls_kernels.hip) through the C ABI, and tail.SearchMeter
riding the weight / architecture steps (tfnas_amd/search.py: w_step / a_step with ``meter=``).

Reference: train_search.py:318-432 -- ``objs_w.update(loss_w.item(), n)``, ``top1 / top5.update(prec.item(), n)`` on the gumbel path's
logits, ``objs_a`` / ``objs_l`` in the architecture step, AverageMeter of tools/utils.py:37-58.  Top-k follows the rank rule of
include/tfnas_hip.h (rank = #{k: l_k > l_t} + #{k < t: l_k == l_t}, top-k is rank < k), computed here in numpy from the logits, not
with torch.topk (which promises no order among ties)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rank_np(logits, target):
    """The header's rank rule; -1 for a target outside [0, K)."""
    lg = np.asarray(logits, dtype=np.float32)
    out = []
    for row, t in zip(lg, np.asarray(target).tolist()):
        if not 0 <= t < row.size:
            out.append(-1)
            continue
        out.append(int((row > row[t]).sum() + (row[:t] == row[t]).sum()))
    return np.asarray(out, dtype=np.int64)


def _counts(rank, N):
    return [float(((rank >= 0) & (rank < 1)).sum()), float(((rank >= 0) & (rank < 5)).sum()), float(N), float((rank < 0).sum())]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tail_inputs(N, Cf, K, npath, seed, target=None, W=None, b=None):
    """Per path: pooled, logits, loss_n, dlogits from the per-image launch -- path 0 by tfnas_cls_ce_ex (eps = 0: it yields rank),
    path 1 by tfnas_cls_ce, which is what BiTail.run enqueues with a meter."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(seed)
    W = ((torch.randn(K, Cf, generator=g) * 0.3) if W is None else W).cuda()
    b = ((torch.randn(K, generator=g) * 0.1) if b is None else b).cuda()
    target = (torch.randint(0, K, (N,), generator=g) if target is None else target).cuda()
    paths, rank = [], torch.full((N,), -7, device='cuda', dtype=torch.int32)
    for p in range(npath):
        x = torch.randn(N, Cf, generator=g).cuda()
        logits, dlog = torch.empty(N, K, device='cuda'), torch.empty(N, K, device='cuda')
        loss_n, dpool = torch.empty(N, device='cuda'), torch.empty(N, Cf, device='cuda')
        if p == 0:
            rc = lib.tfnas_cls_ce_ex(N, Cf, K, _lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(target), 1.0 / N, 0.0, _lib.ptr(logits),
                                     _lib.ptr(loss_n), _lib.ptr(rank), _lib.ptr(dlog), _lib.ptr(dpool), _stream())
        else:
            rc = lib.tfnas_cls_ce(N, Cf, K, _lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(target), 1.0 / N, _lib.ptr(logits),
                                  _lib.ptr(loss_n), _lib.ptr(dlog), _lib.ptr(dpool), _stream())
        assert rc == 0
        paths.append(dict(pooled=x, logits=logits, loss_n=loss_n, dlogits=dlog))
    torch.cuda.synchronize()
    return paths, rank, target


def _wgrad(paths, N, Cf, K, rank=None, meter=None, ex=True):
    """One summation launch into fresh (poisoned) outputs -> (rc, dW, db, loss)."""
    from tfnas_amd import _lib
    lib = _lib.lib()
    arr = lambda key: _lib.raw_array([p[key].data_ptr() for p in paths])
    dW = torch.full((K, Cf), float('nan'), device='cuda')
    db = torch.full((K,), float('nan'), device='cuda')
    loss = torch.full((), float('nan'), device='cuda')
    if ex:
        rc = lib.tfnas_cls_wgrad_ex(len(paths), N, Cf, K, arr('pooled'), arr('dlogits'), arr('loss_n'), _lib.ptr(rank), 1.0 / N,
                                    _lib.ptr(dW), _lib.ptr(db), _lib.ptr(loss), _lib.ptr(meter), _stream())
    else:
        rc = lib.tfnas_cls_wgrad(len(paths), N, Cf, K, arr('pooled'), arr('dlogits'), arr('loss_n'), 1.0 / N, _lib.ptr(dW),
                                 _lib.ptr(db), _lib.ptr(loss), _stream())
    torch.cuda.synchronize()
    return rc, dW, db, loss


@pytest.mark.parametrize('npath', [1, 2])
@pytest.mark.parametrize('Cf,K', [(4, 1), (260, 3), (64, 6), (1280, 100)])
@pytest.mark.parametrize('N', [1, 5, 63, 65, 130])
def test_wgrad_ex_is_bit_identical_to_wgrad_and_counts_exactly(N, Cf, K, npath):
    """N below, at and above one wave of the lane-strided loop; K not a multiple of 4, K < 5 (every valid rank is a top-5 hit), two
    feature tiles (C = 260, 1280); one and two paths."""
    paths, rank, target = _tail_inputs(N, Cf, K, npath, 1000 * N + K + npath)
    rc, dW0, db0, loss0 = _wgrad(paths, N, Cf, K, ex=False)
    assert rc == 0
    # meter == NULL: the old call, rank0 ignored (given or not)
    for rk in (None, rank):
        rc, dW, db, loss = _wgrad(paths, N, Cf, K, rank=rk)
        assert rc == 0 and torch.equal(dW, dW0) and torch.equal(db, db0) and torch.equal(loss, loss0)
    meter = torch.zeros(5, device='cuda', dtype=torch.float64)
    rc, dW, db, loss = _wgrad(paths, N, Cf, K, rank=rank, meter=meter)
    assert rc == 0 and torch.equal(dW, dW0) and torch.equal(db, db0) and torch.equal(loss, loss0)
    rk = rank.cpu().numpy()
    assert (rk == _rank_np(paths[0]['logits'].cpu().numpy(), target.cpu().numpy())).all()
    want_sum = float(np.sum(np.concatenate([p['loss_n'].cpu().numpy().astype(np.float64) for p in paths])))
    got = meter.tolist()
    assert got[1:] == _counts(rk, N), (got, _counts(rk, N))
    assert abs(got[0] - want_sum) <= 1e-12 * abs(want_sum), (got[0], want_sum)
    if K < 5:
        assert got[2] == N
    # a second launch on the same meter adds to it, and is bit-identical in what it stores
    rc, dW2, db2, loss2 = _wgrad(paths, N, Cf, K, rank=rank, meter=meter)
    assert rc == 0 and torch.equal(dW2, dW0) and torch.equal(db2, db0) and torch.equal(loss2, loss0)
    assert meter.tolist() == [2.0 * v for v in got]


def test_wgrad_ex_flags_invalid_targets_like_the_retrain_meter():
    """One target == K and one == -1 among valid ones: tfnas_cls_ce_ex marks them (rank -1, loss_n NaN), the meter counts two invalid
    targets and its loss sum is NaN -- the semantics of tfnas_cls_reduce's meter.  Kernel level only."""
    N, Cf, K = 65, 64, 6
    g = torch.Generator().manual_seed(77)
    target = torch.randint(0, K, (N,), generator=g)
    target[3], target[64] = K, -1
    paths, rank, _ = _tail_inputs(N, Cf, K, 2, 78, target=target)
    rk = rank.cpu().numpy()
    assert rk[3] == -1 and rk[64] == -1 and (np.delete(rk, [3, 64]) >= 0).all()
    rc, dW0, db0, _l = _wgrad(paths, N, Cf, K, ex=False)
    meter = torch.zeros(5, device='cuda', dtype=torch.float64)
    rc, dW, db, loss = _wgrad(paths, N, Cf, K, rank=rank, meter=meter)
    assert rc == 0 and torch.equal(dW, dW0) and torch.equal(db, db0)
    got = meter.tolist()
    assert got[4] == 2.0 and got[0] != got[0]
    assert got[1:] == _counts(rk, N)
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())      # (invalid rows carry zero gradient)


@pytest.mark.parametrize('invalid', [False, True])
@pytest.mark.parametrize('Cf,K', [(4, 1), (260, 3), (64, 6)])
@pytest.mark.parametrize('N', [1, 63, 65, 130])
def test_reduce_and_wgrad_ex_of_one_path_share_their_sums_bit_for_bit(N, Cf, K, invalid):
    """The three summation kernels call ONE row and ONE tile: for a single path tfnas_cls_reduce(gscale = NULL, accumulate = 0) and
    tfnas_cls_wgrad_ex(npath = 1) on the same pooled / dlogits / loss_n / rank store bit-identical dW and db and, from the same
    meter contents, leave bit-identical five doubles (compared as bit patterns: with an out-of-range label the loss sum is NaN).
    N: a partial wave, just over one wave, more than two lane strides; (C, K): the minimum, a ragged feature tile with K % 4 != 0,
    K > 5."""
    from tfnas_amd import _lib
    g = torch.Generator().manual_seed(31 * N + K)
    target = torch.randint(0, K, (N,), generator=g)
    if invalid:
        target[N // 2] = K
    paths, rank, _ = _tail_inputs(N, Cf, K, 1, 500 * N + K, target=target)
    start = torch.tensor([0.5, 3.0, 7.0, 11.0, 2.0], device='cuda', dtype=torch.float64)
    m_w, m_r = start.clone(), start.clone()
    rc, dW_w, db_w, _loss = _wgrad(paths, N, Cf, K, rank=rank, meter=m_w)
    assert rc == 0
    p = paths[0]
    dW_r, db_r = torch.full((K, Cf), float('nan'), device='cuda'), torch.full((K,), float('nan'), device='cuda')
    rc = _lib.lib().tfnas_cls_reduce(N, Cf, K, _lib.ptr(p['pooled']), _lib.ptr(p['dlogits']), _lib.ptr(p['loss_n']), _lib.ptr(rank),
                                     None, 0, _lib.ptr(dW_r), _lib.ptr(db_r), None, _lib.ptr(m_r), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(dW_r, dW_w) and torch.equal(db_r, db_w) and bool(torch.isfinite(dW_r).all())
    assert torch.equal(m_r.view(torch.int64), m_w.view(torch.int64)), (m_r.tolist(), m_w.tolist())
    got = m_r.tolist()
    assert [v - s for v, s in zip(got[1:], start.tolist()[1:])] == _counts(rank.cpu().numpy(), N)
    assert got[4] == 2.0 + int(invalid) and (got[0] != got[0]) == invalid


def test_wgrad_ex_counts_tied_rows_by_the_lower_index_rule():
    """W = 0: every row's logits are the bias, with ties.  Expected counts from the header's formula: among equal logits the lower
    class index ranks first."""
    N, Cf, K = 12, 8, 6
    b = torch.tensor([1., 1., 0., 1., 2., 2.])
    target = torch.tensor([0, 1, 2, 3, 4, 5] * 2)
    paths, rank, _ = _tail_inputs(N, Cf, K, 1, 5, target=target, W=torch.zeros(K, Cf), b=b)
    assert rank.tolist() == [2, 3, 5, 4, 0, 1] * 2
    assert (rank.cpu().numpy() == _rank_np(np.tile(b.numpy(), (N, 1)), target.numpy())).all()
    meter = torch.zeros(5, device='cuda', dtype=torch.float64)
    rc, _dW, _db, _l = _wgrad(paths, N, Cf, K, rank=rank, meter=meter)
    assert rc == 0
    assert meter.tolist()[1:] == [2.0, 10.0, 12.0, 0.0]       # top-1: the two rows with target 4 (not 5, its tie); top-5: all but rank 5


def test_wgrad_ex_refuses_a_meter_without_rank():
    N, Cf, K = 5, 64, 6
    paths, rank, _ = _tail_inputs(N, Cf, K, 2, 9)
    meter = torch.zeros(5, device='cuda', dtype=torch.float64)
    rc, dW, _db, _l = _wgrad(paths, N, Cf, K, rank=None, meter=meter)
    assert rc == -2                                                            # TFNAS_ENULL, before any launch
    assert meter.tolist() == [0.0] * 5 and bool(torch.isnan(dW).all())


# ---- steps ---------------------------------------------------------------------------------------------------------------------------

NUM_CLASSES = 8


def _states(count, B=8, seed=3):
    """``count`` identical (model, state, opt_w, opt_a) at 8 classes -- hits and misses both occur -- and six batches."""
    from tfnas_amd import Network, load_lat_lookup, geometry, search
    lut = load_lat_lookup('gpu')
    out = []
    for _ in range(count):
        torch.manual_seed(seed)
        m = Network(NUM_CLASSES, geometry.initial_mc_num_dddict(), lut).cuda()
        m.set_temperature(5.0)
        st = search.SearchState(m)
        ow, oa = search.make_optimizers(m)
        out.append((m, st, ow, oa))
    g = torch.Generator().manual_seed(11)
    batches = [(torch.randn(B, 3, 224, 224, generator=g).cuda(),          # (the latency table is keyed by the 224 x 224 geometry)
                torch.randint(0, NUM_CLASSES, (B,), generator=g).cuda()) for _ in range(6)]
    return out, batches


def _hits(logits, target, k):
    return int((_rank_np(logits.cpu().numpy(), target.cpu().numpy()) < k).sum())


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_a_meter_does_not_change_the_weight_step():
    """One bi-sampling w-step from identical state, with a meter and without: every parameter and the momentum arena bit-identical
    (tfnas_cls_ce_ex(eps = 0) == tfnas_cls_ce, tfnas_cls_wgrad_ex == tfnas_cls_wgrad in what they store)."""
    from tfnas_amd import search
    from tfnas_amd.tail import SearchMeter
    ((ma, sa, owa, _), (mb, sb, owb, _)), batches = _states(2)
    x, y = batches[0]
    meter = SearchMeter(x.device)
    outs = []
    for st, ow, mt in ((sa, owa, meter), (sb, owb, None)):
        noise = search.NoiseSource(5)
        outs.append(search.w_step(st, x, y, ow, 5.0, noise.exp(x.device), noise.rand_pos(), meter=mt))
    torch.cuda.synchronize()
    assert sa._bitail is not None and sa._bitail.a is not None                # (the fused tail ran)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for (ka, pa), (kb, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert ka == kb and torch.equal(pa, pb), ka
    assert torch.equal(sa.arena.m, sb.arena.m)
    m = meter.read()
    assert m['images_w'] == 8 and m['invalid'] == 0 and _rel(m['objs_w'], float(outs[0][0])) <= 1e-6


def test_meter_equals_a_host_recomputation_of_the_reference_meters():
    """Four w-steps and two alpha-steps (the order of train_w_arch: an alpha-step after every even w-step) with a meter; every
    step's returned loss / logits / loss_a / loss_l pulled to the host afterwards and run through the reference's AverageMeter
    arithmetic.  Counts exact; averages within 1e-6 relative (the returned losses are fp32 roundings of the per-image sums the
    meter holds in double)."""
    from tfnas_amd import search
    from tfnas_amd.tail import SearchMeter
    ((_, st, ow, oa),), batches = _states(1)
    dev = batches[0][0].device
    meter = SearchMeter(dev)
    noise = search.NoiseSource(5)
    rec_w, rec_a = [], []
    for step in range(4):
        x, y = batches[step]
        loss, logits = search.w_step(st, x, y, ow, 5.0, noise.exp(dev), noise.rand_pos(), meter=meter)
        rec_w.append((loss, logits, y))
        if step % 2 == 0:
            xa, ya = batches[4 + step // 2]
            la, ll, _lat, _ = search.a_step(st, xa, ya, oa, 15.0, 0.1, 5.0, noise.exp(dev), meter=meter)
            rec_a.append((la, ll, ya.size(0)))
    m = meter.read()
    objs_w, top1, top5, objs_a, objs_l = (search.AverageMeter() for _ in range(5))
    c1 = c5 = 0
    for loss, logits, y in rec_w:
        n = y.size(0)
        h1, h5 = _hits(logits, y, 1), _hits(logits, y, 5)
        c1, c5 = c1 + h1, c5 + h5
        objs_w.update(float(loss), n)
        top1.update(100.0 * h1 / n, n)
        top5.update(100.0 * h5 / n, n)
    for la, ll, n in rec_a:
        objs_a.update(float(la), n)
        objs_l.update(float(ll), n)
    print('host: top-1 hits %d, top-5 hits %d of %d; objs_w %.9g objs_a %.9g objs_l %.9g; meter %r' % (
        c1, c5, int(top1.cnt), objs_w.avg, objs_a.avg, objs_l.avg, m))
    assert 0 < c1 < c5 < top1.cnt == 32                                    # (hits and misses both occur)
    w = meter.buf.tolist()
    assert w[1:5] == [float(c1), float(c5), 32.0, 0.0]
    assert m['images_w'] == 32 and m['images_a'] == 16 and m['invalid'] == 0
    assert abs(m['top1'] - top1.avg) <= 1e-9 and abs(m['top5'] - top5.avg) <= 1e-9
    assert 0 <= m['top1_a'] <= m['top5_a'] <= 100
    assert _rel(m['objs_w'], objs_w.avg) <= 1e-6, (m['objs_w'], objs_w.avg)
    assert _rel(m['objs_a'], objs_a.avg) <= 1e-6, (m['objs_a'], objs_a.avg)
    assert _rel(m['objs_l'], objs_l.avg) <= 1e-6, (m['objs_l'], objs_l.avg)


def test_torch_op_routes_fill_the_meter_like_the_fused_route(monkeypatch):
    """Three identical states, one alpha-step then one w-step each (teacher-forced: an alpha-step changes no weight, so the w-steps
    start from the same weights and sample the same gumbel path): A on the fused tails, B with FUSED_TAIL off (SearchMeter.add_a /
    add_w after the torch classifier + loss), C's w-step without bi-sampling (the warm-up step: add_w, one path).
    Counts of B and C equal A's; B's sums agree with A's within 1e-5 relative (the torch tail's loss differs from the fused one by
    the tolerance tests/test_gpu_tail.py uses); C's loss is the gumbel path's alone, so its sum is checked against its own returned
    loss (1e-6) and must lie below A's two-path sum."""
    from tfnas_amd import search
    from tfnas_amd.tail import SearchMeter
    runs, batches = _states(3)
    dev = batches[0][0].device
    (xa, ya), (xw, yw) = batches[4], batches[0]
    meters, ret = [], []
    for (m, st, ow, oa), fused, bi in zip(runs, (True, False, True), (True, True, False)):
        monkeypatch.setattr(search, 'FUSED_TAIL', fused)
        meter, noise = SearchMeter(dev), search.NoiseSource(5)
        la, ll, _lat, _ = search.a_step(st, xa, ya, oa, 15.0, 0.1, 5.0, noise.exp(dev), meter=meter)
        if bi:
            lw, lg = search.w_step(st, xw, yw, ow, 5.0, noise.exp(dev), noise.rand_pos(), meter=meter)
        else:
            lw, lg = search.w_step(st, xw, yw, ow, 5.0, noise.exp(dev), bi_sampling=False, meter=meter)
        meters.append(meter.buf.tolist())
        ret.append((float(lw), float(la), float(ll)))
    a, b, c = meters
    print('fused %r\ntorch tail %r\none path %r\nreturned %r' % (a, b, c, ret))
    assert a[1:5] == b[1:5] == c[1:5] and a[3] == 8.0                       # w block: hits, images, invalid
    assert a[6:10] == b[6:10] == c[6:10] and a[8] == 8.0                    # a block
    for i in (0, 5, 10):
        assert _rel(b[i], a[i]) <= 1e-5, (i, a[i], b[i])
    assert c[5] == a[5] and c[10] == a[10]                                  # (C's alpha-step ran the same fused route)
    assert _rel(c[0], 8.0 * ret[2][0]) <= 1e-6 and 0 < c[0] < a[0]
    assert _rel(a[0], 8.0 * ret[0][0]) <= 1e-6
