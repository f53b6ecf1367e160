"""Host-side checks of the search loop's meters (tfnas_amd/tail.py: SearchMeter, target_rank; tfnas_amd/epoch.py: train_stats) and
of the C ABI of tfnas_cls_wgrad_ex -- no GPU.

Reference: train_search.py:318-432 keeps AverageMeters (tools/utils.py:37-58) objs_w / top1 / top5 / objs_a / objs_l, updated with
``.item()`` values and the batch size; top-k comes from tools/utils.py:61-74.  The expectations below are that arithmetic written out
by hand, with top-k by the rank rule of include/tfnas_hip.h (rank = #{k: l_k > l_t} + #{k < t: l_k == l_t}; top-k is rank < k)."""
import ctypes as C
import os
import re
import socket

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
KEYS = ('objs_w', 'top1', 'top5', 'images_w', 'objs_a', 'objs_l', 'top1_a', 'top5_a', 'images_a', 'invalid')


class _Avg:
    def __init__(self):
        self.sum = self.cnt = 0.0

    def update(self, val, n):
        self.sum += val * n
        self.cnt += n

    @property
    def avg(self):
        return self.sum / self.cnt


def _rank(row, t):
    return sum(1 for k, v in enumerate(row) if v > row[t] or (v == row[t] and k < t))


def _prec(logits, target, k):
    """tools/utils.py:61-74: hits among the top k, in percent of the batch."""
    rows = logits.tolist()
    return 100.0 * sum(1 for r, t in zip(rows, target.tolist()) if _rank(r, t) < k) / len(rows)


def test_target_rank_follows_the_header_rule_on_ties_and_invalid_targets():
    from tfnas_amd.tail import target_rank
    lg = torch.tensor([[1., 1., 0., 1., 2., 2.]] * 8)
    t = torch.tensor([0, 1, 2, 3, 4, 5, 6, -1])
    rank, valid = target_rank(lg, t)
    assert rank.tolist() == [2, 3, 5, 4, 0, 1, -1, -1]
    assert valid.tolist() == [True] * 6 + [False] * 2


def test_search_meter_equals_a_hand_written_average_meter_loop():
    from tfnas_amd.tail import SearchMeter
    g = torch.Generator().manual_seed(5)
    meter = SearchMeter('cpu')
    assert meter.read() == dict(zip(KEYS, (0.0, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0)))
    objs_w, top1, top5, objs_a, objs_l, top1_a, top5_a = (_Avg() for _ in range(7))
    for step, n in enumerate((3, 8, 1, 6)):
        logits = torch.randn(n, 7, generator=g)
        target = torch.randint(0, 7, (n,), generator=g)
        loss = torch.rand((), generator=g) * 3
        meter.add_w(loss, logits, target)
        objs_w.update(loss.item(), n)
        top1.update(_prec(logits, target, 1), n)
        top5.update(_prec(logits, target, 5), n)
        if step % 2 == 0:
            la, ll = torch.rand((), generator=g), torch.rand(1, generator=g) * 0.1
            lg_a = torch.randn(n, 7, generator=g)
            meter.add_a(la, ll, n, lg_a, target)
            objs_a.update(la.item(), n)
            objs_l.update(ll.item(), n)
            top1_a.update(_prec(lg_a, target, 1), n)
            top5_a.update(_prec(lg_a, target, 5), n)
    m = meter.read()
    assert tuple(m) == KEYS
    assert m['images_w'] == 18 and m['images_a'] == 4 and m['invalid'] == 0
    want = dict(objs_w=objs_w.avg, top1=top1.avg, top5=top5.avg, objs_a=objs_a.avg, objs_l=objs_l.avg, top1_a=top1_a.avg,
                top5_a=top5_a.avg)
    for k, v in want.items():                     # (doubles summed in another order: 1e-12 relative)
        assert abs(m[k] - v) <= 1e-12 * abs(v), (k, m[k], v)
    assert 0 < m['top1'] < m['top5'] < 100        # (the data exercises hits and misses)
    # the fused architecture tail adds its own block: add_a(None, ...) only adds n * loss_l
    before = meter.buf.clone()
    meter.add_a(None, torch.tensor(0.25), 4)
    assert torch.equal(meter.buf[:10], before[:10]) and float(meter.buf[10] - before[10]) == 1.0
    # without logits: loss and images only
    meter.add_a(torch.tensor(2.0), torch.tensor(0.0), 2)
    assert (meter.buf[5:10] - before[5:10]).tolist() == [4.0, 0.0, 0.0, 2.0, 0.0]
    meter.reset()
    assert meter.read()['images_w'] == 0 and float(meter.buf.abs().sum()) == 0.0


def test_device_meter_and_search_meter_share_one_block_arithmetic():
    """DeviceMeter.add and SearchMeter.add_w fed the same (loss, logits, target) leave the same five numbers, with hits by the
    rank rule: a target tied with a LOWER-indexed class misses top-1, one tied with a HIGHER-indexed class hits, and a target equal
    to K is counted as invalid (and is no hit)."""
    from tfnas_amd.tail import DeviceMeter, SearchMeter
    logits = torch.tensor([[1., 0., 1., 0., -1., -2., -3.],       # target 2 tied with class 0: rank 1
                           [0., 2., 0., 2., -1., -2., -3.],       # target 1 tied with class 3: rank 0
                           [3., 2., 1., 0., -1., -2., -3.],       # target 7 == K
                           [6., 5., 4., 3., 2., 1., 0.]])         # target 5: rank 5, outside the top 5
    target = torch.tensor([2, 1, 7, 5])
    loss = torch.tensor(0.75)
    dm, sm = DeviceMeter('cpu'), SearchMeter('cpu')
    dm.add(loss, logits, target)
    sm.add_w(loss, logits, target)
    assert dm.buf.tolist() == [3.0, 1.0, 2.0, 4.0, 1.0]            # {n * loss, top-1, top-5, images, invalid}
    assert torch.equal(dm.buf, sm.buf[SearchMeter.W:SearchMeter.W + 5]) and float(sm.buf[5:].abs().sum()) == 0.0
    assert dm.read() == (0.75, 25.0, 50.0, 4, 1)
    m = sm.read()
    assert (m['objs_w'], m['top1'], m['top5'], m['images_w'], m['invalid']) == dm.read()


def test_epoch_end_check_raises_on_invalid_targets_and_fills_the_stats():
    from tfnas_amd.epoch import train_stats
    from tfnas_amd.tail import SearchMeter
    meter = SearchMeter('cpu')
    logits = torch.tensor([[0., 1., 2.], [2., 1., 0.], [0., 2., 1.], [1., 0., 2.]])
    meter.add_w(torch.tensor(1.5), logits, torch.tensor([2, 1, 0, 2]))
    meter.add_a(torch.tensor(0.5), torch.tensor(0.125), 4, logits, torch.tensor([2, 0, 1, 1]))
    stats = train_stats({}, meter.read(), 3, False, 3)
    assert stats == dict(train_top1=50.0, train_top5=100.0, train_objs_w=1.5)
    stats = train_stats({}, meter.read(), 3, True, 3)
    assert stats == dict(train_top1=50.0, train_top5=100.0, train_objs_w=1.5, train_objs_a=0.5, train_objs_l=0.125)
    meter.add_w(torch.tensor(1.5), logits, torch.tensor([3, -1, 0, 2]))
    assert meter.read()['invalid'] == 2
    with pytest.raises(ValueError, match=r'epoch 3 saw 2 target\(s\) outside \[0, 3\)'):
        train_stats({}, meter.read(), 3, True, 3)


def test_steps_feed_a_host_meter_on_the_cpu_oracle_model():
    """The model-agnostic step logic (what tests/test_dp_gloo.py drives) with ``meter=``: a bi-sampling w-step, an alpha-step and a
    one-path w-step of the CPU oracle model add what a host AverageMeter loop over the returned values holds -- and with
    ``meter=None`` nothing else changes (same returned loss from an identical second model)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import tfnas_oracle as orc
    from tfnas_amd import search
    from tfnas_amd.latency import load_lat_lookup
    from tfnas_amd.tail import SearchMeter
    g = torch.Generator().manual_seed(100)
    x, y = torch.randn(4, 3, 224, 224, generator=g), torch.randint(0, 8, (4,), generator=g)
    first = []
    for meter in (SearchMeter('cpu'), None):
        torch.manual_seed(2)
        model = orc.Network(8, orc.initial_mc_num_dddict(), load_lat_lookup('gpu'))
        model.set_temperature(5.0)
        state = search.SearchState(model)
        opt_w, opt_a = search.make_optimizers(model)
        noise = search.NoiseSource(7)
        lw, lg = search.w_step(state, x, y, opt_w, 5.0, noise.exp('cpu'), noise.rand_pos(), meter=meter)
        first.append(float(lw))
        if meter is None:
            break
        la, ll, _lat, _ = search.a_step(state, x, y, opt_a, 15.0, 0.1, 5.0, noise.exp('cpu'), meter=meter)
        lw2, lg2 = search.w_step(state, x, y, opt_w, 5.0, noise.exp('cpu'), bi_sampling=False, meter=meter)
        objs_w, top1, top5 = _Avg(), _Avg(), _Avg()
        for loss, logits in ((lw, lg), (lw2, lg2)):
            objs_w.update(loss.item(), 4)
            top1.update(_prec(logits, y, 1), 4)
            top5.update(_prec(logits, y, 5), 4)
        m = meter.read()
        assert m['images_w'] == 8 and m['images_a'] == 4 and m['invalid'] == 0
        assert m['top1'] == top1.avg and m['top5'] == top5.avg and abs(m['objs_w'] - objs_w.avg) <= 1e-12 * objs_w.avg
        assert abs(m['objs_a'] - la.item()) <= 1e-12 * la.item() and abs(m['objs_l'] - ll.item()) <= 1e-12 * ll.item()
        assert 0 <= m['top1_a'] <= m['top5_a'] <= 100
    assert first[0] == first[1]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_buffer(rank):
    return torch.arange(11, dtype=torch.float64) * (rank + 1) + 0.5 * rank


def _worker(rank, world, port, outdir):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tf-nas_amd'))
    import torch.distributed as dist
    from tfnas_amd.tail import SearchMeter
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    meter = SearchMeter('cpu')
    meter.buf.copy_(_rank_buffer(rank))
    meter.reduce_(None)
    torch.save(meter.buf, os.path.join(outdir, 'm%d.pt' % rank))
    dist.destroy_process_group()


def test_reduce_sums_the_buffers_of_two_gloo_ranks(tmp_path):
    from tfnas_amd.tail import SearchMeter
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want = _rank_buffer(0) + _rank_buffer(1)
    for r in range(world):
        assert torch.equal(torch.load(os.path.join(tmp_path, 'm%d.pt' % r)), want)
    meter = SearchMeter('cpu')                    # not distributed: nothing happens
    meter.buf.copy_(_rank_buffer(0))
    meter.reduce_(None)
    assert torch.equal(meter.buf, _rank_buffer(0))


def test_steps_accept_a_meter_argument():
    import inspect
    from tfnas_amd import epoch, search, tail
    for fn in (search.w_step, search.a_step, tail.BiTail.run, tail.frozen_classifier_loss):
        assert inspect.signature(fn).parameters['meter'].default is None, fn
    assert inspect.signature(epoch.search_epoch).parameters['print_freq'].default == 100


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_wgrad_ex_is_declared_exported_and_bound_under_abi_4(lib):
    from tfnas_amd import _lib
    src = open(HEADER).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'^\s*int\s+tfnas_cls_wgrad_ex\s*\(([^;]*)\)\s*;', code, flags=re.M | re.S)
    assert m, 'tfnas_cls_wgrad_ex is not declared in include/tfnas_hip.h'
    assert len([a for a in m.group(1).split(',') if a.strip()]) == 14
    res, args = _lib._PROTOS['tfnas_cls_wgrad_ex']
    assert res is C.c_int and len(args) == 14
    assert [i for i, a in enumerate(args) if a is C.c_float] == [8] and args[:4] == [C.c_int] * 4
    assert hasattr(lib, 'tfnas_cls_wgrad_ex') and 'tfnas_cls_wgrad_ex' in _lib.exported_names()
    assert lib.tfnas_abi_version() == 4 and re.search(r'#define TFNAS_ABI_VERSION 4\b', src)
    doc = src[src.index('tfnas_cls_wgrad_ex ='):src.index('int tfnas_cls_wgrad_ex(')]
    for word in ('bit-identical', 'rank0', 'meter[0]', 'meter[4]', 'NaN', 'TFNAS_ENULL', 'ordered by their stream', 'no atomics'):
        assert word in doc, word


def test_wgrad_ex_argument_checks_answer_before_any_launch(lib):
    """Host pointers are never dereferenced on the device here: every call is refused by the argument checks."""
    one = (C.c_void_p * 2)(1, 1)
    none = (C.c_void_p * 2)(None, None)
    p = C.c_void_p(1)
    f = lib.tfnas_cls_wgrad_ex
    assert f(2, 4, 8, 3, one, one, one, None, 1.0, p, p, p, p, None) == -2          # meter without rank0
    assert f(2, 4, 8, 3, None, one, one, p, 1.0, p, p, p, p, None) == -2
    assert f(2, 4, 8, 3, one, one, one, p, 1.0, None, p, p, p, None) == -2
    assert f(2, 4, 8, 3, one, none, one, p, 1.0, p, p, p, p, None) == -2
    assert f(3, 4, 8, 3, one, one, one, p, 1.0, p, p, p, p, None) == -3
    assert f(1, 0, 8, 3, one, one, one, p, 1.0, p, p, p, p, None) == -3
