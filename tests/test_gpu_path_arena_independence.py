"""Workspace independence of the path level (tfnas_path_* / tfnas_amd/path.py): a search iteration on an arena that is exactly as
large as planned, guard-banded and poisoned comes out bit-identical to the one on the stock arena (zero-initialised, 2 % + 4 KB
of slack), whatever the poison.

Contract: no entry point reads a workspace buffer it has not written in the same call; nothing past
the reported sizes (TfnasPathWs.total) is touched.  tests/test_gpu_paths.py compares the path level with the per-cell route, to
which a stale read is as invisible as to itself; here PathRunner._grow is replaced (in the test, not in path.py) by one that hands
out a 256-byte aligned view of exactly ``need`` floats inside a guarded slab (tests/_wsprobe.py), every float of it poisoned -- the
`part` pieces at its start included: their reserved words are read by nothing any more (csrc/kernels.h).

The default supernet at 64 x 64, batch 2 (latencies from _kinds.AnyLut: the shipped tables end at 224 x 224); one w_step, one a_step, one more w_step as tests/test_gpu_paths.py::_run, the fused
optimizer steps and the fused classifier tail at their defaults; the same model seed, noise and batches in all three runs.  No
tolerance anywhere: parameters, alpha-gradients and the latency agree in every bit."""
import pytest
import torch

import _wsprobe as wp

pytestmark = pytest.mark.gpu


class ProbeArenas:
    """PathRunner._grow's stand-in for one run, and what it hands out"""

    def __init__(self, seed):
        self.seed, self.made, self.log = seed, [], []

    def grow(self, runner, s, need):
        if s.arena is not None and s.arena.numel() >= need:
            return
        if s.arena is not None:
            torch.cuda.synchronize(runner.device)           # (pending kernels may still use the old arena)
        s.arena = None
        slab = wp.Slab(need, torch.float32, runner.device, align=True)
        slab.fill(self.seed)
        assert slab.view.numel() == need and slab.view.data_ptr() % 256 == 0
        s.arena = slab.view
        self.made.append([s, slab, slab.view.clone()])

    def after_step(self, step):
        """guards of every arena in use, and the floats behind its slot's planned total: (step, arena, touched guard words,
        planned floats, floats behind them, those of them that changed in this step).  A slot is planned again for every step's
        candidates, so a later total may be smaller than an earlier one: the floats between the two were written by the earlier
        step, inside what it had planned.  What every step is held to: nothing behind ITS total changed while it ran (against a
        copy taken after the step before) -- and so every float behind the largest total so far still holds its poison."""
        torch.cuda.synchronize()
        for k, ent in enumerate(self.made):
            s, slab, before = ent
            if s.arena is not slab.view:                    # (replaced by a larger one: no launch uses it any more)
                continue
            total = int(s.ws.total)
            assert total <= slab.n
            self.log.append((step, k, slab.touched(), total, slab.n - total, wp.diff_count(slab.view[total:], before[total:])))
            ent[2] = slab.view.clone()


def _sequence(lut, arenas=None):
    from tfnas_amd import Network, geometry, path, search
    stock = path.PathRunner._grow
    if arenas is not None:
        path.PathRunner._grow = lambda runner, s, need: arenas.grow(runner, s, need)
    try:
        torch.manual_seed(2)
        m = Network(100, geometry.initial_mc_num_dddict(), lut).cuda()
        m.set_temperature(5.0)
        st = search.SearchState(m)
        assert st.runner is not None and search.USE_PATHS and search.FUSED_OPT and search.FUSED_TAIL
        ow, oa = search.make_optimizers(m)
        noise = search.NoiseSource(11)
        gen = torch.Generator(device='cuda').manual_seed(5)

        def batch():
            return (torch.randn(2, 3, 64, 64, device='cuda', generator=gen),
                    torch.randint(0, 100, (2,), device='cuda', generator=gen))

        def done(step):
            if arenas is not None:
                arenas.after_step(step)
        b0, ba, b1 = batch(), batch(), batch()
        search.w_step(st, b0[0], b0[1], ow, 5.0, noise.exp('cuda'), noise.rand_pos())
        done('w1')
        _, _, lat, g = search.a_step(st, ba[0], ba[1], oa, 15.0, 0.1, 5.0, noise.exp('cuda'), return_grads=True)
        res = {'latency': lat.detach().clone().reshape(-1)}
        res.update(('dalpha.%d' % i, t.detach().clone()) for i, t in enumerate(g))
        done('a')
        search.w_step(st, b1[0], b1[1], ow, 5.0, noise.exp('cuda'), noise.rand_pos())
        done('w2')
        torch.cuda.synchronize()
        res.update((k, p.detach().clone()) for k, p in m.named_parameters())
        slots = sorted(k for k, s in st.runner._slots.items() if s.arena is not None and s.arena.numel())
        return res, slots
    finally:
        path.PathRunner._grow = stock


@pytest.fixture(scope='module')
def runs():
    import _kinds
    lut = _kinds.AnyLut()              # (the shipped tables hold the extents of 224 x 224 images only: a latency for every key)
    lut['base'] = 1.5
    wp.check_seed_pair(wp.SEED_A, wp.SEED_B)
    a, b = ProbeArenas(wp.SEED_A), ProbeArenas(wp.SEED_B)
    stock, slots = _sequence(lut)
    ra, slots_a = _sequence(lut, a)
    rb, slots_b = _sequence(lut, b)
    assert slots == slots_a == slots_b and slots                     # the probe arenas were what the steps ran on
    return stock, ra, rb, a, b


def test_iteration_on_a_poisoned_exact_arena_is_bit_identical_to_the_stock_arena(runs):
    stock, ra, rb, _, _ = runs
    assert any(k.startswith('dalpha.') for k in stock) and 'latency' in stock
    assert all(bool(torch.isfinite(v).all()) for v in stock.values())
    assert wp.compare(ra, rb) == {}, 'the iteration depends on what the arena held before'
    assert wp.compare(stock, ra) == {}, 'the iteration depends on the zeros or the slack of the stock arena'


def test_arena_guards_stay_intact_and_nothing_behind_the_planned_total_is_touched(runs):
    for arenas in runs[3:]:
        assert len(arenas.made) >= 3                                 # the soft path and the two bi-sampling paths
        assert {step for step, *_ in arenas.log} == {'w1', 'a', 'w2'}
        assert any(behind > 0 for *_, behind, _ in arenas.log)       # (a sampled path's arena is sized for the widest candidates)
        for step, k, touched, total, behind, lost in arenas.log:
            print('%s arena %d: planned %d floats, %d behind them, %d changed, guards %s' % (step, k, total, behind, lost, touched or 'intact'))
        for step, k, touched, total, behind, lost in arenas.log:
            assert touched == [], (step, k, touched)
            assert lost == 0, (step, k, total, behind, lost)
