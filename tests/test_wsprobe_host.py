"""The workspace probe's own parts (tests/_wsprobe.py) on CPU tensors: a probe that cannot see a flipped word proves nothing on
the GPU (tests/test_gpu_ws_independence.py, tests/test_gpu_path_arena_independence.py)."""
import pytest
import torch

import _wsprobe as wp

DTYPES = [torch.float32, torch.float64]


def _flip(t, i, bit=0):
    b = wp.bits(t).view(-1)
    assert b.data_ptr() == t.data_ptr()
    top = 8 * t.element_size() - 1
    b[i] ^= -(1 << top) if bit == top else 1 << bit                            # (the sign bit of a two's-complement word)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_poison_is_finite_in_range_seeded_and_differs_everywhere(dtype):
    n = 100003
    a, b = wp.poison(wp.SEED_A, n, dtype), wp.poison(wp.SEED_B, n, dtype)
    for p in (a, b):
        assert p.dtype == dtype and p.shape == (n,)
        assert bool(torch.isfinite(p).all())
        assert float(p.abs().min()) >= 1.0 and float(p.abs().max()) <= 1000.0
        assert 0.4 < float((p > 0).double().mean()) < 0.6                      # (both signs)
    assert torch.equal(a, wp.poison(wp.SEED_A, n, dtype))                      # (seeded)
    assert wp.differs_everywhere(a, b)
    assert not wp.differs_everywhere(a, a.clone())
    c = a.clone()
    c[1:] = b[1:]
    assert not wp.differs_everywhere(a, c)                                     # (one equal element is enough to say no)


def test_seed_pairs_are_checked():
    wp.check_seed_pair(wp.SEED_A, wp.SEED_B)
    with pytest.raises(AssertionError):
        wp.check_seed_pair(3, 19)                                              # (same tag: equal elements are possible)


def test_reserved_part_words_stay_zero_and_the_rest_is_poisoned():
    piece, slots = 4096, 64
    v = wp.part_fill(torch.empty(3 * piece), wp.SEED_A, piece, slots)
    rows = v.view(3, piece)
    assert wp.part_reserved_zero(v, piece, slots)
    assert not bool(wp.bits(rows[:, piece - slots:]).any())
    assert bool((rows[:, :piece - slots].abs() >= 1.0).all())
    w = wp.part_fill(torch.empty(3 * piece), wp.SEED_B, piece, slots)
    assert wp.differs_everywhere(rows[:, :piece - slots], w.view(3, piece)[:, :piece - slots])
    _flip(v, 2 * piece - 1)                                                    # last reserved word of the middle piece
    assert not wp.part_reserved_zero(v, piece, slots)


def test_the_librarys_part_geometry_is_what_the_probe_fills():
    piece, slots = wp.part_sizes()
    assert 0 < slots < piece
    v = wp.part_fill(torch.empty(2 * piece), wp.SEED_B, piece, slots)
    assert wp.part_reserved_zero(v, piece, slots)
    assert int((v == 0).sum()) == 2 * slots


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('align', [False, True], ids=['plain', 'aligned'])
def test_guard_check_reports_one_flipped_word_in_either_band_at_either_end(dtype, align):
    n = 777
    s = wp.Slab(n, dtype, align=align)
    assert s.view.numel() == n and s.lo >= wp.GUARD and s.raw.numel() - s.lo - n >= wp.GUARD
    if align:
        assert s.view.data_ptr() % 256 == 0
    s.fill(wp.SEED_A)
    assert s.touched() == []
    s.view.neg_()                                                              # (the interior is not guarded)
    assert s.touched() == []
    hi = s.raw.numel() - s.lo - n
    for band, i, at in (('before', 0, 0), ('before', s.lo - 1, s.lo - 1), ('after', 0, s.lo + n), ('after', hi - 1, s.raw.numel() - 1)):
        for bit in (0, 8 * s.raw.element_size() - 1):                          # lowest mantissa bit, sign
            _flip(s.raw, at, bit)
            assert s.touched() == [(band, i)], (band, i, bit)
            _flip(s.raw, at, bit)
            assert s.touched() == []


def test_guard_check_sees_a_word_overwritten_with_an_equal_looking_value():
    s = wp.Slab(16)
    s.raw[3] = float('nan')                                                    # (through floats NaN != NaN either way ...)
    assert s.touched() == [('before', 3)]
    s.raw[3] = wp.SENTINEL
    assert s.touched() == []                                                   # (... and the sentinel itself is the sentinel)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_comparator_reports_a_single_differing_bit(dtype):
    a = wp.poison(wp.SEED_A, 4097, dtype).view(17, 241)
    ra = {'out': a, 'dx': a.t()}                                               # (a non-contiguous result too)
    rb = {'out': a.clone(), 'dx': a.t().clone()}
    assert wp.compare(ra, rb) == {}
    _flip(rb['out'], 4096)
    assert wp.compare(ra, rb) == {'out': 1}
    assert wp.diff_count(ra['out'], rb['out']) == 1
    z = torch.zeros(4, dtype=dtype)
    assert wp.diff_count(z, -z) == 4                                           # -0.0 is not 0.0 here
    nan = torch.full((4,), float('nan'), dtype=dtype)
    assert wp.diff_count(nan, nan.clone()) == 0                                # ... and equal NaNs are equal
    with pytest.raises(AssertionError):
        wp.compare(ra, {'out': a})                                             # (a missing result is not "equal")
