"""The helpers of tests/test_gpu_far_offsets.py (tests/far_offsets.py) on the CPU: the periodic selection against brute force at
scaled-down bounds and in closed form at 2^31 and 2^32, the periodic comparison on CPU tensors, and the far signals' extents."""
import numpy as np
import pytest

from tests.far_offsets import B31, B32, TILES, far_packed_signal, far_padded_signal, periodic_mismatch, plan_cycles

COUNT_SETS = [[5, 0, 12, 7, 3, 9], [4, 6, 1, 8], [101, 300, 77, 2, 64], [2, 3], [7, 7, 7, 7]]


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("per", [1, 2, 3, 7, 128])
def test_selection_against_brute_force_at_small_bounds(per, padded):
    bounds = (1 << 15, 1 << 16)
    for counts in COUNT_SETS:
        order = list(range(len(counts)))[::-1]
        p = plan_cycles(counts, per, bounds, padded, order)
        assert p.steps % 2 == 1 and p.steps > 1 and p.period == p.steps * per and (per % 2 == 0 or p.period % 2 == 1)
        assert set(p.cycle) <= set(order) and len(p.cycle) >= len(order) - 1 and [u for u in order if u in p.cycle] == p.cycle
        sel = p.selection()
        assert len(sel) == p.repeats * len(p.cycle) and list(sel[:len(p.cycle)]) == p.cycle and list(sel[-len(p.cycle):]) == p.cycle
        # brute force: the first element of every row of the selection, as the export lays them out
        widths = np.full(len(sel), p.rowStride) if padded else np.asarray(counts)[sel]
        if padded:
            assert p.rowStride >= max(counts[u] for u in p.cycle) and p.rowStride % 2 == 1
        first = np.concatenate([[0], np.cumsum(widths * per)])
        assert first[-1] == p.total
        starts = first[::len(p.cycle)]      # where the cycles begin
        assert np.all(np.diff(starts) == p.period)
        beyond = [k for k in range(p.repeats) if starts[k] > max(bounds)]
        assert beyond == [p.repeats - 1]      # one whole cycle beyond, and no more: R is the smallest
        for b in bounds:
            k = p.straddles[b]
            assert starts[k] <= b < starts[k + 1] and b % p.period != 0
        owner = np.repeat(np.arange(p.repeats), p.period)      # element by element
        for b in bounds:
            assert owner[b] == p.straddles[b]


def test_selection_in_closed_form_at_the_real_bounds():
    counts = [23126, 4001, 17, 30000, 12345, 8192]
    for per in (1, 3, 33, 128):
        for padded in (False, True):
            p = plan_cycles(counts, per, (B31, B32), padded)
            assert (p.repeats - 1) * p.period > B32 >= (p.repeats - 2) * p.period
            assert p.straddles[B31] * p.period <= B31 < (p.straddles[B31] + 1) * p.period
            assert p.straddles[B32] == p.repeats - 2 and p.total == p.repeats * p.period
            assert B31 % p.period and B32 % p.period and p.steps % 2 == 1
    with pytest.raises(ValueError):
        plan_cycles([2, 4, 6], 1, (B31,), False)


def test_periodic_comparison_names_cycle_and_offset():
    import torch
    P, R = 37, 23
    base = torch.arange(P, dtype=torch.int32) * 7 - 50
    for slab in (1, P, 5 * P, 5 * P + 3, 1 << 20):      # one cycle a slab; five (22 later cycles: a partial slab of two at the end); all at once
        flat = base.repeat(R)
        assert periodic_mismatch(flat, P, slab) is None
        m = max(1, slab // P)
        cases = [(R - 1, P - 1), (1, 0), (min(1 + m, R - 1), 0), (min(m, R - 1), P - 1), (R - 2, 5)]      # the last, the first later one, either side of a slab border, the partial slab
        for cycle, off in cases:
            bad = flat.clone()
            bad[cycle * P + off] += 1
            assert periodic_mismatch(bad, P, slab) == (cycle, off), (slab, cycle, off)
        bad = flat.clone()      # in the first cycle: every later cycle differs there, the first of them is named
        bad[11] ^= 1
        assert periodic_mismatch(bad, P, slab) == (1, 11)
        two = flat.clone()      # two differences: the first in memory order
        two[9 * P + 30] += 1; two[9 * P + 4] += 1
        assert periodic_mismatch(two, P, slab) == (9, 4)
    bits = torch.tensor([float("nan"), 1.0, -0.0] * 4).view(torch.int32)      # on bits: a NaN equals itself, -0 is not +0
    assert periodic_mismatch(bits, 3) is None
    bits[5] = 0
    assert periodic_mismatch(bits, 3) == (1, 2)


def edge_groups():
    lens = sorted({1} | {t + d for t in TILES for d in (-1, 0, 1)})
    g31 = [1025] + [L for L in lens if L not in (1025, 1023) and L % 2]
    g32 = [1023] + [L for L in lens if L % 2 == 0] + [2049]
    return lens, g31, g32


def test_far_packed_signal_extents():
    from nvspeechplayer_amd import speechPlayer as sp
    lens, g31, g32 = edge_groups()
    s = far_packed_signal([g31, g32], (B31, B32))
    assert sorted(s.length(r) for r in s.real) == sorted(g31 + g32) and set(lens) <= set(g31 + g32) and len(set(g31 + g32)) == len(g31 + g32)
    assert not set(s.real) & set(s.fillers) and sorted(s.real + s.fillers) == list(range(len(s.extent) - 1))
    assert all(s.start(r) % 2 == 1 for r in s.real)
    for b in (B31, B32):
        r = s.straddlers[b]
        assert r in s.real and s.start(r) < b < s.start(r) + s.length(r) - 1
    assert s.length(s.fillers[0]) > B31 - 2048 and s.start(s.fillers[0]) == 0 and B32 < s.need < B32 + (1 << 16)
    assert all(s.start(r) > B31 - 1024 for r in s.real) and sum(s.start(r) > B32 for r in s.real) >= 3

    import torch
    # the checks read dtype, dim, shape and contiguity alone: a meta tensor has them all and no memory
    meta = torch.empty(s.need, dtype=torch.int16, device="meta")
    tensor, fmt, n, stride, ext, rowlens = sp.check_signal_request((meta, s.extent))
    assert fmt == 0 and n == len(s.extent) - 1 and stride == 0 and list(rowlens[s.real]) == g31 + g32
    with pytest.raises(ValueError):
        sp.check_signal_request((torch.empty(s.need - 1, dtype=torch.int16, device="meta"), s.extent))


def test_far_padded_signal_extents():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    width = (1 << 20) - 1
    g31, g32 = [2305, 1023, 65, 1], [4353, 257, 1, 1025, 64]
    n, lens, real, straddlers = far_padded_signal([g31, g32], (B31, B32), width)
    assert width % 2 == 1 and [int(lens[r]) for r in real] == g31 + g32 and int((lens > 0).sum()) == len(real) == len(set(real))
    for b in (B31, B32):
        r = straddlers[b]
        assert r * width < b < r * width + lens[r] - 1 and r in real
    assert n * width > B32 and n - 1 == max(real) and abs(straddlers[B31] - n // 2) <= 2
    meta = torch.empty((n, width), dtype=torch.float32, device="meta")
    tensor, fmt, rows, stride, ext, rowlens = sp.check_signal_request((meta, lens))
    assert fmt == 1 and rows == n and stride == width and np.array_equal(rowlens, lens)
    n31, lens31, real31, st31 = far_padded_signal([g31], (B31,), width)      # the float32 signal: to just past 2^31 elements
    assert B31 < n31 * width < B31 + 8 * width and st31[B31] == straddlers[B31]
