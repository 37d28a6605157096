"""What tests/test_gpu_far_offsets.py builds its cases with, held on the CPU by tests/test_far_offsets_host.py: the periodic selection
that carries an export's output past 2^31 and 2^32 elements, the comparison of every later cycle with the first, and the extents of a
signal whose chosen rows lie beyond those elements.  Nothing here needs a GPU; the arithmetic is on counts and extents alone."""
import numpy as np

B31, B32 = 1 << 31, 1 << 32
TILES = (64, 256, 1024)      # the tile sizes of the tile-wise exports (csrc/klatt_tiles.h)


class Cycles(object):
    """cycle: the rows of one cycle (indices into the counts given); rowStride: 0 packed, else every row's steps; steps: the cycle's steps;
    period: its elements (steps * per); repeats: R; total: R * period; straddles: {bound: the cycle that holds element `bound`}."""

    def __init__(self, cycle, rowStride, steps, per, bounds):
        self.cycle, self.rowStride, self.steps, self.per, self.bounds = list(cycle), rowStride, steps, per, tuple(bounds)
        self.period = steps * per
        self.repeats = max(bounds) // self.period + 2
        self.total = self.repeats * self.period
        self.straddles = {b: b // self.period for b in bounds}

    def selection(self):
        return np.tile(np.asarray(self.cycle, np.int64), self.repeats)


def plan_cycles(counts, per, bounds, padded, order=None):
    """The periodic selection: rows `order` (None: all, as they come) of `counts` steps each, `per` elements a step, selected R times so
    that one whole cycle begins beyond the largest of `bounds`.  The cycle's STEPS are made odd and more than one -- packed: the first
    row of an odd count is dropped where the sum is even; padded: a row is dropped where the rows are even in number and the stride is
    the largest count, plus one where that is even.  The period, steps * per, then has an odd factor above one and divides no power of
    two: an element written or read 2^31 or 2^32 elements from its place lands at another offset of its cycle (and where `per` is odd
    the period itself is odd).  ValueError where no such cycle exists."""
    counts = np.asarray(counts, np.int64)
    cycle = list(range(len(counts))) if order is None else [int(u) for u in order]
    if padded:
        if len(cycle) % 2 == 0:
            cycle = cycle[:-1]
        stride = int(counts[cycle].max()) if cycle else 0
        stride += 1 - stride % 2
        steps = len(cycle) * stride
    else:
        stride = 0
        if int(counts[cycle].sum()) % 2 == 0:
            odd = [i for i, u in enumerate(cycle) if counts[u] % 2]
            if not odd:
                raise ValueError("no row of an odd count to drop: the cycle's steps stay even")
            del cycle[odd[0]]
        steps = int(counts[cycle].sum())
    if steps < 3 or steps % 2 == 0:
        raise ValueError("a cycle of %d steps" % steps)
    plan = Cycles(cycle, stride, steps, per, bounds)
    assert all(b % plan.period for b in bounds)
    return plan


def periodic_mismatch(flat, period, slab=1 << 28):
    """Every later cycle of `flat` (one-dimensional, whole cycles of `period` elements, an integer view so that the comparison is on bits)
    against the first, in slabs of whole cycles of about `slab` elements: None, or (cycle, offset) of the first element that differs."""
    assert flat.dim() == 1 and flat.numel() % period == 0 and flat.numel() >= period and not flat.dtype.is_floating_point
    repeats = flat.numel() // period
    first, m = flat[:period], max(1, slab // period)
    for k in range(1, repeats, m):
        mm = min(m, repeats - k)
        differs = flat[k * period:(k + mm) * period].view(mm, period) != first
        if bool(differs.any()):
            at = int(differs.view(-1).byte().argmax())      # (the first of the largest: the first that differs)
            return k + at // period, at % period
    return None


class FarSignal(object):
    """extent: a packed signal's n + 1 offsets; real: its rows that carry a length and are chosen, in the order of the lengths given;
    fillers: the rows between them, never chosen; straddlers: {bound: the real row that holds element `bound`}; need: its elements."""

    def __init__(self, extent, real, fillers, straddlers):
        self.extent, self.real, self.fillers, self.straddlers = np.asarray(extent, np.int64), list(real), list(fillers), dict(straddlers)
        self.need = int(self.extent[-1])

    def start(self, r):
        return int(self.extent[r])

    def length(self, r):
        return int(self.extent[r + 1] - self.extent[r])


def far_packed_signal(groups, bounds):
    """A packed signal: for each of `bounds` (ascending) a filler row up to just below it, then the rows of groups[i] lengths -- the
    first, of two samples or more, straddles the bound --, every real row starting on an odd element: a filler of one sample stands
    between two real rows where the next would start on an even one."""
    extent, real, fillers, straddlers = [0], [], [], {}
    for lens, bound in zip(groups, bounds):
        assert lens[0] >= 2
        start = bound - lens[0] // 2
        start -= 1 - start % 2
        assert extent[-1] < start
        fillers.append(len(extent) - 1)
        extent.append(start)
        for i, L in enumerate(lens):
            if extent[-1] % 2 == 0:
                fillers.append(len(extent) - 1)
                extent.append(extent[-1] + 1)
            if i == 0:
                straddlers[bound] = len(extent) - 1
            real.append(len(extent) - 1)
            extent.append(extent[-1] + L)
    return FarSignal(extent, real, fillers, straddlers)


def far_padded_signal(groups, bounds, width):
    """A padded signal [n, width]: for each bound the row that holds it gets groups[i][0] samples -- enough to reach the bound --, the
    row before it groups[i][1], the rows after it the rest; every other row has length 0.  -> (n, lens [n], real rows in the order of
    the lengths given, {bound: row})."""
    lens, real, straddlers = {}, [], {}
    for g, bound in zip(groups, bounds):
        r = bound // width
        assert r >= 1 and r * width + g[0] > bound and g[0] <= width and max(g) <= width
        rows = [r, r - 1] + [r + 1 + i for i in range(len(g) - 2)]
        for row, L in zip(rows, g):
            assert row not in lens
            lens[row] = L
            real.append(row)
        straddlers[bound] = r
    n = max(lens) + 1
    out = np.zeros(n, np.int64)
    for row, L in lens.items():
        out[row] = L
    return n, out, real, straddlers
