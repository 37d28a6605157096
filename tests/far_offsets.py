"""What tests/test_gpu_far_offsets.py builds its cases with, held on the CPU by tests/test_far_offsets_host.py: the periodic selection
that carries an export's output past 2^31 and 2^32 elements, the comparison of every later cycle with the first, and the extents of a
signal whose chosen rows lie beyond those elements.  Nothing here needs a GPU; the arithmetic is on counts and extents alone.

For tests/test_gpu_stage_far.py, held by tests/test_stage_far_host.py: the plan of a deep stream -- the period P of the input, Q of the
outputs, the chunk c, the pushes needed to pass a bound and the push that holds it (DeepStream) --, the cases (DEEP), their period tables,
their host statements and the steady period W cut from the statement on a short stream (deep_*), and the far pushes' width."""
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


# ---- a deep stream: one periodic chunk pushed again and again (tests/test_gpu_stage_far.py, held by tests/test_stage_far_host.py) ---------
class DeepStream(object):
    """A row fed the same chunk push after push.  P: the input's period in samples; Q: the outputs (samples, or steps) of one period;
    lag: the outputs a fresh row holds back in its first push (the resampler's floor(Z up / down), the spectrogram's frames that reach
    past the chunk, 0 for the convolution); c: the chunk, the largest multiple of P at or below `near`; G: the outputs of a steady
    push, c / P * Q.  Before push k (from 0) the row has consumed k c samples and emitted max(k G - lag, 0) outputs: c is a multiple
    of the operation's own period, so the closed forms' ceilings and floors move by whole numbers from push to push."""

    def __init__(self, P, Q, lag, near=1 << 27):
        assert P >= 1 and Q >= 1 and near >= P
        self.P, self.Q, self.lag = int(P), int(Q), int(lag)
        self.c = near // self.P * self.P
        self.G = self.c // self.P * self.Q
        assert 0 <= self.lag <= self.G

    def consumed(self, k):
        return k * self.c

    def emitted(self, k):
        return max(k * self.G - self.lag, 0)

    def count(self, k, of):
        return self.consumed(k) if of == "N" else self.emitted(k)

    def pushes_to_pass(self, bound, of):
        """The fewest pushes after which the count -- "N" consumed, "M" emitted -- is above `bound`."""
        return bound // self.c + 1 if of == "N" else (bound + self.lag) // self.G + 1

    def crossing(self, bound, of):
        """The push k that holds index `bound`: count(k) <= bound < count(k + 1)."""
        return self.pushes_to_pass(bound, of) - 1

    def rotation(self, k):
        """The first output of push k, modulo the outputs' period: the same for every steady push, G being a multiple of Q."""
        return self.emitted(k) % self.Q


def rotated(W, first, count=None):
    """The period W (its first axis) tiled from output `first` on: element i is W[(first + i) mod len(W)]; `count` of them (None: one period)."""
    W = np.asarray(W)
    count = len(W) if count is None else count
    return W[(first + np.arange(count, dtype=np.int64)) % len(W)]


# A padded signal's width for the far pushes: odd; 2^31 = 21846 * FAR_WIDTH + 2 and 2^32 = 43692 * FAR_WIDTH + 4, so a row begins two or four
# elements below a bound and the shortest chunk still straddles it; narrow, so that the 2^32 elements are many rows (the filter and ADPCM
# stages take a lane per row and walk a padded row's stride serially)
FAR_WIDTH = 98301

# The deep cases: the kind, what makes the stage, the rows, the chunk's type, the period's odd factor and the depth N must pass
DEEP = {
    "resample 22050 -> 48000": dict(kind="resample", rates=(22050, 48000), rows=2, npt=np.int16, k=7, bound=B31),
    "resample 48000 -> 4000": dict(kind="resample", rates=(48000, 4000), rows=2, npt=np.int16, k=85, bound=B32),
    "convolution": dict(kind="convolution", taps=(5, 1025), rows=2, npt=np.float32, P=999, bound=B32, both=True),      # both: row 1 as well, behind its reset
    "spectrogram 1024 / 8192 + 3": dict(kind="spectrogram", geometry=(1024, 8192, 3), mel=False, rows=1, npt=np.float32, q=3, bound=B32),
    "spectrogram 512 / 160 bins": dict(kind="spectrogram", geometry=(512, 160, 0), mel=False, rows=1, npt=np.int16, q=7, bound=B32),
    "spectrogram 512 / 160 mel": dict(kind="spectrogram", geometry=(512, 160, 0), mel=True, rows=1, npt=np.int16, q=7, bound=B32),
}
SHORT = 4      # periods of the short stream the steady period is cut from: its third


def deep_ratio(case):
    from math import gcd
    src, dst = case["rates"]
    g = gcd(src, dst)
    return dst // g, src // g      # up, down


def deep_period(case):
    """-> (P samples, Q outputs of a period, multiplier: what an output's index is multiplied by in the kernel -- down, 1, hop)."""
    if case["kind"] == "resample":
        up, down = deep_ratio(case)
        return down * case["k"], up * case["k"], down
    if case["kind"] == "convolution":
        return case["P"], case["P"], 1
    hop = case["geometry"][1]
    return case["q"] * hop, case["q"], hop


def deep_response(K):
    """A decaying response of K taps, zero taps among them, small enough that the int16 outputs do not clip."""
    rng = np.random.default_rng(900 + K)
    h = (rng.normal(0.0, 1.0, K) * np.exp(-np.arange(K) / (0.3 * K + 1.0)) * 0.5 / np.sqrt(K)).astype(np.float32)
    h[2::7] = 0.0
    return h


def deep_bank(case):
    import nvspeechplayer_amd as eng
    return eng.melFilterbank(16000, case["geometry"][0], 20) if case["mel"] else None


def deep_bands(case):
    return 1 if case["kind"] != "spectrogram" else 20 if case["mel"] else case["geometry"][0] // 2 + 1


def deep_table(name, row, rotate=0, length=None, seed=0):
    """Row `row`'s period table of the case -- random, so that two offsets of a period hold different samples --, rotated: element n is
    element (n + rotate) mod P of the unrotated one.  length, seed: a chunk of another length instead (a stream's last)."""
    case = DEEP[name]
    P = deep_period(case)[0] if length is None else length
    rng = np.random.default_rng([sorted(DEEP).index(name), row, seed])
    x = rng.integers(-32768, 32768, P).astype(np.int16) if case["npt"] == np.int16 else rng.uniform(-1.0, 1.0, P).astype(np.float32)
    return np.roll(x, -rotate)


def deep_statement(name, row, x, fmt, ended=True):
    """The host statement of the case's operation on the whole signal x, in the push's format `fmt` (1 float32; 0 int16, the spectrogram's
    float64): [outputs] or [steps, bands].  ended False: the convolution without its tail."""
    import nvspeechplayer_amd as eng
    case = DEEP[name]
    x = x.astype(np.float32) / np.float32(32767.0) if x.dtype == np.int16 else x      # the reader's conversion
    if case["kind"] == "resample":
        return eng.signalResample(x, *case["rates"], dtype=np.float32 if fmt else np.int16)
    if case["kind"] == "convolution":
        return eng.signalConvolve(x, deep_response(case["taps"][row % len(case["taps"])]), tail=bool(ended), dtype=np.float32 if fmt else np.int16)
    y = eng.signalSpectrogram(x, *case["geometry"], bank=deep_bank(case), power=2)
    return y.astype(np.float32) if fmt else y


def deep_emitted(name, row, N, ended=False):
    """The outputs a row of the case has emitted after N samples, from the host's closed forms."""
    import nvspeechplayer_amd as eng
    case = DEEP[name]
    if case["kind"] == "resample":
        return eng.resampleEmitted(N, *case["rates"], ended=ended)
    if case["kind"] == "convolution":
        return N + (case["taps"][row % len(case["taps"])] - 1 if ended else 0)
    return eng.spectrogramEmitted(N, *case["geometry"], ended=ended)


def deep_plan(name, near=1 << 27):
    """The case's DeepStream: the lag from the closed form of the first push, the same for every row."""
    case = DEEP[name]
    P, Q, _ = deep_period(case)
    c = near // P * P
    lags = {c // P * Q - deep_emitted(name, i, c) for i in range(case["rows"])}
    assert len(lags) == 1
    return DeepStream(P, Q, lags.pop(), near)


def deep_short(name, row, fmt, rotate=0, last=None):
    """The statement on the short stream: SHORT periods of the row's table, then `last` (a chunk, or None), ended."""
    x = np.tile(deep_table(name, row, rotate), SHORT)
    return deep_statement(name, row, x if last is None else np.concatenate([x, last]), fmt)


def deep_W(name, row, fmt, rotate=0):
    """The steady period W, [Q] or [Q, bands]: outputs 2 Q .. 3 Q - 1 of the statement on SHORT periods -- no tap or frame of theirs reaches
    before sample 0 or past the end (asserted by the host test against a longer stream)."""
    Q = deep_period(DEEP[name])[1]
    y = deep_short(name, row, fmt, rotate)
    assert len(y) >= 3 * Q
    return y[2 * Q:3 * Q]
