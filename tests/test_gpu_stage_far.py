"""The signal stages' 64-bit bookkeeping run where it matters (include/speechPlayer_batch.h, "Signal stages" and "Signal stages that keep a
window"; csrc/klatt_stage.h, klatt_stage_window.h, klatt_resample.h: resample_rows<KEPT>, klatt_convolve.h: conv_rows<KEPT>, klatt_engine.hip:
Stage::N, Stage::M): what tests/test_gpu_stage.py and test_gpu_stage_window.py hold on short streams, held on long ones.

  0. The resampler's products m * down past 2^31 and 2^32 inside a push, directly against signalResample on 12 to 16 million samples a row.
  1. Deep streams: a row's N, M, M * down and (M + j) * hop past 2^31 and 2^32.  One device chunk of whole periods is pushed again and again;
     every steady push must be periodic, equal the first steady push of its format, and hold the steady period W of the host statement on a
     short stream, rotated by the push's first output index (tests/test_stage_far_host.py holds, on the CPU, that this is the statement's
     value and that an index short of 2^31 or 2^32 changes it).  The stream's end, a row reset midway and a new stream on the same stage
     are held too.  The filter and ADPCM stages are not part of this section: their kernels never see N or M -- StageLaneRow carries
     neither --, and a lane per row being sequential, 2^31 steps of one row would take minutes.
  2. Far addresses inside one push, all five kinds: a padded chunk whose fed rows straddle, precede and follow elements 2^31 and 2^32 of the
     signal (int16; a float32 chunk goes past element 2^31, byte 2^33), every other row of length 0, and a padded output of n * rowStride
     past 2^32 elements: the fed rows against the host statements, everything else +0, and the rows that were not fed untouched.

A truncated index lands inside the test's own buffers or reads poison: it shows as a wrong value, bit for bit.  The helpers are
tests/far_offsets.py.  Needs a GPU with some 30 GB free; a case that finds less skips and says so (none does on an MI355X)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.far_offsets import (B31, B32, DEEP, FAR_WIDTH, SHORT, deep_bands, deep_bank, deep_emitted, deep_period, deep_plan, deep_ratio, deep_response,
                               deep_short, deep_table, deep_W, far_padded_signal, periodic_mismatch, rotated)
from tests.test_filter_host import seven
from tests.test_gpu_far_offsets import GUARD, give_back, guarded, guards_intact, int_view, peak, room  # noqa: F401  (give_back and peak are fixtures)
from tests.test_gpu_signal import edge_rows, poison, record
from tests.test_gpu_stage import F32, FORMS, Raw, bare, check_segments, same, x_of  # noqa: F401  (bare is a fixture)

pytestmark = pytest.mark.gpu


def p(a):
    return None if a is None else a.ctypes.data


def torch_type(fmt, spec=False, codes=False):
    import torch
    return torch.uint8 if codes else torch.float32 if fmt else torch.float64 if spec else torch.int16


class Window(object):
    """One allocation between guards (`guarded`), handed out again and again as a poisoned buffer of another type and size."""

    def __init__(self, dev, elements, dtype):
        self.whole, _ = guarded(dev, elements, dtype)
        self.poisoned = (elements, dtype)      # what `guarded` left: a first take of the same needs no second fill

    def take(self, elements, dtype):
        import torch
        raw = self.whole.view(torch.uint8)
        size = torch.empty(0, dtype=dtype).element_size()
        assert (elements + 2 * GUARD) * size <= raw.numel()
        buf = raw[:(elements + 2 * GUARD) * size].view(dtype)
        if self.poisoned != (elements, dtype) or size == 1:
            buf.fill_(float("nan") if dtype.is_floating_point else 0x55 if size == 1 else -7)
        self.poisoned = None
        return buf, buf[GUARD:GUARD + elements]


def intact(buf):
    import torch
    if buf.dtype == torch.uint8:
        return bool((buf[:GUARD] == 0x55).all()) and bool((buf[-GUARD:] == 0x55).all())
    return guards_intact(buf)


def nonzero_words(flat, slab=1 << 28):
    """The elements of a one-dimensional integer view that are not +0, counted on the device in slabs."""
    return sum(int((flat[a:a + slab] != 0).sum()) for a in range(0, flat.numel(), slab))


# ---- 0. the 32-bit products, directly against the statement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates, n, samples", [((22050, 16000), 3, 16_000_000), ((48000, 4000), 1, 12_000_000)], ids=["22050-16000", "48000-4000"])
def test_resampler_products_past_2_31_and_2_32_against_the_statement(bare, rates, n, samples):
    """22050 -> 16000 (up 320, down 441) on 3 rows of 16 million int16 samples, 48000 -> 4000 (down / up = 12, spans split) on one of 12
    million: nine pushes a row, their lengths drawn per row and unsorted, one of 0 and one of 1 among them, the last ending every row.  At
    down 441 the product m * down passes 2^31 at output 4.87 million and 2^32 at 9.74 million, inside a push (asserted from the counts).
    Per row the outputs concatenate to signalResample of the concatenated chunks, float32 and int16 pushes alternating, bit for bit; every
    push's counts are speechPlayer_stage_plan's (Raw.push) and the differences of resampleEmitted."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    src, dst = rates
    up, down = deep_ratio(dict(rates=rates))
    raw = Raw(bare, L.speechPlayer_batch_stageResample(bare._h, n, src, dst, 6, 0.99, 0, 0.0), n)
    rng = np.random.default_rng(src % 97 + n)
    pushes, lens = 9, []
    for i in range(n):      # per row: seven unequal parts of samples - 1, a 0 and a 1, in an order of the row's own
        cuts = np.sort(rng.choice(np.arange(1, samples - 1), 6, replace=False))
        parts = list(np.diff(np.concatenate([[0], cuts, [samples - 1]]))) + [0, 1]
        lens.append([int(parts[j]) for j in rng.permutation(pushes)])
        assert sum(lens[-1]) == samples and sorted(lens[-1]) != lens[-1] and len(set(lens[-1])) == pushes
    segments = [[dict(x=[], out=[])] for _ in range(n)]
    N, M = np.zeros(n, np.int64), np.zeros((pushes + 1, n), np.int64)
    for k in range(pushes):
        ls = [lens[i][k] for i in range(n)]
        end = np.full(n, k == pushes - 1, np.uint8)
        rows = edge_rows(ls, np.int16, 7000 + 10 * k + n)
        form = dict(FORMS[k % len(FORMS)])
        if form["in_stride"] < 0:
            form["in_stride"] = max(ls) + 5
        got = raw.push(rows, end, **form)()
        for i in range(n):
            want = eng.resampleEmitted(int(N[i]) + ls[i], src, dst, ended=bool(end[i])) - eng.resampleEmitted(int(N[i]), src, dst)
            assert len(got[i][0]) == want, (rates, k, i)
            segments[i][0]["x"].append(x_of(rows[i]))
            segments[i][0]["out"].append((form["fmt"], got[i]))
        N += np.array(ls)
        M[k + 1] = M[k] + [len(g[0]) for g in got]
    for i in range(n):
        assert M[-1, i] == -(-samples * up // down)
        for bound in (B31, B32):
            m = -(-bound // down)      # the first output whose product is at or past the bound
            if m < M[-1, i] - 1:
                k = int(np.searchsorted(M[:, i], m, side="right")) - 1
                assert M[k, i] < m < M[k + 1, i] - 1, (rates, i, bound)      # inside push k, outputs on both sides of it
                print("products %s row %d: m * down passes 2^%d at output %d, in push %d (outputs %d .. %d)" % (rates, i, bound.bit_length() - 1, m, k, M[k, i], M[k + 1, i] - 1))
            else:
                assert down == 12      # one twelfth: a million outputs, no product past 2^31 -- the spans' case
    if down == 441:
        assert all((M[-1, i] - 1) * down > B32 for i in range(n))
    consumed, emitted = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    assert L.speechPlayer_stage_counts(raw.h, p(consumed), p(emitted)) == 0 and not consumed.any() and not emitted.any()
    # the statement: a plain loop over the row's outputs, once per row and format, the rows side by side (the library call holds no lock)
    whole = [np.concatenate(segments[i][0]["x"]) for i in range(n)]
    with ThreadPoolExecutor(2 * n) as pool:
        want = {(i, fmt): pool.submit(eng.signalResample, whole[i], src, dst, dtype=F32 if fmt else np.int16) for i in range(n) for fmt in (0, 1)}
    check_segments(segments, lambda i, x, fmt: (want[i, fmt].result(),), (rates, n))
    raw.free()


# ---- 1. deep into a stream -------------------------------------------------------------------------------------------------------------------
def make_deep_stage(bare, name):
    from nvspeechplayer_amd import _native
    L = _native.load()
    case = DEEP[name]
    n = case["rows"]
    if case["kind"] == "resample":
        h = L.speechPlayer_batch_stageResample(bare._h, n, case["rates"][0], case["rates"][1], 6, 0.99, 0, 0.0)
    elif case["kind"] == "convolution":
        irs = [deep_response(K) for K in case["taps"]]
        flat, start = np.concatenate(irs), np.concatenate([[0], np.cumsum(case["taps"])]).astype(np.int64)
        of = (np.arange(n) % len(irs)).astype(np.int64)
        h = L.speechPlayer_batch_stageConvolve(bare._h, n, p(flat), p(start), len(irs), p(of), 1)
    else:
        nFft, hop, phase = case["geometry"]
        bank = deep_bank(case)
        h = L.speechPlayer_batch_stageSpectrogram(bare._h, n, nFft, hop, phase, None, p(bank), 0 if bank is None else len(bank), 2, 0.0, 0.0)
    assert h, _native.last_error()
    return L, h


@pytest.mark.parametrize("name", list(DEEP))
def test_deep_streams_hold_the_statements_period(bare, name):
    """See the module's docstring, section 1, and DEEP of tests/far_offsets.py for the cases.  In a two-row case row 1 is reset after the
    push that takes N past 2^30: from then on the two rows of every launch are at different depths, row 1's next push is its very first
    push again, and row 0 is undisturbed."""
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    case = DEEP[name]
    n, per, spec = case["rows"], deep_bands(case), case["kind"] == "spectrogram"
    P, Q, mult = deep_period(case)
    plan = deep_plan(name)
    c, G, period = plan.c, plan.G, Q * per
    assert B31 % P and B32 % P and B31 % Q and B32 % Q and c % P == 0 and G % Q == 0
    deepest = plan.pushes_to_pass(case["bound"], "N")      # pushes that take a row past the case's bound
    reset_after = plan.pushes_to_pass(1 << 30, "N") - 1 if n == 2 else -1      # the push that takes N past 2^30
    pushes = deepest + (reset_after + 1 if case.get("both") else 0)      # both rows that deep: row 1 starts again behind its reset
    L, h = make_deep_stage(bare, name)
    dev = "cuda:%d" % bare.device
    stride = G + 3
    elements = n * stride * per
    big = Window(bare.device, elements, torch_type(1 if not spec else 0, spec))
    room(bare.device, 4 * elements * (8 if spec else 4) + n * c * 4)      # the first push and the steady push of each format are kept
    tables = [deep_table(name, i) for i in range(n)]
    chunk = torch.stack([torch.from_numpy(t).to(dev).repeat(c // P) for t in tables])
    assert chunk.shape == (n, c) and chunk.is_contiguous()
    extent = np.full(n, c, np.int64)      # (the record holds its address)
    rec = record(sp, chunk.data_ptr(), 1 if case["npt"] == np.float32 else 0, n, c, extent)
    W = {(i, fmt): np.ascontiguousarray(deep_W(name, i, fmt)).reshape(-1) for i in range(n) for fmt in (0, 1)}
    head = {(i, fmt): np.ascontiguousarray(deep_short(name, i, fmt)[:3 * Q]).reshape(-1) for i in range(n) for fmt in (0, 1)}

    # the pushes of a row that hold a crossing, by the row's depth: of N, of M, and of the kernel's product M * mult (m * down, (M + j) * hop)
    crossings = {}
    for bound in (B31, B32):
        for what, of, b in (("N", "N", bound), ("M", "M", bound), ("M * %d" % mult, "M", -(-bound // mult))):
            k = plan.crossing(b, of)
            if k < deepest and not (what[0] == "M" and mult == 1 and what != "M"):
                crossings.setdefault(k, []).append("%s passes 2^%d (%s %d .. %d)" % (what, bound.bit_length() - 1, of, plan.count(k, of), plan.count(k + 1, of)))
    assert plan.crossing(case["bound"], "N") == deepest - 1

    depth = [0] * n              # pushes a row has taken since it was fresh
    lengths, consumed, emitted = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    first, steady, seen_steady = None, {}, set()

    def push(fmt, signal, end, row_stride):
        buf, body = big.take(n * row_stride * per, torch_type(fmt, spec))
        got = L.speechPlayer_stage_push(h, p(signal), p(end), body.data_ptr(), fmt, None, row_stride, p(lengths), None)
        assert got == n * row_stride * per, (name, got, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert guards_intact(buf), (name, "guards")
        return int_view(body).view(n, row_stride * per), body

    def check_fresh(i, row, fmt, tag):
        """A fresh row's push: the statement's first outputs, then its period to the end."""
        cnt = int(lengths[i]) * per
        assert int(lengths[i]) == G - plan.lag and cnt >= 3 * period
        assert same(row[:3 * period].cpu().numpy().view(head[i, fmt].dtype), head[i, fmt]), tag + ("the first outputs",)
        whole = (cnt - 2 * period) // period * period
        bad = periodic_mismatch(row[2 * period:2 * period + whole], period)
        assert bad is None, tag + ("cycle %d differs at offset %d" % bad if bad else "",)
        rest = cnt - 2 * period - whole
        assert torch.equal(row[2 * period + whole:cnt], row[2 * period:2 * period + rest]), tag + ("the last partial period",)
        assert not bool(row[cnt:].any()), tag + ("padding",)

    def check_steady(i, row, fmt, host, tag):
        cnt = int(lengths[i]) * per
        assert int(lengths[i]) == G, tag
        bad = periodic_mismatch(row[:cnt], period)
        assert bad is None, tag + ("cycle %d differs from the first at offset %d" % bad if bad else "",)
        assert not bool(row[cnt:].any()), tag + ("padding",)
        if host:      # the period itself, on the host: W from the push's first output on
            m0 = plan.emitted(depth[i])
            want = np.ascontiguousarray(rotated(W[i, fmt].reshape(Q, per), m0)).reshape(-1)
            assert same(row[:period].cpu().numpy().view(want.dtype), want), tag + ("W rotated by", m0 % Q)

    for k in range(pushes):
        fmt = 0 if k == reset_after + 1 and n == 2 else k % 2      # (row 1's push after its reset is in the first push's format)
        rows, body = push(fmt, rec, None, stride)
        tag = (name, "push", k, "format", fmt)
        is_steady = all(d >= 1 for d in depth)
        for i in range(n):
            if depth[i] in crossings:
                print("deep %s: push %d of %d samples a row, row %d in its push %d: %s" % (name, k, c, i, depth[i], "; ".join(crossings[depth[i]])))
            if depth[i] == 0:
                check_fresh(i, rows[i], fmt, tag + ("row", i))
            else:
                check_steady(i, rows[i], fmt, depth[i] in crossings or (is_steady and fmt not in seen_steady), tag + ("row", i))
        if k == 0:
            first = rows.clone()
        elif depth[-1] == 0:      # row 1 behind its reset: its very first push again, bit for bit, beside row 0 deep in its stream
            assert torch.equal(rows[1], first[1]), tag + ("row 1 after its reset",)
            assert fmt in steady and torch.equal(rows[0], steady[fmt][0]), tag + ("row 0 beside the reset row",)
        elif fmt not in steady:
            steady[fmt] = rows.clone()
            seen_steady.add(fmt)
        else:
            assert torch.equal(rows, steady[fmt]), tag + ("the first steady push of the format",)
        for i in range(n):
            depth[i] += 1
        assert L.speechPlayer_stage_counts(h, p(consumed), p(emitted)) == 0
        assert list(consumed) == [plan.consumed(d) for d in depth] and list(emitted) == [plan.emitted(d) for d in depth], tag
        assert list(emitted) == [deep_emitted(name, i, plan.consumed(depth[i])) for i in range(n)], tag
        if k == reset_after:
            assert consumed[1] > 1 << 30 >= consumed[1] - c
            assert L.speechPlayer_stage_reset(h, p(np.array([0, 1], np.uint8)), None) == 0
            depth[1] = 0
            assert L.speechPlayer_stage_counts(h, p(consumed), p(emitted)) == 0 and list(consumed) == [plan.consumed(depth[0]), 0] and emitted[1] == 0
    assert consumed[0] > case["bound"] and set(steady) == {0, 1} and (n == 1 or depth[1] < depth[0])
    assert not case.get("both") or consumed[1] > case["bound"]
    for i in range(n):
        print("deep %s: %d pushes, row %d at N = %d, M = %d, M * %d = %d; %d outputs a push" % (name, pushes, i, consumed[i], emitted[i], mult, emitted[i] * mult, G))

    # the end: a short chunk and the end flag; the last outputs of the statement on four periods and that chunk
    short = 37 if case["kind"] == "convolution" else P + 37
    last = [deep_table(name, i, length=short, seed=1) for i in range(n)]
    tail = torch.stack([torch.from_numpy(x).to(dev) for x in last])
    tail_extent = np.full(n, short, np.int64)
    tail_rec = record(sp, tail.data_ptr(), 1 if case["npt"] == np.float32 else 0, n, short, tail_extent)
    counts = [deep_emitted(name, i, SHORT * P + short, ended=True) - deep_emitted(name, i, SHORT * P) for i in range(n)]
    fmt = pushes % 2
    rows, body = push(fmt, tail_rec, np.ones(n, np.uint8), max(counts) + 3)
    assert list(lengths) == counts, (name, "the end", list(lengths), counts)
    for i in range(n):
        want = np.ascontiguousarray(deep_short(name, i, fmt, last=last[i])).reshape(-1)
        cnt = counts[i] * per
        assert same(rows[i, :cnt].cpu().numpy().view(want.dtype), want[len(want) - cnt:]), (name, "the end", i)
        assert not bool(rows[i, cnt:].any())
    assert L.speechPlayer_stage_counts(h, p(consumed), p(emitted)) == 0 and not consumed.any() and not emitted.any()
    # a new stream on the same stage: the very first push of the case
    rows, body = push(0, rec, None, stride)
    assert torch.equal(rows, first), (name, "a new stream")
    L.speechPlayer_stage_free(h)


# ---- 2. far addresses inside one push ----------------------------------------------------------------------------------------------------------
def far_kinds():
    """{kind: (chunk type, make(L, batch, n) -> handle, per-row pool of chunk lengths (row -> [the straddler's, three more]), statement(row, x,
    fmt) -> the parts check_segments compares, output format, bands, codes as well)}"""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer as sp
    T = sp.FILTER_TILE
    Z = eng.resampleKernel(22050, 16000)[0].shape[1] // 2
    filters = seven()
    flat, start = np.concatenate(filters), np.concatenate([[0], np.cumsum([len(f) for f in filters])]).astype(np.int64)
    irs = [deep_response(5), deep_response(1025)]
    taps, tstart = np.concatenate(irs), np.array([0, 5, 1030], np.int64)
    held = {}

    def filter_stage(L, b, n):
        held["of"] = ((np.arange(n) * 3) % 7).astype(np.int64)
        return L.speechPlayer_batch_stageFilter(b, n, p(flat), p(start), 7, p(held["of"]), T + 3)

    def conv_stage(L, b, n):
        held["irOf"] = (np.arange(n) % 2).astype(np.int64)
        return L.speechPlayer_batch_stageConvolve(b, n, p(taps), p(tstart), 2, p(held["irOf"]), 1)

    def code(codec):
        return (np.int16, lambda L, b, n: L.speechPlayer_batch_stageCode(b, n, sp.CODECS.index(codec)), lambda r: [2 * T + 3, T - 1, T + 1, 2 * T + 3],
                lambda r, x, fmt: eng.signalCode(x, codec, codes=True, decoded=True, dtype=F32 if fmt else np.int16), 0, 1, True)

    return {
        "resample": (np.int16, lambda L, b, n: L.speechPlayer_batch_stageResample(b, n, 22050, 16000, 6, 0.99, 0, 0.0), lambda r: [137, Z, 2 * Z, 137],
                     lambda r, x, fmt: (eng.signalResample(x, 22050, 16000, dtype=F32 if fmt else np.int16),), 0, 1, False),
        "filter": (np.int16, filter_stage, lambda r: [2 * T + 3, T - 1, T + 1, 2 * T + 3],
                   lambda r, x, fmt: (eng.signalFilter(x, filters[held["of"][r]], tail=T + 3, dtype=F32 if fmt else np.int16),), 0, 1, False),
        "adpcm": code("adpcm"),
        "alaw": code("alaw"),
        "convolution": (np.float32, conv_stage, lambda r: [1025, (5, 1025)[r % 2] - 1, (5, 1025)[r % 2], 1025],
                        lambda r, x, fmt: (eng.signalConvolve(x, irs[r % 2], tail=True, dtype=F32 if fmt else np.int16),), 0, 1, False),
        "spectrogram": (np.float32, lambda L, b, n: L.speechPlayer_batch_stageSpectrogram(b, n, 64, 16, 0, None, None, 0, 2, 0.0, 0.0), lambda r: [1000, 15, 64, 1000],
                        lambda r, x, fmt: (eng.signalSpectrogram(x, 64, 16, 0, power=2).astype(F32 if fmt else np.float64),), 1, 33, False),
    }


@pytest.mark.parametrize("kind", ["resample", "filter", "adpcm", "alaw", "convolution", "spectrogram"])
def test_far_addresses_inside_one_push(bare, kind):
    """See the module's docstring, section 2.  A chunk [n, FAR_WIDTH]: 2^31 and 2^32 lie two and four elements inside rows 21846 and 43692;
    those rows, the row before each and the two after each are fed -- the kind's own edge lengths (filter and codecs T - 1, T + 1, 2 T + 3;
    convolution K - 1, K, 1025; resampler Z, 2 Z, 137; spectrogram hop - 1, nFft, 1000), in another order in the second push, the straddling
    row the longest both times --, every other row has length 0 and its end flag clear.  The second push ends the fed rows.  A third
    feeds and ends three rows that were never fed: what a fresh stage gives."""
    import torch
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    npt, make, pool, statement, fmt, per, codes = far_kinds()[kind]
    spec = kind == "spectrogram"
    bounds = (B31, B32) if npt == np.int16 else (B31,)      # (a float32 chunk past element 2^32 and its output would not fit in 30 GB together)
    rows_of = {b: [b // FAR_WIDTH, b // FAR_WIDTH - 1, b // FAR_WIDTH + 1, b // FAR_WIDTH + 2] for b in bounds}
    groups = [[pool(r)[j] for j, r in enumerate(rows_of[b])] for b in bounds]
    n, lens1, real, straddlers = far_padded_signal(groups, bounds, FAR_WIDTH)
    assert real == [r for b in bounds for r in rows_of[b]]
    order2 = [0, 2, 3, 1]      # the second push: the straddler's length again, the others' in another order
    lens2 = np.zeros(n, np.int64)
    for b in bounds:
        for j, r in enumerate(rows_of[b]):
            lens2[r] = pool(r)[order2[j]]
    for b in bounds:
        r = straddlers[b]
        assert all(r * FAR_WIDTH < b < r * FAR_WIDTH + ls[r] - 1 for ls in (lens1, lens2))      # the bound inside the row's chunk, both pushes
    assert n * FAR_WIDTH > max(bounds) and FAR_WIDTH % 2 == 1
    h = make(L, bare._h, n)
    assert h, _native.last_error()
    dev = "cuda:%d" % bare.device
    td = torch.int16 if npt == np.int16 else torch.float32
    el_out = torch.empty(0, dtype=torch_type(fmt, spec)).element_size()
    # the output: padded, n * rowStride * per past 2^32 elements, rowStride odd
    counts = np.zeros(n, np.int64)
    most = 0
    for ls, end in ((lens1, None), (lens2, (lens2 > 0).astype(np.uint8))):      # (planned on a scratch walk: a plan moves no state)
        assert L.speechPlayer_stage_plan(h, p(ls), p(end), p(counts)) >= 0
        most = max(most, int(counts.max()))
    far_rows = rows_of[bounds[-1]]      # the rows around the signal's last bound: their outputs begin past element 2^32 of the output
    stride = max(B32 // (min(far_rows) * per) + 1, most + 1) | 1
    elements = n * stride * per
    assert min(far_rows) * stride * per > B32 and stride > most and elements * el_out < 18e9
    assert all(max(rows_of[b]) * stride * per > b for b in bounds)
    room(bare.device, n * FAR_WIDTH * np.dtype(npt).itemsize + elements * (el_out + (1 if codes else 0)) + (1 << 30))
    seed = torch.from_numpy(poison(1 << 20, npt).view(np.int16 if npt == np.int16 else np.int32)).to(dev)
    numel = n * FAR_WIDTH
    signal = torch.empty(numel, dtype=seed.dtype, device=dev)
    whole = numel - numel % len(seed)
    signal[:whole].view(-1, len(seed))[:] = seed
    signal[whole:] = seed[:numel - whole]
    signal = signal.view(td).view(n, FAR_WIDTH)
    out = Window(bare.device, elements, torch_type(fmt, spec))
    cod = Window(bare.device, elements, torch.uint8) if codes else None
    lengths = np.zeros(n, np.int64)
    segments = [[dict(x=[], out=[])] for _ in real]

    def feed(ls, rows, seed_):
        chunks = edge_rows([int(ls[r]) for r in rows], npt, seed_)
        for r, x in zip(rows, chunks):
            signal[r, :len(x)] = torch.from_numpy(x).to(dev)
        extent = np.array(ls, np.int64)
        return chunks, (record(sp, signal.data_ptr(), 1 if npt == np.float32 else 0, n, FAR_WIDTH, extent), extent)      # (the record holds the extent's address)

    for k, ls in enumerate((lens1, lens2)):
        chunks, (rec, _extent) = feed(ls, real, 300 + k)
        end = None if k == 0 else (ls > 0).astype(np.uint8)
        (buf, body), (cbuf, cbody) = out.take(elements, torch_type(fmt, spec)), cod.take(elements, torch.uint8) if codes else (None, None)
        got = L.speechPlayer_stage_push(h, p(rec), p(end), body.data_ptr(), fmt, None if cbody is None else cbody.data_ptr(), stride, p(lengths), None)
        assert got == elements, (kind, k, got, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert intact(buf) and (cbuf is None or intact(cbuf)), (kind, k, "guards")
        assert lengths.sum() == lengths[real].sum() > 0      # (a fed row may still emit nothing: Z samples of an open resampler row, less than a frame)
        views = [int_view(body).view(n, stride * per)] + ([cbody.view(n, stride)] if codes else [])
        for v in views:      # everything outside the fed rows' spans is +0
            inside = sum(int((v[r, :int(lengths[r]) * (per if v is views[0] else 1)] != 0).sum()) for r in real)
            assert nonzero_words(v.view(-1)) == inside > 0, (kind, k, "something outside the fed rows' outputs is not +0")
        for j, r in enumerate(real):
            parts = [body.view(n, stride * per)[r, :int(lengths[r]) * per].cpu().numpy().reshape((-1, per) if spec else (-1,))]
            if codes:
                parts.append(cbody.view(n, stride)[r, :int(lengths[r])].cpu().numpy())
            segments[j][0]["x"].append(x_of(chunks[j]))
            segments[j][0]["out"].append((fmt, tuple(parts)))
    check_segments(segments, lambda j, x, f: statement(real[j], x, f), (kind,))
    first_out = min(real) * stride * per
    print("far push %s: %d rows of %d, fed rows %s; output stride %d, %d elements, the fed rows' outputs from element %d on" % (kind, n, FAR_WIDTH, sorted(real), stride, elements, first_out))

    # the rows that were never fed: a third push feeds and ends three of them, packed, and gives what a fresh stage gives
    fresh = [r for r in (0, n // 3, min(real) - 7) if r not in real]
    assert len(fresh) == 3
    lens3 = np.zeros(n, np.int64)
    for j, r in enumerate(fresh):
        lens3[r] = pool(r)[1 + j]
    chunks, (rec, _extent) = feed(lens3, fresh, 400)
    end = (lens3 > 0).astype(np.uint8)
    total = L.speechPlayer_stage_plan(h, p(lens3), p(end), p(counts))
    assert total == counts.sum() > 0
    (buf, body), (cbuf, cbody) = out.take(total * per, torch_type(fmt, spec)), cod.take(total, torch.uint8) if codes else (None, None)
    got = L.speechPlayer_stage_push(h, p(rec), p(end), body.data_ptr(), fmt, None if cbody is None else cbody.data_ptr(), 0, p(lengths), None)
    assert got == total * per and list(lengths) == list(counts), (kind, "third push", got, L.speechPlayer_lastError())
    torch.cuda.synchronize()
    assert intact(buf) and (cbuf is None or intact(cbuf))
    at = 0
    for j, r in enumerate(fresh):
        want = statement(r, x_of(chunks[j]), fmt)
        cnt = int(lengths[r])
        assert same(body[at * per:(at + cnt) * per].cpu().numpy().reshape(want[0].shape), want[0]), (kind, "row", r, "was not fresh")
        if codes:
            assert same(cbody[at:at + cnt].cpu().numpy(), want[1]), (kind, "row", r, "codes")
        at += cnt
    assert at == total
    L.speechPlayer_stage_free(h)
