"""The exports' 64-bit addressing run where it matters: outputs past elements 2^31 and 2^32 (a periodic selection of a small batch: every
later cycle is the first, and the first is the host statement), signals whose chosen rows lie past those elements, and a pool whose
utterances lie past sample 2^31 (include/speechPlayer_batch.h; csrc/klatt_tiles.h, klatt_timeline.h, klatt_export.h, klatt_filter.h,
klatt_codec.h, klatt_stems.h, klatt_response.h, klatt_spectrum.h, klatt_engine.hip: pcm_export).  A truncated index lands inside the
test's own buffer or reads poison: it shows as a wrong value, bit for bit.  The helpers are tests/far_offsets.py.  Needs a GPU with
some 30 GB free; a case that finds less skips and says so."""
import contextlib

import numpy as np
import pytest

from tests.far_offsets import B31, B32, far_packed_signal, far_padded_signal, periodic_mismatch, plan_cycles
from tests.test_codec_host import statement
from tests.test_convolve_host import decaying, x_of
from tests.test_alignment_host import COLUMNS, unit_first, unit_table
from tests.test_far_offsets_host import edge_groups
from tests.test_gpu_alignment import host_cases
from tests.test_gpu_codec import same
from tests.test_gpu_resample import rows_of
from tests.test_gpu_signal import edge_rows, poison
from tests.test_gpu_spectrogram import player
from tests.test_gpu_stems import wanted
from tests.test_gpu_timeline import Walked, set_host
from tests.test_gpu_timeline import same as same_nan
from tests.test_mix_host import bank
from tests.test_stems_host import OUTPUT, VOICE, compared

pytestmark = pytest.mark.gpu
GUARD = 64
ORDER = [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]      # a cycle of the ten-utterance batches: fixed, not sorted
POISON = {1: 0xC9, 2: -7, 4: -7, 8: -7}


def int_view(t):
    import torch
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def room(dev, need):
    """Skips unless `need` bytes and a tenth more are free, counting what torch holds from the cases before; that is given back only
    where the driver's free memory alone does not do (a case's buffers are dropped with the case, the allocation is kept for the next)."""
    import torch
    torch.cuda.init()
    free, _ = torch.cuda.mem_get_info(dev)
    held = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if free + held < need * 1.1:
        pytest.skip("needs %d bytes of device memory and a tenth more, %d are free" % (need, free + held))
    if free < need * 1.1:
        torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def give_back():
    """What the cases kept allocated goes back to the driver when the module is done."""
    yield
    import torch
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def peak(request):
    """Prints the most device memory torch held allocated during the case (profiles/far_offsets.txt)."""
    import torch
    torch.cuda.init()
    torch.cuda.reset_peak_memory_stats()
    yield
    print("peak %s: %.2f GB" % (request.node.name, torch.cuda.max_memory_allocated() / 1e9))


def guarded(dev, elements, dtype):
    """`elements` of poison (NaN; -7; 0xC9) between guards: -> (buffer, body)."""
    import torch
    room(dev, (elements + 2 * GUARD) * torch.empty(0, dtype=dtype).element_size() + (1 << 30))
    fill = float("nan") if dtype.is_floating_point else POISON[torch.empty(0, dtype=dtype).element_size()]
    buf = torch.full((elements + 2 * GUARD,), fill, dtype=dtype, device="cuda:%d" % dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + elements]


def guards_intact(buf):
    v = int_view(buf)
    fill = int_view(buf.new_full((1,), float("nan") if buf.dtype.is_floating_point else POISON[buf.element_size()]))[0]
    return bool((v[:GUARD] == fill).all()) and bool((v[-GUARD:] == fill).all())


def want_cycle(plan, rows, pad, npt):
    """One cycle as the export lays it out: rows[u] is [steps, ...] of utterance u; padded, each row is filled up with `pad`."""
    out = []
    for u in plan.cycle:
        r = np.ascontiguousarray(rows[u], dtype=npt).reshape(-1)
        assert len(r) % plan.per == 0
        out.append(r)
        if plan.rowStride:
            out.append(np.full(plan.rowStride * plan.per - len(r), pad, npt))
    out = np.concatenate(out)
    assert len(out) == plan.period
    return out


def check_cycles(buf, body, plan, want, got, tag, eq=same):
    """The return value, the crossing itself, the guards, every later cycle against the first on the device, and the first, the
    straddling and the last cycle against the host statement."""
    import torch
    assert got == plan.total == body.numel(), (tag, got, plan.total)
    last = (plan.repeats - 1) * plan.period
    assert last > max(plan.bounds), tag      # the last cycle begins past the largest bound
    torch.cuda.synchronize()
    assert guards_intact(buf), tag + ("guards",)
    bad = periodic_mismatch(int_view(body), plan.period)
    assert bad is None, tag + ("cycle %d differs from the first at offset %d" % bad if bad else "",)
    for k in sorted({0, plan.repeats - 1} | set(plan.straddles.values())):
        g = body[k * plan.period:(k + 1) * plan.period].cpu().numpy()
        assert eq(g, want), tag + ("cycle", k, "first element", k * plan.period)


@contextlib.contextmanager
def into_guarded(bp, kept, rows, rowStride, per, total):
    """bp's ...Tensor methods write `rows` rows of `per` elements a step, `total` elements in all, into a poisoned buffer between guards
    with the given rowStride instead of a fresh tensor: BatchPlayer._export_rows, which makes the output of every such method, is
    replaced on this player while the block runs."""
    import torch

    def export_rows(counts, tail_shape, dtype, padded, call, always=False):      # (always: the wrapper's, for empty outputs; none here)
        counts = np.asarray(counts, np.int64)
        assert per == int(np.prod(tail_shape, dtype=np.int64)) and bool(padded) == (rowStride > 0) and len(counts) == rows
        assert rowStride == 0 or rowStride >= counts.max()
        assert total == (len(counts) * rowStride if padded else int(counts.sum())) * per      # the buffer is what the export writes
        buf, body = guarded(bp.device, total, dtype)
        got = bp._check(call(body.data_ptr(), rowStride, total, torch.cuda.current_stream(bp.device).cuda_stream))
        kept.update(buf=buf, body=body, got=got)
        return body, torch.from_numpy(counts if padded else np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))

    bp._export_rows = export_rows
    try:
        yield
    finally:
        del bp._export_rows


class Export(object):
    """One export of a small batch: tail: an entry's shape; counts[u]: utterance u's entries; call(sel, padded) makes the ...Tensor call;
    rows[u]: the host's [entries, ...] of utterance u; pad: what lies past a padded row's end."""

    def __init__(self, tail, npt, counts, call, rows, pad=0, eq=same):
        self.tail, self.npt, self.counts, self.call, self.rows, self.pad, self.eq = tuple(tail), npt, np.asarray(counts, np.int64), call, rows, pad, eq

    def run(self, bp, padded, tag, order=ORDER):
        per = int(np.prod(self.tail, dtype=np.int64))
        bounds = (B31,) if np.dtype(self.npt).itemsize == 8 else (B31, B32)
        plan = plan_cycles(self.counts, per, bounds, padded, order)
        kept = {}
        with into_guarded(bp, kept, plan.repeats * len(plan.cycle), plan.rowStride, plan.per, plan.total):
            result = self.call(plan.selection(), padded)
        check_cycles(kept["buf"], kept["body"], plan, want_cycle(plan, self.rows, self.pad, self.npt), kept["got"], tag + (padded,), self.eq)
        print("far output %s: %d cycles of %d elements, %d rows, %.2f GB written" % (
            tag + (padded,), plan.repeats, plan.period, plan.repeats * len(plan.cycle), plan.total * np.dtype(self.npt).itemsize / 1e9))
        return plan, result, kept


def ipa_spec():
    """Two sampleIpa sentences, of 25 and of 32 units, each at two pitches and three times the speed (the two of tests/test_gpu_response.py:
    set_ipa have 6 and 12 units: no cycle of them has an odd number of units, and so short a cycle takes four times the rows)."""
    from nvspeechplayer_amd import workloads
    texts = workloads.cfg2_spec(1)["texts"]
    return dict(texts=[texts[2], texts[5]], speed=3.0, basePitch=[100.0, 130.0, 100.0, 130.0], clauseType=".", textOf=[0, 1, 0, 1])


def set_ipa(bp):
    bp.setIpa(noiseSeed=[1, 2, 3, 4], **ipa_spec())


def small(call, n):
    """The rows of a ...Tensor call on every utterance once, packed: what the module's neighbours hold to the restatements."""
    out, second = call(np.arange(n, dtype=np.int64), False)[:2]
    return rows_of(out, second, False)[0]


@pytest.fixture(scope="module")
def plain():
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    yield bp, pcm, s
    bp.close()


# ---- (a) far outputs ------------------------------------------------------------------------------------------------------------------------
def pcm_exports(bp, pcm, s):
    """The PCM-derived exports whose rows the host states: {name: Export}.  What a row gets -- its response, its filter, its terms, its
    gain -- goes by its UTTERANCE, so it repeats with the cycle whichever row the plan drops."""
    import torch
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    n, lens = s.n, np.array([len(p) for p in pcm], np.int64)
    td = {np.int16: torch.int16, np.float32: torch.float32}
    out = {}
    for npt in (np.int16, np.float32):
        out["pcm", npt] = Export((), npt, lens, lambda sel, padded, npt=npt: bp.pcmTensor(utterances=sel, dtype=td[npt], padded=padded),
                                 [p if npt == np.int16 else x_of(p) for p in pcm])
    out["resampled"] = Export((), np.int16, -(-lens * 320 // 441), lambda sel, padded: bp.resampledTensor(16000, utterances=sel, dtype=torch.int16, padded=padded),
                              [eng.pcmResample(p, s.sr, 16000, dtype=np.int16) for p in pcm])
    irs = [decaying(5, 31), decaying(1025, 32)]
    out["convolved"] = Export((), np.float32, lens + np.array([len(irs[u % 2]) - 1 for u in range(n)]),
                              lambda sel, padded: bp.convolvedTensor(irs, irOf=sel % 2, tail=True, utterances=sel, padded=padded),
                              [eng.pcmConvolve(p, irs[u % 2]) for u, p in enumerate(pcm)])
    filters = [eng.preEmphasis(), np.concatenate([eng.biquad("lowpass", s.sr, 3000.0), eng.biquad("peaking", s.sr, 800.0, 2.0, 6.0), eng.dcBlock()])]
    assert [len(f) for f in filters] == [1, 3]
    out["filtered"] = Export((), np.int16, lens, lambda sel, padded: bp.filteredTensor(filters, filterOf=sel % 2, utterances=sel, dtype=torch.int16, padded=padded),
                             [eng.pcmFilter(p, filters[u % 2], dtype=np.int16) for u, p in enumerate(pcm)])
    out["spectrogram"] = Export((33,), np.float32, -(-lens // 16), lambda sel, padded: bp.spectrogramTensor(nFft=64, hop=16, utterances=sel, padded=padded),
                                [eng.pcmSpectrogram(p, nFft=64, hop=16).astype(np.float32) for p in pcm])
    # mixed: a noise term on every row, another utterance on two rows of three, a gain per row
    clips = bank()
    bp.setNoiseBank(clips)
    big = [k for k, c in enumerate(clips) if len(c) > 100 and c.any()]
    dev_terms = [[M(noise=big[u % len(big)], snr=12.0 - u, offset=3 * u)] + ([M(utterance=(u + 3) % n, snr=3.0, loop=False, offset=-2)] if u % 3 else []) for u in range(n)]
    host_terms = [[M(noise=big[u % len(big)], snr=12.0 - u, offset=3 * u)] + ([M(utterance=len(clips) + (u + 3) % n, snr=3.0, loop=False, offset=-2)] if u % 3 else []) for u in range(n)]
    gain = np.array([1.0 - 0.05 * u for u in range(n)], np.float32)
    mixed = [eng.pcmMix(pcm[u], clips + pcm, host_terms[u], speechGain=gain[u], gains=True) for u in range(n)]
    records = [np.array([t.record() for t in row], eng.mixTermDtype) for row in dev_terms]

    def mix(sel, padded):
        cyc = next(c for c in range(1, n + 1) if len(sel) % c == 0 and np.array_equal(sel[:c], sel[c:2 * c]))      # the cycle's rows
        flat = np.tile(np.concatenate([records[u] for u in sel[:cyc]]), len(sel) // cyc)
        start = np.concatenate([[0], np.cumsum(np.array([len(r) for r in records], np.int64)[sel])]).astype(np.int64)
        return bp.mixedTensor((flat, start), speechGain=gain[sel], utterances=sel, padded=padded, gains=True)
    out["mixed"] = Export((), np.float32, lens, mix, [m for m, _ in mixed])
    out["mixed"].gains = [g for _, g in mixed]
    return out


PCM_CASES = [("pcm", np.int16), ("pcm", np.float32), "resampled", "convolved", "filtered", "spectrogram", "mixed"]


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("name", PCM_CASES, ids=lambda c: c if isinstance(c, str) else "%s-%s" % (c[0], c[1].__name__))
def test_far_outputs_of_the_pcm_exports(plain, name, padded):
    """exportPcm, Resampled (22 050 -> 16 000), Convolved (two responses, the tail on), Filtered (one and three sections), Spectrogram
    (nFft 64, hop 16) and Mixed (noise and another utterance, the gains returned) past elements 2^31 and 2^32, packed and padded."""
    bp, pcm, s = plain
    case = pcm_exports(bp, pcm, s)[name]
    plan, result, kept = case.run(bp, padded, (str(name),))
    if name == "mixed":      # the gains applied: one per term, periodic with the cycle, the host's in the first
        applied = result[2]
        want = np.concatenate([case.gains[u] for u in plan.cycle])
        assert applied.numel() == plan.repeats * len(want)
        assert periodic_mismatch(int_view(applied), len(want)) is None and same(applied[:len(want)].cpu().numpy(), want)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("codec", ["ulaw", "adpcm"])
def test_far_outputs_of_the_codecs(plain, codec, padded):
    """exportCoded, both outputs at once through the entry point: int16 decoded samples and uint8 codes past elements 2^31 and 2^32; a
    padded row has the natural stride, made odd (the ADPCM kernel walks a row's stride serially)."""
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    bp, pcm, s = plain
    lens = np.array([len(p) for p in pcm], np.int64)
    plan = plan_cycles(lens, 1, (B31, B32), padded, ORDER)
    want = [statement(p, codec) for p in pcm]
    sel = plan.selection()
    src = bp._rows("codedTensor", None, sel)
    (dbuf, d), (cbuf, c) = guarded(bp.device, plan.total, torch.int16), guarded(bp.device, plan.total, torch.uint8)
    got = bp._check(bp._entry("Coded", src)(sp.CODECS.index(codec), d.data_ptr(), 0, c.data_ptr(), plan.rowStride, torch.cuda.current_stream(bp.device).cuda_stream))
    for which, (buf, body, npt) in enumerate(((dbuf, d, np.int16), (cbuf, c, np.uint8))):
        check_cycles(buf, body, plan, want_cycle(plan, [w[which] for w in want], 0, npt), got, (codec, padded, which))


def dense_exports(bp, s, ipa):
    """The exports of the frame lists, 8-byte and 4-byte elements: {name: Export}.  Tracks are held to the walk of
    tests/test_timeline_host.py, alignment and units to align_walk and unit_table of tests/test_alignment_host.py.  Source, epochs and
    response are held to the SAME export of every utterance once: tests/test_gpu_source.py and test_gpu_response.py hold those near
    exports to restatements that are exact only within bounds, so bit for bit the far rows can be held to the near ones alone."""
    import torch
    n = ipa.nUtterances if ipa is not None else s.n
    out = {}
    if ipa is None:
        w = Walked(s.b)
        lens = np.array([w.length(u) for u in range(n)], np.int64)
        cols = [0, 7, 44]      # voicePitch (the pitch table), a formant, the gated gain
        for npt, td in ((np.float32, torch.float32), (np.float64, torch.float64)):
            out["tracks", npt] = Export((3,), npt, -(-lens // 4), lambda sel, padded, td=td: bp.trackTensor(cols, hop=4, utterances=sel, dtype=td, padded=padded),
                                        [w.expected(u, cols, hop=4, dtype=npt) for u in range(n)], eq=same_nan)
        calls = {"source": ((2,), np.float64, -(-lens // 2), lambda sel, padded: bp.sourceTensor(["f0", "wave"], hop=2, utterances=sel, dtype=torch.float64, padded=padded), 0.0),
                 "epochs": ((4,), np.float64, bp.epochCounts(), lambda sel, padded: bp.epochTensor(utterances=sel, padded=padded), -1.0),
                 "response": ((2, 64), np.float64, -(-lens // 64), lambda sel, padded: bp.responseTensor(64, hop=64, utterances=sel, dtype=torch.float64, padded=padded), 0.0)}
        for name, (tail, npt, counts, call, pad) in calls.items():
            out[name] = Export(tail, npt, counts, call, small(call, n), pad=pad, eq=same_nan)
    else:
        cases = host_cases(**ipa_spec())
        lens = np.array([c.length for c in cases], np.int64)
        assert [ipa.utteranceSamples(u) for u in range(n)] == list(lens) and list(ipa.unitCounts()) == [len(unit_first(c.labels)) - 1 for c in cases]
        phase = 0 if (lens % 2).any() else 1      # (four even lengths: from sample 1 on, each has an odd number of steps)
        cols = ["phoneme", "position"]
        out["alignment"] = Export((2,), np.int32, lens - phase, lambda sel, padded: ipa.alignmentTensor(cols, phase=phase, utterances=sel, dtype=torch.int32, padded=padded),
                                  [c.dense([COLUMNS.index(k) for k in cols], 1, phase) for c in cases], pad=-1)
        out["units"] = Export((7,), np.int64, ipa.unitCounts(), lambda sel, padded: ipa.unitTensor(hop=1, utterances=sel, padded=padded),
                              [unit_table(c.first, c.labels, 1, 0, "unit") for c in cases], pad=-1)
    return out


@pytest.fixture(scope="module")
def wild():
    import nvspeechplayer_amd as eng
    s = compared("wild")
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    yield bp, s
    bp.close()


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("name", [("tracks", np.float32), ("tracks", np.float64), "source", "epochs", "response"],
                         ids=lambda c: c if isinstance(c, str) else "%s-%s" % (c[0], c[1].__name__))
def test_far_outputs_of_the_frame_list_exports(wild, name, padded):
    """Tracks (three columns, voicePitch among them; float32 past 2^32, float64 past 2^31), Source, Epochs and Response (two kinds at 64
    frequencies) of the wild batch."""
    bp, s = wild
    dense_exports(bp, s, None)[name].run(bp, padded, (str(name),))


@pytest.mark.parametrize("padded", [False, True])
def test_far_outputs_of_the_lane_per_list_source_walk(padded):
    """Option "source_lane_lists" = 1: the other walk behind klatt_source_dense."""
    import nvspeechplayer_amd as eng
    s = compared("wild")
    bp = eng.BatchPlayer(s.sr)
    bp.setOption("source_lane_lists", 1)
    set_host(bp, s.b)
    dense_exports(bp, s, None)["source"].run(bp, padded, ("source, one lane per list",))
    bp.close()


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("name", ["alignment", "units"])
def test_far_outputs_of_the_label_exports(name, padded):
    """Alignment (int32, past 2^32) and Units (int64, past 2^31) of a batch set from IPA text."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    set_ipa(bp)
    dense_exports(bp, None, bp)[name].run(bp, padded, (name,), order=[2, 0, 3, 1])
    bp.close()


@pytest.mark.parametrize("padded", [False, True])
def test_far_outputs_of_the_stems(plain, padded):
    """Stems of the plain batch, two columns, float64 past element 2^31 through the entry point, against the restatement of
    tests/test_stems_host.py (bit for bit on this batch: tests/test_gpu_stems.py): a row holds its columns one after the other, so the
    period is the cycle's samples (made odd) times two; the natural stride (the kernel walks a row serially)."""
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    bp, _, s = plain
    cols, fmt = sp.check_stem_request(["voice", "output"], torch.float64)
    lens = np.array([bp.utteranceSamples(u) for u in range(s.n)], np.int64)
    rows = [np.ascontiguousarray(w[:, [VOICE, OUTPUT]].T) for w in wanted("plain")]
    assert [r.shape for r in rows] == [(2, int(L)) for L in lens]
    plan = plan_cycles(lens, 2, (B31,), padded, ORDER)
    if padded:      # [row][column][rowStride]
        want = np.zeros((len(plan.cycle), 2, plan.rowStride), np.float64)
        for i, u in enumerate(plan.cycle):
            want[i, :, :lens[u]] = rows[u]
        want = want.reshape(-1)
    else:
        want = np.concatenate([rows[u].reshape(-1) for u in plan.cycle])
    assert len(want) == plan.period
    src = bp._rows("stemTensor", None, plan.selection())
    buf, body = guarded(bp.device, plan.total, torch.float64)
    got = bp._check(bp._entry("Stems", src)(cols.ctypes.data, len(cols), body.data_ptr(), fmt, plan.rowStride, torch.cuda.current_stream(bp.device).cuda_stream))
    check_cycles(buf, body, plan, want, got, ("stems", padded), same_nan)


@pytest.mark.parametrize("name", ["tracks", "source", "alignment"])
def test_rows_beyond_2_32_elements_of_an_inflated_stride(request, name):
    """The three kernels that place their lanes with dense_locate, padded with rowStride 2^30 + 5 and two columns of 4 bytes: three rows,
    the last of which begins past element 2^32 -- the 64-bit e0 / nCols with live values behind it.  The padding carries the count.
    Each row is the same export of its utterance alone (the near rows: tests/test_gpu_timeline.py, test_gpu_source.py, test_gpu_alignment.py)."""
    import torch
    import nvspeechplayer_amd as eng
    stride, per = (1 << 30) + 5, 2
    if name == "alignment":
        bp = eng.BatchPlayer(22050)
        set_ipa(bp)
        call = lambda sel, padded: bp.alignmentTensor(["phoneme", "position"], utterances=sel, dtype=torch.int32, padded=padded)
        pad, npt, eq = -1, np.int32, same
    else:
        bp, _ = request.getfixturevalue("wild")
        call = {"tracks": lambda sel, padded: bp.trackTensor([0, 7], utterances=sel, padded=padded),
                "source": lambda sel, padded: bp.sourceTensor(["f0", "wave"], utterances=sel, padded=padded)}[name]
        pad, npt, eq = 0, np.float32, same_nan
    sel = np.array([5, 1, 2], np.int64) % bp.nUtterances
    want = small(call, bp.nUtterances)
    total = len(sel) * stride * per
    assert (len(sel) - 1) * stride * per > B32 and total * 4 < 27e9      # the last row begins past element 2^32
    kept = {}
    with into_guarded(bp, kept, len(sel), stride, per, total):
        call(sel, True)
    torch.cuda.synchronize()
    assert kept["got"] == total and guards_intact(kept["buf"])
    body = kept["body"].view(len(sel), stride * per)
    fill = int_view(body.new_full((1,), pad))[0]
    for i, u in enumerate(sel):
        live = want[u].size
        assert 0 < live < stride * per and eq(body[i, :live].cpu().numpy(), np.ascontiguousarray(want[u], dtype=npt).reshape(-1)), (name, i)
        for a in range(live, stride * per, 1 << 28):      # the padding, in slabs
            assert bool((int_view(body[i, a:a + (1 << 28)]) == fill).all()), (name, i, "padding from", a)
    if name == "alignment":
        bp.close()


# ---- (b) far inputs -------------------------------------------------------------------------------------------------------------------------
def signal_exports(bp, order, rows):
    """Every ...Of export of the rows rows[k], k in `order`, packed: {name: (export(signal, row number of k) -> (out, offsets), host
    statement of output row i)}.  A row's response and filter go by its place in the output; a term's source is the next chosen row."""
    import torch
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    irs = [decaying(5, 41), decaying(1025, 42)]
    filters = [eng.preEmphasis(), np.concatenate([eng.biquad("lowpass", 22050, 3000.0), eng.biquad("peaking", 22050, 800.0, 2.0, 6.0), eng.dcBlock()])]
    m = len(order)
    of = np.arange(m) % 2
    nxt = [order[(i + 1) % m] for i in range(m)]
    sel = lambda at: np.array([at(k) for k in order], np.int64)
    out = {
        "spectrogram": (lambda sig, at: bp.spectrogramTensor(nFft=64, hop=16, utterances=sel(at), padded=False, dtype=torch.float64, signal=sig),
                        lambda i, x: eng.signalSpectrogram(x, nFft=64, hop=16)),
        "resampled": (lambda sig, at: bp.resampledTensor(16000, utterances=sel(at), padded=False, signal=sig), lambda i, x: eng.signalResample(x, 22050, 16000)),
        "convolved": (lambda sig, at: bp.convolvedTensor(irs, irOf=of, utterances=sel(at), padded=False, signal=sig), lambda i, x: eng.signalConvolve(x, irs[of[i]])),
        "filtered": (lambda sig, at: bp.filteredTensor(filters, filterOf=of, tail=3, utterances=sel(at), padded=False, signal=sig),
                     lambda i, x: eng.signalFilter(x, filters[of[i]], tail=3)),
        "mixed": (lambda sig, at: bp.mixedTensor([[M(utterance=int(at(k)), snr=6.0, loop=False, offset=1)] for k in nxt], utterances=sel(at), padded=False, signal=sig),
                  lambda i, x: eng.signalMix(x, [rows[nxt[i]]], [M(utterance=0, snr=6.0, loop=False, offset=1)])),
    }
    for codec in ("ulaw", "alaw", "adpcm"):
        out[codec] = (lambda sig, at, codec=codec: bp.codedTensor(codec, utterances=sel(at), padded=False, signal=sig), lambda i, x, codec=codec: eng.signalCode(x, codec))
        out[codec + " codes"] = (lambda sig, at, codec=codec: bp.codedTensor(codec, codes=True, decoded=False, utterances=sel(at), padded=False, signal=sig),
                                 lambda i, x, codec=codec: eng.signalCode(x, codec, codes=True, decoded=False))
    return out


def check_far_signal(bp, tensor, second, real, rows, tag):
    """real[k]: the signal's row that holds rows[k].  The chosen rows out of order, one twice, through every ...Of export: each output
    row is the host statement of its row, and the same export of the rows laid out as a small signal."""
    import torch
    import nvspeechplayer_amd as eng
    order = [len(real) - 1, 0] + list(range(1, len(real) - 1)) + [0]
    near = (torch.from_numpy(np.concatenate(rows)).to(tensor.device), torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)))
    for name, (export, host) in signal_exports(bp, order, rows).items():
        far_rows = rows_of(*export((tensor, second), lambda k: real[k])[:2], False)[0]
        near_rows = rows_of(*export(near, lambda k: k)[:2], False)[0]
        assert len(far_rows) == len(near_rows) == len(order)
        for i, k in enumerate(order):
            w = host(i, rows[k])
            assert (same_nan if w.dtype.kind == "f" else same)(far_rows[i], w), tag + (name, "row", int(real[k]), "the statement")
            assert same(far_rows[i], near_rows[i]), tag + (name, "row", int(real[k]), "the small signal")
    sel = np.array([real[k] for k in order], np.int64)
    power, lens = bp.powerTensor(utterances=sel, signal=(tensor, second))
    assert [float(p) for p in power.cpu()] == [eng.signalPower(rows[k]) for k in order] and [int(v) for v in lens.cpu()] == [len(rows[k]) for k in order], tag


@pytest.mark.parametrize("npt", [np.int16, np.float32])
def test_far_inputs_a_signal_whose_chosen_rows_lie_beyond_the_bounds(npt):
    """One poisoned tensor -- int16 to past element 2^32, float32 to past 2^31 (byte 2^33) -- taken as a packed signal (fillers that
    are never chosen up to the bounds, rows of the tiles' edge lengths on odd elements straddling and after them) and as a padded one of
    an odd width near 2^20 (all rows of length 0 but those around the bounds)."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    dev = "cuda:%d" % bp.device
    _, g31, g32 = edge_groups()
    width = (1 << 20) - 1
    groups, bounds = ([g31, g32], (B31, B32)) if npt == np.int16 else ([g31], (B31,))
    packed = far_packed_signal(groups, bounds)
    pgroups = ([[2305, 1023, 65, 1], [4353, 257, 1, 1025, 64]] if npt == np.int16 else [[2305, 1023, 65, 1]])
    n, plens, preal, pstraddle = far_padded_signal(pgroups, bounds, width)
    numel = max(packed.need, n * width)
    td = torch.int16 if npt == np.int16 else torch.float32
    room(bp.device, numel * np.dtype(npt).itemsize + (1 << 30))
    seed = torch.from_numpy(poison(1 << 20, npt).view(np.int16 if npt == np.int16 else np.int32)).to(dev)

    def poisoned():
        t = torch.empty(numel, dtype=seed.dtype, device=dev)
        whole = numel - numel % len(seed)
        t[:whole].view(-1, len(seed))[:] = seed
        t[whole:] = seed[:numel - whole]
        return t.view(td)

    tensor = poisoned()
    # packed: the extents say where the rows lie; the crossing itself
    rows = edge_rows([packed.length(r) for r in packed.real], npt, 31)
    for r, x in zip(packed.real, rows):
        tensor[packed.start(r):packed.start(r) + len(x)] = torch.from_numpy(x).to(dev)
    for b in bounds:
        r = packed.straddlers[b]
        assert packed.start(r) < b < packed.start(r) + packed.length(r) - 1 and r in packed.real
    assert all(packed.start(r) % 2 == 1 for r in packed.real) and sum(packed.start(r) > max(bounds) for r in packed.real) >= 3
    check_far_signal(bp, tensor, torch.from_numpy(packed.extent), packed.real, rows, (npt.__name__, "packed"))
    # padded: the same tensor, poisoned again, [n, width]
    del tensor
    tensor = poisoned()[:n * width].view(n, width)
    rows = edge_rows([int(plens[r]) for r in preal], npt, 32)
    for r, x in zip(preal, rows):
        tensor[r, :len(x)] = torch.from_numpy(x).to(dev)
    for b in bounds:
        r = pstraddle[b]
        assert r * width < b < r * width + plens[r] - 1
    assert width % 2 == 1 and int((plens > 0).sum()) == len(preal)
    check_far_signal(bp, tensor, torch.from_numpy(plens), preal, rows, (npt.__name__, "padded"))
    print("far input %s: %d elements" % (npt.__name__, numel))
    del tensor
    bp.close()


# ---- (c) a far pool -------------------------------------------------------------------------------------------------------------------------
def test_far_pool_utterances_past_sample_2_31():
    """configs[2] with as many utterances as put the last four past sample 2^31 of the PCM pool: the exports of the first utterance, the
    last three and the one that holds sample 2^31 against the host statements of what read() gives; the packed int16 PCM of ALL
    utterances -- past element 2^31, nothing periodic -- against the pool itself, row for row on the device."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    M = eng.MixTerm
    per = int(workloads.sample_counts("cfg2", 512).sum())
    counts = workloads.sample_counts("cfg2", (B31 // per + 2) * 512)
    cum = np.concatenate([[0], np.cumsum(counts)])
    n = int(np.searchsorted(cum, B31, side="right")) + 4      # the smallest n with utterance n - 4 past sample 2^31, by the counts
    bp = eng.BatchPlayer(22050)
    room(bp.device, 3 * 2 * (B31 + (1 << 28)))
    bp.setIpa(**workloads.cfg2_spec(n))
    bp.synthesize()
    assert bp.deviceOffset(n - 4) > B31 >= cum[n - 5]
    lens = bp._lengths()
    offs = np.array([bp.deviceOffset(u) for u in (0, n - 3, n - 2, n - 1)])
    lo, hi = 0, n - 1      # the utterance whose pool range holds sample 2^31
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if bp.deviceOffset(mid) <= B31 else (lo, mid - 1)
    across = lo
    assert bp.deviceOffset(across) <= B31 < bp.deviceOffset(across) + int(lens[across]) and offs[1] > B31
    sel = [n - 1, 0, across, n - 3, n - 2, across]
    pcm = {u: bp.read(u).copy() for u in set(sel)}
    assert all(len(pcm[u]) == lens[u] and pcm[u].any() for u in sel)
    irs = [decaying(5, 51), decaying(1025, 52)]
    of = np.arange(len(sel)) % 2
    filters = [eng.preEmphasis(), np.concatenate([eng.biquad("lowpass", 22050, 3000.0), eng.dcBlock()])]
    terms = [[M(utterance=sel[(i + 1) % len(sel)], snr=6.0, offset=1)] for i in range(len(sel))]
    cases = {
        "pcm": (lambda: bp.pcmTensor(utterances=sel, dtype=torch.int16, padded=False), lambda i, p: p),
        "spectrogram": (lambda: bp.spectrogramTensor(nFft=64, hop=16, utterances=sel, padded=False, dtype=torch.float64), lambda i, p: eng.pcmSpectrogram(p, nFft=64, hop=16)),
        "resampled": (lambda: bp.resampledTensor(16000, utterances=sel, padded=False), lambda i, p: eng.pcmResample(p, 22050, 16000)),
        "convolved": (lambda: bp.convolvedTensor(irs, irOf=of, utterances=sel, padded=False), lambda i, p: eng.pcmConvolve(p, irs[of[i]])),
        "filtered": (lambda: bp.filteredTensor(filters, filterOf=of, utterances=sel, padded=False), lambda i, p: eng.pcmFilter(p, filters[of[i]])),
        "ulaw": (lambda: bp.codedTensor("ulaw", utterances=sel, padded=False), lambda i, p: eng.pcmCode(p, "ulaw")),
        "adpcm": (lambda: bp.codedTensor("adpcm", codes=True, decoded=False, utterances=sel, padded=False), lambda i, p: eng.pcmCode(p, "adpcm", codes=True, decoded=False)),
        "mixed": (lambda: bp.mixedTensor(terms, utterances=sel, padded=False), lambda i, p: eng.pcmMix(p, [pcm[sel[(i + 1) % len(sel)]]], [M(utterance=0, snr=6.0, offset=1)])),
    }
    for name, (export, host) in cases.items():
        got = rows_of(*export()[:2], False)[0]
        for i, u in enumerate(sel):
            assert same(got[i], host(i, pcm[u])), (name, "utterance", u, "at sample", bp.deviceOffset(u))
    sums, _ = bp.powerTensor(utterances=sel)
    assert [int(v) for v in sums.cpu()] == [int((pcm[u].astype(np.int64) ** 2).sum()) for u in sel]
    # every utterance, packed: past element 2^31 with nothing periodic in it
    out, second = bp.pcmTensor(dtype=torch.int16, padded=False)
    second = second.numpy()
    assert out.numel() == int(lens.sum()) > B31 and second[n - 3] > B31
    at = int(np.searchsorted(second, B31))      # the rows around element 2^31 of the output
    near = list(range(max(0, at - 3), min(n, at + 3)))
    sample = sorted(set(list(range(0, n, max(1, n // 200))) + near + [across - 1, across, across + 1, n - 1]))
    pcm_all = pool_view(bp, int(bp.deviceOffset(n)))
    for u in sample:
        a = bp.deviceOffset(u)
        assert torch.equal(out[second[u]:second[u + 1]], pcm_all[a:a + int(lens[u])]), ("utterance", u, "pool sample", a, "element", int(second[u]))
    print("far pool: %d utterances, %d samples" % (n, int(lens.sum())))
    del out, pcm_all
    bp.close()


def pool_view(bp, samples):
    """The batch's PCM pool as an int16 torch tensor of `samples` elements (devicePcm is its address)."""
    import torch

    class Pool(object):
        __cuda_array_interface__ = dict(shape=(samples,), typestr="<i2", data=(int(bp.devicePcm()), False), version=2)
    return torch.as_tensor(Pool(), device="cuda:%d" % bp.device)
