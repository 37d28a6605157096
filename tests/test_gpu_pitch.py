"""Pitch estimated from a batch's PCM and from a signal's rows (include/speechPlayer_batch.h: speechPlayer_batch_exportPitch, exportPitchOf;
BatchPlayer.pitchTensor; csrc/klatt_pitch.h) against the host's statements of the definition -- speechPlayer_pcmPitch / signalPitch applied
to what the engine read -- bit for bit, on integer views; and against the truth: the fundamental sourceTensor states for steady vowels.
The statements themselves are held to a transcription by tests/test_pitch_host.py.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_gpu_lpc import the_batch, NULL, SHORT, SILENT
from tests.test_gpu_signal import lay_out, poison, record
from tests.test_gpu_spectrogram import player, rows_of
from tests.test_gpu_timeline import set_host
from tests.test_lpc_host import bits, float_row, golden_pcm
from tests.test_pitch_host import PITCHES, TRUTH_RATE, VOWELS, inside_steps, vowel_frames
from tests.test_stems_host import compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64
ALL = 63


@pytest.fixture(scope="module")
def batch():
    """The thirteen utterances of tests/test_gpu_lpc.py in MODE_EXACT: ten of 840 .. 5860 samples, one of none, one of 3 samples (shorter
    than every frame here) and one with a long exact silence inside."""
    bp, pcm = player(the_batch())
    assert len(pcm) == 13 and len(pcm[NULL]) == 0 and len(pcm[SHORT]) == 3 and len(pcm[SILENT]) > 7000
    yield bp, pcm
    bp.close()


@pytest.fixture(scope="module")
def bare():
    """A player that was never set: the exports of a signal need no batch content."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    yield bp
    bp.close()


def statement_of(row, rate, **kw):
    import nvspeechplayer_amd as eng
    return (eng.pcmPitch if row.dtype == np.int16 else eng.signalPitch)(row, rate, **kw)


def check_pitch(bp, rows, kw, forms, tag, sel=None, signal=None, rate=22050):
    """pitchTensor in each of `forms` (dtype, padded) against the statement of every chosen row: shapes, step counts, bits, +0 padding."""
    import torch
    idx = list(range(len(rows))) if sel is None else list(sel)
    want = [statement_of(rows[u], rate, **kw) for u in idx]
    steps = [len(w) for w in want]
    for dtype, padded in forms:
        npt = np.float32 if dtype == torch.float32 else np.float64
        out, second = bp.pitchTensor(dtype=dtype, padded=padded, utterances=sel, signal=signal, sampleRate=None if signal is None else rate, **kw)
        assert out.dtype == dtype and list(second.numpy()) == (steps if padded else list(np.concatenate([[0], np.cumsum(steps)]))), tag
        assert tuple(out.shape) == ((len(idx), max(steps, default=0), want[0].shape[1]) if padded else (sum(steps), want[0].shape[1])), tag
        got, past = rows_of(out, second, padded)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(bits(g), bits(w.astype(npt))), tag + (dtype, padded, i, idx[i])
        for i, z in enumerate(past):
            assert not bits(z).any(), tag + ("padding", i)
    return want


def every_form():
    import torch
    return [(torch.float64, True), (torch.float32, False), (torch.float64, False), (torch.float32, True)]


# ---- 1. the pool form against the host statement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lags", [(2, 3), (2, 65), (44, 368), (1023, 1024)])
@pytest.mark.parametrize("W", [32, 34, 401, 2048])
def test_pitch_is_the_statements_bits(batch, W, lags):
    """The thirteen utterances, every field at once, float64 and float32, padded and packed: a hop that gives a few steps a row at phase
    0 and 7, and -- the short frames -- hop 1 on the three shortest rows.  The four output forms are rotated over the combinations, two
    forms each, so that every form meets every (W, lags)."""
    bp, pcm = batch
    lagMin, lagMax = lags
    forms = every_form()
    big = W == 2048 or lagMax == 1024
    k = 0
    for hop, sel in ((997 if big else 160, None), (8192, None)) + (() if big else ((1, [SHORT, 9, NULL, 8]),)):
        for phase, threshold in ((0, 0.15), (7, 0.5)):
            kw = dict(nWin=W, lagMin=lagMin, lagMax=lagMax, threshold=threshold, hop=hop, phase=phase, fields=ALL)
            want = check_pitch(bp, pcm, kw, forms[k % 4:k % 4 + 2] if k % 4 < 3 else [forms[3], forms[0]], (W, lags, hop, phase), sel=sel)
            k += 1
            if hop < 8192 and lags == (44, 368) and W >= 401 and sel is None:      # the batch holds voiced and unvoiced steps
                voiced = np.concatenate([w[:, 4] for w in want])
                assert (voiced == 1).any() and (voiced == 0).any()


def test_every_field_alone_a_selection_with_repeats_and_step_counts_around_16(batch):
    """Each field alone and some sets; a selection with repeats in reverse order; hops that give the longest utterance 15, 16, 17 and 33
    steps (whole groups of the kernel and a step either side), twice over, with the 3-sample utterance behind."""
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    bp, pcm = batch
    forms = every_form()
    assert sp.PITCH_GROUP == 16
    for k, fields in enumerate([(f,) for f in sp.PITCH_FIELDS] + [("f0", "aperiodicity"), ("cmnd", "lag"), ("voiced", "period", "f0")]):
        check_pitch(bp, pcm, dict(nWin=300, lagMin=30, lagMax=200, threshold=0.2, hop=160, phase=3, fields=fields), [forms[k % 4]], ("fields", fields))
    sel = [12, 11, 10, 9, 9, 5, 2, 2, 0]
    check_pitch(bp, pcm, dict(nWin=256, lagMin=44, lagMax=368, hop=100, phase=0, fields=("f0", "aperiodicity")), forms, ("selection",), sel=sel)
    L = len(pcm[2])
    for steps in (15, 16, 17, 33):
        hop = next(h for h in range(1, L) if -(-L // h) == steps)
        want = check_pitch(bp, pcm, dict(nWin=128, lagMin=20, lagMax=130, threshold=0.3, hop=hop, phase=0, fields=ALL), forms[:2], ("steps", steps), sel=[2, 2, 11])
        assert len(want[0]) == steps
    none = bp.pitchTensor(nWin=64, hop=160, utterances=[NULL, NULL], dtype=torch.float64)      # rows of nothing: nothing to launch
    assert tuple(none[0].shape) == (2, 0, 2) and list(none[1].numpy()) == [0, 0]


def test_the_raw_entry_point_on_a_side_stream_into_a_misaligned_buffer(batch):
    """speechPlayer_batch_exportPitch on a non-default stream, the output one element past a 16-byte boundary, between guards: float64 and
    float32, padded and packed."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    bp, pcm = batch
    dev = "cuda:%d" % bp.device
    sel = np.array([7, 12, 0, 11, 10, 3], np.int64)
    want = [eng.pcmPitch(pcm[u], 22050, nWin=400, lagMin=40, lagMax=300, threshold=0.25, hop=160, phase=7, fields=ALL) for u in sel]
    steps, cols = [len(w) for w in want], want[0].shape[1]
    side = torch.cuda.Stream(device=dev)
    for fmt, dtype, npt in ((0, torch.float64, np.float64), (1, torch.float32, np.float32)):
        for stride in (0, max(steps) + 2):
            elements = (sum(steps) if stride == 0 else len(sel) * stride) * cols
            buf = torch.full((elements + 2 * GUARD + 1,), -7.0, dtype=dtype, device=dev)
            torch.cuda.synchronize()
            out = buf.data_ptr() + (GUARD + 1) * buf.element_size()
            assert buf.data_ptr() % 16 == 0 and out % 16 != 0
            got = L.speechPlayer_batch_exportPitch(bp._h, sel.ctypes.data, len(sel), 400, 40, 300, 0.25, 160, 7, ALL, out, fmt, stride, side.cuda_stream)
            assert got == elements, (fmt, stride, L.speechPlayer_lastError())
            side.synchronize()
            a = buf.cpu().numpy()
            assert np.all(a[:GUARD + 1] == -7.0) and np.all(a[GUARD + 1 + elements:] == -7.0), (fmt, stride, "guards")
            a, at = a[GUARD + 1:GUARD + 1 + elements], 0
            for i, w in enumerate(want):
                span = (len(w) if stride == 0 else stride) * cols
                assert np.array_equal(bits(a[at:at + w.size]), bits(w.astype(npt).reshape(-1))), (fmt, stride, i)
                assert not bits(a[at + w.size:at + span]).any(), (fmt, stride, i, "padding")
                at += span


# ---- 2. signal= ---------------------------------------------------------------------------------------------------------------------------------
def test_the_signal_forms(bare):
    """Hand-made int16 and float32 signals with poison either side of every row (padded: in the rows' remainders; packed: before the first
    and behind the last), rows chosen out of order with a repeat, on a player that was never set: the statement's bits at the signal's own
    rate, and the signal unchanged afterwards.  Row lengths give 16 and 17 steps among others."""
    import torch
    forms = every_form()
    dev = "cuda:%d" % bare.device
    hop = 40
    lens = [16 * hop, 16 * hop + 1, 0, 3, 1500, 199, 33 * hop]
    for npt in (np.int16, np.float32):
        src = golden_pcm("ipa_l15_s10_c0_p100_i05")
        rows = [src[700 + 13 * i:700 + 13 * i + L].copy() for i, L in enumerate(lens)]
        rows = rows if npt == np.int16 else [float_row(r) for r in rows]
        for stride, shift in ((max(lens) + 5, 1), (0, 3)):
            host, first, extent = lay_out(rows, npt, stride, poison, shift)
            data = torch.from_numpy(host.view(np.int32 if npt == np.float32 else np.int16)).to(dev)
            before = data.clone()
            body = data.view(torch.float32 if npt == np.float32 else torch.int16)[first:first + (len(rows) * stride if stride else sum(lens))]
            signal = (body.view(len(rows), stride), torch.from_numpy(extent)) if stride else (body, torch.from_numpy(extent))
            sel = [6, 1, 0, 4, 2, 3, 1, 5]
            want = check_pitch(bare, rows, dict(nWin=65, lagMin=16, lagMax=134, threshold=0.3, hop=hop, phase=0, fields=ALL), forms[:2] if stride else forms[2:],
                               ("made", npt.__name__, stride), sel=sel, signal=signal, rate=8000)
            assert [len(w) for w in want[:3]] == [33, 17, 16]
            torch.cuda.synchronize()
            assert torch.equal(data, before), "the signal and its guards are as they were"
    with pytest.raises(ValueError, match="needs its sampleRate"):
        bare.pitchTensor(signal=signal)
    with pytest.raises(ValueError, match="comes with a signal"):
        bare.pitchTensor(sampleRate=16000)


def test_the_chain_mixed_resampled_pitch(batch):
    """pitchTensor(signal=resampledTensor(16000, signal=mixedTensor(...)), sampleRate=16000) is signalPitch of the same rows: the front end's
    view of a noisy row at 16 kHz, nothing leaving the device in between."""
    import torch
    import nvspeechplayer_amd as eng
    bp, pcm = batch
    sel = [2, 12, 11, 0, 10]
    terms = [[eng.MixTerm(utterance=5, snr=10.0, offset=100 * i)] for i in range(len(sel))]
    mixed = bp.mixedTensor(terms, utterances=sel, dtype=torch.float32)
    at16k = bp.resampledTensor(16000, signal=mixed, signalRate=22050, dtype=torch.float32)
    rows = rows_of(at16k[0], at16k[1], True)[0]
    for i, u in enumerate(sel):      # the rows are the host's chain too
        want = eng.signalResample(eng.pcmMix(pcm[u], pcm, terms[i]), 22050, 16000)
        assert rows[i].dtype == np.float32 and np.array_equal(bits(rows[i]), bits(want)), u
    lagMin, lagMax = eng.pitchLags(16000)
    kw = dict(nWin=512, hop=128, threshold=0.15, fields=("f0", "period", "aperiodicity", "voiced"))
    got, steps = bp.pitchTensor(signal=at16k, sampleRate=16000, dtype=torch.float64, **kw)
    any_voiced = False
    for i, g in enumerate(rows_of(got, steps, True)[0]):
        w = eng.signalPitch(rows[i], 16000, **kw)
        assert np.array_equal(bits(g), bits(w)), i
        any_voiced = any_voiced or bool((w[:, 3] == 1).any())
    assert any_voiced and (lagMin, lagMax) == (32, 267)


# ---- 3. the truth ---------------------------------------------------------------------------------------------------------------------------------
def test_steady_vowels_against_the_source_on_the_device():
    """Steady vowels a and u at six constant pitches and a silent utterance in one batch: every step whose frame lies 2000 samples inside a
    vowel is voiced and its period lies within half a sample of rate / f0, f0 being what sourceTensor states at the step's centre; the
    silent utterance is unvoiced throughout."""
    import torch
    import nvspeechplayer_amd as eng
    cases = [(v, p) for v in VOWELS for p in PITCHES]
    frames, mins, fades = zip(*[vowel_frames(v, p) for v, p in cases])
    n = len(cases)
    bp = eng.BatchPlayer(TRUTH_RATE)
    bp.setUtterances(np.arange(n + 2), np.stack(list(frames) + [np.zeros(47)]), list(mins) + [3000], list(fades) + [1], None, [0] * n + [1], np.arange(n + 1) + 1)
    bp.synthesize()
    truth, _ = bp.sourceTensor(["f0"], hop=256, dtype=torch.float64)
    truth = truth.cpu().numpy()[:, :, 0]
    worst = 0.0
    for W in (512, 1024):
        got, steps = bp.pitchTensor(nWin=W, lagMin=44, lagMax=368, hop=256, threshold=0.1, fields=("period", "voiced", "f0"), dtype=torch.float64)
        got, steps = got.cpu().numpy(), steps.numpy()
        for u, (vowel, pitch) in enumerate(cases):
            inside = inside_steps(bp.utteranceSamples(u), W, 368, 256)
            assert len(inside) >= 20 and np.all(np.abs(truth[u, inside] - pitch) <= 1e-9 * pitch), (vowel, pitch, truth[u, inside])
            err = np.abs(got[u, inside, 1] - TRUTH_RATE / truth[u, inside])
            worst = max(worst, float(err.max()))
            assert np.all(got[u, inside, 2] == 1) and np.all(err <= 0.5), (vowel, pitch, W, float(err.max()))
            assert np.array_equal(bits(got[u, :steps[u]]), bits(eng.pcmPitch(bp.read(u), TRUTH_RATE, nWin=W, lagMin=44, lagMax=368, hop=256, threshold=0.1,
                                                                               fields=("period", "voiced", "f0")))), (vowel, pitch, W)
        assert steps[n] > 10 and np.all(got[n, :steps[n], 2] == 0) and np.all(got[n, :steps[n], 0] == 0) and np.all(got[n, :steps[n], 1] == 44)
    print("pitch truth on the device: worst %.4f sample" % worst)
    bp.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_batch_usable():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    s = compared("plain")
    utt = np.arange(s.n, dtype=np.int64)
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    lens = [s.length(u) for u in range(s.n)]
    hop, W, lagMin, lagMax = 100, 200, 30, 120
    steps = [-(-n // hop) for n in lens]
    mostSteps, cols = max(steps), 2
    dev = "cuda:%d" % bp.device
    out = torch.full((s.n * mostSteps * cols + 8,), -7.0, dtype=torch.float64, device=dev)
    canary = out.clone()
    host = np.zeros(s.n * mostSteps * 8, np.float64)
    p = lambda a: None if a is None else a.ctypes.data

    def call(ptr=0, utterances=utt, n=None, W=W, lagMin=lagMin, lagMax=lagMax, threshold=0.2, hop=hop, phase=0, what=9, fmt=0, stride=mostSteps, batch=0):
        return L.speechPlayer_batch_exportPitch(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, W, lagMin, lagMax, threshold, hop, phase, what,
                                                out.data_ptr() if ptr == 0 else ptr, fmt, stride, None)

    def refused(name, fn, entry, words=b"", **kw):
        assert fn(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert entry in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert torch.equal(out, canary), name

    refused("not synthesised since it was set", call, b"exportPitch", b"not been synthesised")
    bp.synthesize()
    pcm = [bp.read(u).copy() for u in range(s.n)]
    cases = dict(no_batch=(dict(batch=None), b"no batch"), hop_0=(dict(hop=0), b"hop 0"), phase_negative=(dict(phase=-1), b"phase -1"), format_2=(dict(fmt=2), b"format 2"),
                 stride_negative=(dict(stride=-1), b"rowStride -1"), utterance_beyond=(dict(utterances=np.array([0, s.n], np.int64)), b"utterances[1]"), negative_count=(dict(n=-1), b""),
                 no_output=(dict(ptr=None), b"no output"), host_memory=(dict(ptr=host.ctypes.data), b""), too_small=(dict(stride=1 << 34), b""),
                 stride_short=(dict(stride=mostSteps - 1), b"below the largest step count"), misaligned=(dict(ptr=out.data_ptr() + 4), b"aligned"),
                 misaligned_float=(dict(ptr=out.data_ptr() + 2, fmt=1), b"aligned"),
                 nwin_31=(dict(W=31), b"nWin 31"), nwin_2049=(dict(W=2049), b"nWin 2049"), lagmin_1=(dict(lagMin=1), b"lagMin 1"), lags_equal=(dict(lagMin=120), b"lagMin 120, lagMax 120"),
                 lagmax_1025=(dict(lagMax=1025), b"lagMax 1025"), threshold_negative=(dict(threshold=-0.5), b"threshold"), threshold_above=(dict(threshold=1.5), b"threshold"),
                 threshold_nan=(dict(threshold=float("nan")), b"threshold"), what_0=(dict(what=0), b"what 0"), what_64=(dict(what=64), b"what 64"), what_negative=(dict(what=-1), b"what -1"))
    for name, (kw, words) in cases.items():
        refused(name, call, b"exportPitch", words, **kw)
    if torch.cuda.device_count() > 1:
        other = torch.zeros(s.n * mostSteps * cols, dtype=torch.float64, device="cuda:%d" % ((bp.device + 1) % torch.cuda.device_count()))
        refused("another device's memory", call, b"exportPitch", b"memory of device", ptr=other.data_ptr())
    # a signal's table, its rate, and the output on the signal
    x = torch.zeros((4, 1000), dtype=torch.int16, device=dev)
    extent = np.full(4, 1000, np.int64)

    def of(rec=None, rows=None, rate=16000, **fields):
        if rec is None:
            rec = record(sp, x.data_ptr(), 0, 4, 1000, extent)
            for key, v in fields.items():
                rec[key] = v
            rec = rec.ctypes.data
        return L.speechPlayer_batch_exportPitchOf(bp._h, rec, p(rows), 0 if rows is None else len(rows), rate, W, lagMin, lagMax, 0.2, hop, 0, 9, out.data_ptr(), 0, 10, None)

    bad_extent = np.array([1000, 1001, 0, 0], np.int64)
    for name, kw, words in (("no signal", dict(rec=0), b"no signal"), ("signal format", dict(format=2), b"signal format 2"), ("signal rows", dict(nRows=-1), b"nRows"),
                            ("no extent", dict(extent=0), b"extent"), ("extent beyond the stride", dict(extent=bad_extent.ctypes.data), b"extent[1]"),
                            ("no data", dict(data=0), b"without data"), ("host data", dict(data=host.ctypes.data), b""), ("row beyond", dict(rows=np.array([4], np.int64)), b"rows[0] = 4"),
                            ("the output is the signal", dict(data=out.data_ptr()), b"overlaps the signal"), ("rate 0", dict(rate=0), b"sampleRate 0"),
                            ("rate negative", dict(rate=-16000), b"sampleRate -16000")):
        refused(name, of, b"exportPitchOf", words, **kw)
    # nothing to write needs no buffer; and the batch is as usable as before
    assert call(ptr=None, utterances=utt[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert of() == 4 * 10 * 2
    torch.cuda.synchronize()
    silent = out[:80].cpu().numpy().reshape(40, 2)
    assert not bits(silent[:, 0]).any() and np.all(silent[:, 1] == 1.0)      # silence: F0 +0, every m 1.0
    out.copy_(canary)
    assert call() == s.n * mostSteps * cols
    torch.cuda.synchronize()
    got = out[:s.n * mostSteps * cols].view(s.n, mostSteps, cols).cpu().numpy()
    for u in range(s.n):
        w = eng.pcmPitch(pcm[u], s.sr, nWin=W, lagMin=lagMin, lagMax=lagMax, threshold=0.2, hop=hop, fields=("f0", "aperiodicity"))
        assert np.array_equal(bits(got[u, :len(w)]), bits(w)) and not bits(got[u, len(w):]).any(), u
    assert torch.equal(out[s.n * mostSteps * cols:], canary[s.n * mostSteps * cols:])
    # seventeen exports in flight: every slot, and one more
    outs = [bp.pitchTensor(nWin=64 + i, lagMin=20, lagMax=100 + i, hop=200, padded=False, dtype=torch.float64) for i in range(17)]
    torch.cuda.synchronize()
    for i, (o, offsets) in enumerate(outs):
        for u, g in enumerate(rows_of(o, offsets, False)[0]):
            assert np.array_equal(bits(g), bits(eng.pcmPitch(pcm[u], s.sr, nWin=64 + i, lagMin=20, lagMax=100 + i, hop=200))), (i, u)
    set_host(bp, s.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.pitchTensor()
    bp.close()


# ---- 5. past elements 2^31 and 2^32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
def test_far_outputs(padded):
    """exportPitch (W 32, lags 2 .. 23, hop 16, every field: 27 values a step, float32) past elements 2^31 and 2^32 with the periodic
    selection of tests/far_offsets.py: every later cycle is the first on the device, the first, the straddling and the last are the host's."""
    import torch
    import nvspeechplayer_amd as eng
    from tests.test_gpu_far_offsets import Export
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    lens = np.array([len(p) for p in pcm], np.int64)
    kw = dict(nWin=32, lagMin=2, lagMax=23, threshold=0.3, hop=16, fields=ALL)
    case = Export((27,), np.float32, -(-lens // 16), lambda sel, pad: bp.pitchTensor(utterances=sel, dtype=torch.float32, padded=pad, **kw),
                  [eng.pcmPitch(p, s.sr, **kw).astype(np.float32) for p in pcm])
    case.run(bp, padded, ("pitch32",))
    bp.close()
    torch.cuda.empty_cache()
