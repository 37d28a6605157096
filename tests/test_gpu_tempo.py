"""A batch's PCM and a signal's rows at another tempo by WSOLA (include/speechPlayer_batch.h: speechPlayer_batch_exportTempoPositions,
exportTempoPositionsOf, exportTempo, exportTempoOf; BatchPlayer.tempoPositionsTensor, tempoTensor; csrc/klatt_tempo.h) against the host's
statements of the definition -- speechPlayer_pcmTempo / signalTempo applied to what the engine read -- bit for bit, on integer views:
the positions of the search kernel and the samples of the render kernel.  The statements themselves are held to a transcription by
tests/test_tempo_host.py.  Needs a GPU."""
import numpy as np
import pytest

from tests.far_offsets import B31, B32, plan_cycles
from tests.test_gpu_signal import lay_out, poison, record
from tests.test_gpu_spectrogram import player, rows_of
from tests.test_gpu_timeline import set_host
from tests.test_lpc_host import float_row, golden_pcm
from tests.test_stems_host import compared
from tests.test_tempo_host import same

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
NULL, SHORT, SILENT = 10, 11, 12      # the utterances added to the ten of the plain batch
CYCLE = (0.25, 0.8, 1.0, 1.1, 4.0)


def the_batch():
    """The ten utterances of the plain batch (840 .. 5860 samples) and three more: one of no frames (length 0), one of 3 samples, and
    one with a null frame of 6000 samples (the resonators ring out, then exact zeros) between two voiced frames: the batch of
    tests/test_gpu_lpc.py."""
    b = dict(compared("plain").b)
    voiced = [k for k in range(len(b["frames"])) if not b["isnull"][k]][:3]
    n = len(b["min"])
    extra_min, extra_fade, extra_null = [0, 400, 6000, 600], [1, 100, 100, 100], [0, 0, 1, 0]
    b["frames"] = np.concatenate([b["frames"], b["frames"][[voiced[0], voiced[1], voiced[1], voiced[2]]]])
    b["min"] = np.concatenate([b["min"], np.array(extra_min, np.uint32)])
    b["fade"] = np.concatenate([b["fade"], np.array(extra_fade, np.uint32)])
    b["index"] = np.concatenate([b["index"], np.full(4, -1, np.int32)])
    b["isnull"] = np.concatenate([b["isnull"], np.array(extra_null, np.uint8)])
    b["frame_start"] = np.concatenate([b["frame_start"], [n, n + 1, n + 4]]).astype(np.int64)
    b["seeds"] = np.concatenate([b["seeds"], np.array([11, 12, 13], np.uint32)])
    return b


@pytest.fixture(scope="module")
def batch():
    bp, pcm = player(the_batch())
    assert len(pcm) == 13 and len(pcm[NULL]) == 0 and len(pcm[SHORT]) == 3 and len(pcm[SILENT]) > 7000
    quiet = np.flatnonzero(pcm[SILENT] == 0)
    assert len(quiet) > 3000 and pcm[SILENT][:300].any() and pcm[SILENT][-300:].any()      # a long silence inside
    yield bp, pcm
    bp.close()


@pytest.fixture(scope="module")
def bare():
    """A player that was never set: the exports of a signal need no batch content."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    yield bp
    bp.close()


def statement(row, *args, **kw):
    import nvspeechplayer_amd as eng
    return (eng.pcmTempo if row.dtype == np.int16 else eng.signalTempo)(row, *args, **kw)


def every_form():
    import torch
    return [(torch.float32, True), (torch.int16, False), (torch.float32, False), (torch.int16, True)]


def two_forms(k):
    forms = every_form()
    return [forms[k % 4], forms[(k + 1) % 4]]


_wanted = {}


def wanted(key, row, tempo, N, D):
    """The statement of a row, computed once per (row's key, tempo, N, D): (float32 samples, int16 samples, positions)."""
    key = (key, float(tempo), N, D)
    if key not in _wanted:
        y, p = statement(row, float(tempo), N, D, returnPositions=True)
        _wanted[key] = (y, statement(row, float(tempo), N, D, positions=p, dtype=np.int16), p)
    return _wanted[key]


def check_tempo(bp, rows, key, tempo, N, D, forms, tag, sel=None, signal=None):
    """tempoTensor with its own search in each of `forms` (dtype, padded) against the statement of every chosen row: lengths, frame
    counts, the positions' and the samples' bits, +0 and 0 padding."""
    import torch
    idx = list(range(len(rows))) if sel is None else list(sel)
    tempos = np.full(len(idx), tempo, np.float64) if np.ndim(tempo) == 0 else np.asarray(tempo, np.float64)
    want = [wanted((key, u), rows[u], t, N, D) for u, t in zip(idx, tempos)]
    lens, frames = [len(w[0]) for w in want], [len(w[2]) for w in want]
    for dtype, padded in forms:
        y, second, pos, counts = bp.tempoTensor(tempo, N, D, utterances=sel, dtype=dtype, padded=padded, signal=signal, returnPositions=True)
        ends = lambda c: list(c) if padded else list(np.concatenate([[0], np.cumsum(c)]))
        assert y.dtype == dtype and pos.dtype == torch.int64 and list(second.numpy()) == ends(lens) and list(counts.numpy()) == ends(frames), tag + (dtype, padded)
        assert tuple(y.shape) == ((len(idx), max(lens, default=0)) if padded else (sum(lens),)), tag
        assert tuple(pos.shape) == ((len(idx), max(frames, default=0)) if padded else (sum(frames),)), tag
        got, past = rows_of(pos, counts, padded)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w[2]), tag + ("positions", dtype, padded, i, idx[i], float(tempos[i]))
        for i, z in enumerate(past):
            assert not z.any(), tag + ("positions' padding", i)
        got, past = rows_of(y, second, padded)
        for i, (g, w) in enumerate(zip(got, want)):
            assert same(g, w[0] if dtype == torch.float32 else w[1]), tag + (dtype, padded, i, idx[i], float(tempos[i]))
        for i, z in enumerate(past):
            assert not z.view(np.uint8).any(), tag + ("padding", i)
    return want


# ---- 1. both kernels against the host statements ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 512, 2048])
def test_positions_and_samples_are_the_statements_bits(batch, N):
    """The thirteen utterances at a scalar tempo of 0.8 and at a tempo per row cycling 0.25, 0.8, 1, 1.1, 4; D 0, 31 and 160, and 1024 at
    N = 2048; the four output forms rotated over the combinations, two a combination."""
    bp, pcm = batch
    cycle = np.array([CYCLE[i % 5] for i in range(len(pcm))])
    k = 0
    for D in (0, 31, 160) + ((1024,) if N == 2048 else ()):
        for tempo in (0.8, cycle):
            want = check_tempo(bp, pcm, "pool", tempo, N, D, two_forms(k), (N, D, np.ndim(tempo)))
            k += 1
            if D == 160 and np.ndim(tempo) == 0:      # the search moved frames off their nominal places, and the silence kept them there
                p = want[SILENT][2]
                a = np.floor(np.arange(len(p)) * (N // 2) * 0.8).astype(np.int64)
                assert np.any(p != a) and (N > 512 or np.any(p[1:] == a[1:])), N


def test_a_selection_with_repeats_gives_one_utterance_two_tempos(batch):
    bp, pcm = batch
    sel = [SILENT, 2, 2, SHORT, NULL, 2, 0, SILENT]
    tempo = [0.8, 0.8, 1.25, 4.0, 1.0, 0.5, 1.1, 3.0]
    want = check_tempo(bp, pcm, "pool", tempo, 256, 40, every_form(), ("repeats",), sel=sel)
    assert len({len(want[i][0]) for i in (1, 2, 5)}) == 3
    pos, counts = bp.tempoPositionsTensor(1.1, 128, 10, utterances=[NULL, NULL])      # rows of nothing: nothing to launch
    assert tuple(pos.shape) == (2, 0) and list(counts.numpy()) == [0, 0]
    y, lengths = bp.tempoTensor(1.1, 128, 10, utterances=[NULL, NULL], padded=False)
    assert tuple(y.shape) == (0,) and list(lengths.numpy()) == [0, 0, 0]


# ---- 2. signal= -----------------------------------------------------------------------------------------------------------------------------
def test_the_signal_forms_on_a_player_never_set(bare):
    """Hand-made int16 and float32 signals with poison either side of every row (padded: in the rows' remainders; packed: before the first
    and behind the last), rows chosen out of order with a repeat: the statement's bits, and the signal unchanged afterwards."""
    import torch
    dev = "cuda:%d" % bare.device
    lens = [2000, 2049, 0, 3, 1500, 199, 4100]
    sel = [6, 1, 0, 4, 2, 3, 1, 5]
    tempo = [CYCLE[i % 5] for i in range(len(sel))]
    k = 0
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
            check_tempo(bare, rows, ("made", npt.__name__), tempo, 128, 31, two_forms(k), ("made", npt.__name__, stride), sel=sel, signal=signal)
            k += 1
            torch.cuda.synchronize()
            assert torch.equal(data, before), "the signal and its guards are as they were"


# ---- 3. the caller's positions ------------------------------------------------------------------------------------------------------------------
def test_the_callers_own_positions(batch):
    """A search's positions shifted by one, and positions of +-2^62 in two rows (masked by construction: the render reads nothing there):
    the host statement's bits, padded and packed positions, every output form."""
    import torch
    bp, pcm = batch
    dev = "cuda:%d" % bp.device
    sel = [2, SILENT, SHORT, 0, NULL, 7]
    N, D, tempo = 128, 20, 1.25
    own = [wanted(("pool", u), pcm[u], tempo, N, D)[2] + 1 for u in sel]
    own[1] = own[1].copy()
    own[1][::3] = 1 << 62
    own[3] = np.full(len(own[3]), -(1 << 62), np.int64)
    own[3][1::2] = (1 << 63) - 1
    frames = [len(p) for p in own]
    padded_pos = np.full((len(sel), max(frames) + 2), 77, np.int64)
    for i, p in enumerate(own):
        padded_pos[i, :len(p)] = p
    for positions in (torch.from_numpy(padded_pos).to(dev), torch.from_numpy(np.concatenate(own + [np.full(3, 77, np.int64)])).to(dev)):
        for dtype, padded in every_form():
            npt = np.float32 if dtype == torch.float32 else np.int16
            y, second, pos, counts = bp.tempoTensor(tempo, N, positions=positions, utterances=sel, dtype=dtype, padded=padded, returnPositions=True)
            assert pos is positions and list(counts.numpy()) == (frames if positions.dim() == 2 else list(np.concatenate([[0], np.cumsum(frames)])))
            got, past = rows_of(y, second, padded)
            for i, (g, u) in enumerate(zip(got, sel)):
                assert same(g, statement(pcm[u], tempo, N, D, positions=own[i], dtype=npt)), (positions.dim(), dtype, padded, i)
            for z in past:
                assert not z.view(np.uint8).any()
    assert not statement(pcm[0], tempo, N, D, positions=own[3]).any()      # every sample of that row was masked


# ---- 4. the pair is a signal ----------------------------------------------------------------------------------------------------------------------
def test_the_pair_feeds_the_resampler_and_the_spectrogram(batch):
    import torch
    import nvspeechplayer_amd as eng
    bp, pcm = batch
    sel = [2, SILENT, SHORT, NULL, 5]
    tempo = [0.8, 1.1, 4.0, 1.0, 1.25]
    for padded in (True, False):
        pair = bp.tempoTensor(tempo, 512, 160, utterances=sel, padded=padded)
        host = [wanted(("pool", u), pcm[u], t, 512, 160)[0] for u, t in zip(sel, tempo)]
        out, second = bp.resampledTensor(16000, signal=pair, padded=padded)
        for g, w in zip(rows_of(out, second, padded)[0], host):
            assert same(g, eng.signalResample(w, 22050, 16000)), padded
        out, second = bp.spectrogramTensor(nFft=256, hop=100, signal=pair, dtype=torch.float64, padded=padded)
        for g, w in zip(rows_of(out, second, padded)[0], host):
            assert same(g, eng.signalSpectrogram(w, nFft=256, hop=100)), padded


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_name_the_row():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    s = compared("plain")
    utt = np.arange(s.n, dtype=np.int64)
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    lens = np.array([s.length(u) for u in range(s.n)], np.int64)
    N, D = 128, 10
    tempo = np.full(s.n, 0.8)
    outLens = sp._tempo_lengths(lens, tempo)
    frames = sp._tempo_frames(outLens, N)
    most, mostK = int(outLens.max()), int(frames.max())
    dev = "cuda:%d" % bp.device
    pos = torch.full((s.n * most + 8,), -7, dtype=torch.int64, device=dev)      # (room for an output laid over it: the overlap case)
    out = torch.full((s.n * most + 8,), -7, dtype=torch.int16, device=dev)
    canary_pos, canary_out = pos.clone(), out.clone()
    host = np.zeros(s.n * most, np.int64)
    p = lambda a: None if a is None else a.ctypes.data

    def search(ptr=0, utterances=utt, n=None, tempo=tempo, nWin=N, search=D, stride=mostK, batch=0):
        return L.speechPlayer_batch_exportTempoPositions(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, p(tempo), nWin, search,
                                                         pos.data_ptr() if ptr == 0 else ptr, stride, None)

    def render(ptr=0, pptr=0, utterances=utt, n=None, tempo=tempo, nWin=N, pstride=mostK, fmt=0, stride=most, batch=0):
        return L.speechPlayer_batch_exportTempo(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, p(tempo), nWin,
                                                pos.data_ptr() if pptr == 0 else pptr, pstride, out.data_ptr() if ptr == 0 else ptr, fmt, stride, None)

    def refused(name, fn, entry, words=b"", **kw):
        assert fn(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert entry in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert torch.equal(pos, canary_pos) and torch.equal(out, canary_out), name

    refused("not synthesised since it was set", search, b"exportTempoPositions", b"not been synthesised")
    refused("not synthesised since it was set", render, b"exportTempo", b"not been synthesised")
    bp.synthesize()
    pcm = [bp.read(u).copy() for u in range(s.n)]
    nan3, slow0, fast9 = tempo.copy(), tempo.copy(), tempo.copy()
    nan3[3], slow0[0], fast9[9] = np.nan, 0.2, np.inf
    shared = dict(no_batch=(dict(batch=None), b"no batch"), nwin_odd=(dict(nWin=127), b"nWin 127"), nwin_62=(dict(nWin=62), b"nWin 62"), nwin_2050=(dict(nWin=2050), b"nWin 2050"),
                  no_tempo=(dict(tempo=None), b"no tempo"), tempo_nan=(dict(tempo=nan3), b"tempo[3] = nan: row 3"), tempo_slow=(dict(tempo=slow0), b"tempo[0] = 0.2: row 0"),
                  tempo_inf=(dict(tempo=fast9), b"tempo[9] = inf: row 9"), stride_negative=(dict(stride=-1), b"rowStride -1"),
                  utterance_beyond=(dict(utterances=np.array([0, s.n], np.int64), tempo=tempo[:2]), b"utterances[1]"), negative_count=(dict(n=-1), b""), no_output=(dict(ptr=None), b"no output"),
                  host_memory=(dict(ptr=host.ctypes.data), b""), too_small=(dict(stride=1 << 34), b""))
    cases = dict(shared, search_negative=(dict(search=-1), b"search -1"), search_1025=(dict(search=1025), b"search 1025"), stride_short=(dict(stride=mostK - 1), b"below the largest frame count"),
                 misaligned=(dict(ptr=pos.data_ptr() + 4), b"aligned"))
    for name, (kw, words) in cases.items():
        refused(name, search, b"exportTempoPositions", words, **kw)
    cases = dict(shared, format_2=(dict(fmt=2), b"format 2"), stride_short=(dict(stride=most - 1), b""), misaligned=(dict(ptr=out.data_ptr() + 1), b"aligned"),
                 pos_stride_short=(dict(pstride=mostK - 1), b"posStride %d is below the largest frame count" % (mostK - 1)), pos_stride_negative=(dict(pstride=-1), b"posStride -1"),
                 pos_host=(dict(pptr=host.ctypes.data), b"positions"), no_positions=(dict(pptr=None), b"no positions"), pos_misaligned=(dict(pptr=pos.data_ptr() + 4), b"aligned"),
                 pos_too_small=(dict(pstride=1 << 34), b"positions"), pos_stride_wraps=(dict(pstride=1 << 62, utterances=utt[:4], tempo=tempo[:4]), b"posStride 4611686018427387904"),
                 overlap=(dict(ptr=pos.data_ptr() + 64), b"overlaps the positions"))
    for name, (kw, words) in cases.items():
        refused(name, render, b"exportTempo", words, **kw)
    # a signal's table, and the outputs on the signal
    x = torch.zeros((4, 1000), dtype=torch.int16, device=dev)
    extent = np.full(4, 1000, np.int64)
    four = np.full(4, 1.0)

    def of(rec=None, rows=None, which="search", **fields):
        if rec is None:
            rec = record(sp, x.data_ptr(), 0, 4, 1000, extent)
            for key, v in fields.items():
                rec[key] = v
            rec = rec.ctypes.data
        if which == "search":
            return L.speechPlayer_batch_exportTempoPositionsOf(bp._h, rec, p(rows), 0 if rows is None else len(rows), four.ctypes.data, N, D, pos.data_ptr(), 20, None)
        return L.speechPlayer_batch_exportTempoOf(bp._h, rec, p(rows), 0 if rows is None else len(rows), four.ctypes.data, N, pos.data_ptr(), 20, out.data_ptr(), 0, 1000, None)

    for which, entry, mine in (("search", b"exportTempoPositionsOf", pos), ("render", b"exportTempoOf", out)):
        for name, kw, words in (("no signal", dict(rec=0), b"no signal"), ("signal format", dict(format=2), b"signal format 2"), ("no data", dict(data=0), b"without data"),
                                ("row beyond", dict(rows=np.array([4], np.int64)), b"rows[0] = 4"), ("the output is the signal", dict(data=mine.data_ptr()), b"overlaps the signal")):
            refused(name, of, entry, words, which=which, **kw)
    # nothing to write needs no buffer; and the batch is as usable as before
    assert search(ptr=None, utterances=utt[:0]) == 0 and render(ptr=None, pptr=None, utterances=utt[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert search() == s.n * mostK and render() == s.n * most
    torch.cuda.synchronize()
    got_pos, got = pos[:s.n * mostK].view(s.n, mostK).cpu().numpy(), out[:s.n * most].view(s.n, most).cpu().numpy()
    for u in range(s.n):
        y, q = eng.pcmTempo(pcm[u], 0.8, N, D, dtype=np.int16, returnPositions=True)
        assert np.array_equal(got_pos[u, :len(q)], q) and not got_pos[u, len(q):].any() and same(got[u, :len(y)], y) and not got[u, len(y):].any(), u
    assert torch.equal(pos[s.n * mostK:], canary_pos[s.n * mostK:]) and torch.equal(out[s.n * most:], canary_out[s.n * most:])
    # the binding names the row before any call
    with pytest.raises(ValueError, match="tempo of row 9"):
        bp.tempoTensor([0.8] * 9 + [9.0])
    with pytest.raises(ValueError, match="one per row"):
        bp.tempoPositionsTensor([0.8] * 9)
    with pytest.raises(ValueError, match="cuda"):
        bp.tempoTensor(0.8, N, positions=torch.zeros((s.n, mostK), dtype=torch.int64))
    with pytest.raises(TypeError, match="int64"):
        bp.tempoTensor(0.8, N, positions=torch.zeros((s.n, mostK), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="frames"):
        bp.tempoTensor(0.8, N, positions=torch.zeros((s.n, mostK - 1), dtype=torch.int64, device=dev))
    set_host(bp, s.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.tempoTensor(0.8)
    bp.close()


# ---- 6. past elements 2^31 and 2^32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
def test_far_outputs(padded):
    """exportTempo (int16, N = 64) with the periodic selection of tests/far_offsets.py and the caller's positions -- the host search's, laid
    out for one cycle and repeated on the device -- so that no search of that size runs: every later cycle is the first on the device, the
    first, the straddling and the last are the host's."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer as sp
    from tests.test_gpu_far_offsets import ORDER, Export
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    dev = "cuda:%d" % bp.device
    N, tempo = 64, 1.1
    lens = np.array([len(q) for q in pcm], np.int64)
    outLens = sp._tempo_lengths(lens, tempo)
    host = [eng.pcmTempo(q, tempo, N, 8, dtype=np.int16, returnPositions=True) for q in pcm]
    plan = plan_cycles(outLens, 1, (B31, B32), padded, ORDER)      # (the plan Export.run makes: the positions are those of its selection)
    if padded:
        one = np.zeros((len(plan.cycle), max(len(host[u][1]) for u in plan.cycle)), np.int64)
        for i, u in enumerate(plan.cycle):
            one[i, :len(host[u][1])] = host[u][1]
        positions = torch.from_numpy(one).to(dev).repeat(plan.repeats, 1)
    else:
        positions = torch.from_numpy(np.concatenate([host[u][1] for u in plan.cycle])).to(dev).repeat(plan.repeats)
    case = Export((), np.int16, outLens, lambda sel, pad: bp.tempoTensor(tempo, N, positions=positions, utterances=sel, dtype=torch.int16, padded=pad), [h[0] for h in host])
    got = case.run(bp, padded, ("tempo",))[0]
    assert got.cycle == plan.cycle and got.repeats == plan.repeats
    bp.close()
    torch.cuda.empty_cache()
