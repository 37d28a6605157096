"""The signal stems of a batch (include/speechPlayer_batch.h: speechPlayer_batch_exportStems; BatchPlayer.stemTensor;
csrc/klatt_stems.h) against `stems`, the sample-by-sample restatement of the header's definition in tests/test_stems_host.py (itself
held to the oracle's PCM there), against the oracle's PCM and against the engine's own MODE_EXACT PCM.  The glottal phase fed to the
restatement is the device's own sourceTensor("phase"), which tests/test_gpu_source.py holds to its definition: utterances with vibrato are
compared bit for bit as well.  The coefficients fed to it are speechPlayer_resonatorCoefficients': inside the range the header documents
they are the device's bits, and the test asserts that the compared utterances stay inside it.  No utterance is set aside.  Needs a GPU."""
import functools

import numpy as np
import pytest

from tests.test_gpu_source import batch_of, voiced
from tests.test_gpu_timeline import bits_equal, set_host, set_tensor
from tests.test_stems_host import (ASPIRATION, CASCADE, FRICATION, OUTPUT, PARALLEL, SOURCE, VOICE, Stemmed, compared, in_documented_range,
                                   native_coefficients, same, stems, to_pcm)

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
ALL = list(range(7))
GUARD = 64


def device_phase(bp):
    """The glottal phase of every utterance of the batch as set, float64, from the device."""
    import torch
    ph, off = bp.sourceTensor(["phase"], dtype=torch.float64, padded=False)
    ph, off = ph.cpu().numpy()[:, 0], off.numpy()
    return [ph[off[u]:off[u + 1]] for u in range(bp.nUtterances)]


def restated(bp, s):
    """The restatement of every utterance of s (a Stemmed) over the phase of the batch set on bp: [L, 7] per utterance."""
    phase = device_phase(bp)
    out = []
    for u in range(s.n):
        cur = s.cur(u)
        assert len(phase[u]) == len(cur), u
        out.append(stems(cur, phase[u], s.seed(u), s.sr, native_coefficients))
    return out


@functools.lru_cache(maxsize=None)
def wanted(name):
    """The restatement of a compared batch, computed once per process (the batch set on a player of its own for the phase)."""
    import nvspeechplayer_amd as eng
    s = compared(name)
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    want = restated(bp, s)
    bp.close()
    return want


def rows_of(flat, offsets, lens, ncol):
    """A packed export -> per row [ncol, L]."""
    flat, offsets = flat.cpu().numpy(), np.asarray(offsets)
    out = []
    for r, L in enumerate(lens):
        assert offsets[r + 1] - offsets[r] == ncol * L, r
        out.append(flat[offsets[r]:offsets[r + 1]].reshape(ncol, int(L)))
    return out


def check_rows(got, want, tag):
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (7, len(w)), (tag, u)
        for c in ALL:
            assert same(g[c], np.ascontiguousarray(w[:, c])), (tag, "utterance", u, "column", c)


@pytest.mark.parametrize("name", ["plain", "plain16k"])
def test_every_column_of_every_sample_against_the_restatement(name):
    """random_batch(default_rng(21), 10) at 22 050 and 16 000 Hz, all seven columns, float64, packed and padded.  All ten utterances keep
    their 28 frequencies and bandwidths finite and inside the documented range (a condition of this test), so the filter columns are
    compared bit for bit as well."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared(name)
    for u in range(s.n):
        assert in_documented_range(s.cur(u), s.sr), u
    want = wanted(name)
    lens = [s.length(u) for u in range(s.n)]
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    flat, offsets = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    assert int(offsets[-1]) == 7 * sum(lens) == 7 * bp.totalSamples
    check_rows(rows_of(flat, offsets.numpy(), lens, 7), want, "packed")
    padded, got_lens = bp.stemTensor(ALL, dtype=torch.float64, padded=True)
    assert tuple(padded.shape) == (s.n, 7, max(lens)) and list(got_lens.numpy()) == lens
    padded = padded.cpu().numpy()
    check_rows([padded[u, :, :lens[u]] for u in range(s.n)], want, "padded")
    for u in range(s.n):
        assert not padded[u, :, lens[u]:].view(np.uint64).any(), u      # padding: +0
    bp.close()


@pytest.mark.parametrize("name", ["plain", "wild"])
def test_output_truncates_to_the_oracles_pcm_and_to_the_engines(name):
    """Clipping and truncating float64 OUTPUT as the reference does gives the oracle's PCM and the engine's MODE_EXACT PCM on every
    sample (the wild batch: non-finite parameters, out-of-range resonators); the export changes no PCM, and neither synthesis nor
    MODE_FAST changes the export."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared(name)
    lens = [s.length(u) for u in range(s.n)]
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    before, offsets = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    got = rows_of(before, offsets.numpy(), lens, 7)
    for u in range(s.n):
        differ = np.flatnonzero(to_pcm(got[u][OUTPUT]) != s.pcm(u))
        assert len(differ) == 0, ("oracle", u, len(differ), int(differ[0]))
    bp.synthesize()
    digests = bp.digest(per_utterance=True)[1].copy()
    pcm, starts = bp.pcmTensor(dtype=torch.int16, padded=False)
    pcm, starts = pcm.cpu().numpy(), starts.numpy()
    for u in range(s.n):
        assert np.array_equal(to_pcm(got[u][OUTPUT]), pcm[starts[u]:starts[u + 1]]), ("engine", u)
    after, _ = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    assert bits_equal(after, before)
    assert np.array_equal(bp.digest(per_utterance=True)[1], digests)
    bp.close()
    fast = eng.BatchPlayer(s.sr, mode=1)
    set_host(fast, s.b)
    assert bits_equal(fast.stemTensor(ALL, dtype=torch.float64, padded=False)[0], before)
    fast.close()


def test_split_identities():
    """Every finite utterance of the plain batch three times in one batch with one seed: as is, with fricationAmplitude zeroed, with the
    three voice-source gains zeroed.  The cascade does not hear the frication, the parallel bank does not hear the voice, and a branch
    without input is exactly silent -- the noisy arithmetic runs for rows whose noise gains are all zero."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared("plain")
    keep = [u for u in range(s.n) if np.isfinite(s.cur(u)).all() and np.isfinite(utterance_frames(s.b, u)).all()]
    assert len(keep) >= 3
    frames, mins, fades, index, isnull, start, seeds = [], [], [], [], [], [0], []
    for variant in range(3):
        for u in keep:
            a, e = int(s.b["frame_start"][u]), int(s.b["frame_start"][u + 1])
            fr = np.array(s.b["frames"][a:e], dtype=np.float64)
            if variant == 1:
                fr[:, 24] = 0.0
            if variant == 2:
                fr[:, [3, 5, 6]] = 0.0
            frames.append(fr); mins.append(s.b["min"][a:e]); fades.append(s.b["fade"][a:e]); index.append(s.b["index"][a:e])
            isnull.append(s.b["isnull"][a:e]); start.append(start[-1] + e - a); seeds.append(s.b["seeds"][u])
    b = dict(frame_start=np.array(start, np.int64), frames=np.concatenate(frames), min=np.concatenate(mins), fade=np.concatenate(fades),
             index=np.concatenate(index), isnull=np.concatenate(isnull), seeds=np.array(seeds, np.uint32))
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, b)
    n = len(keep)
    lens = [s.length(u) for u in keep] * 3
    flat, offsets = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    got = rows_of(flat, offsets.numpy(), lens, 7)
    want = wanted("plain")
    for i, u in enumerate(keep):
        a, bb, c = got[i], got[n + i], got[2 * n + i]
        check_rows([a], [want[u]], "as is")
        assert same(a[CASCADE], bb[CASCADE]) and same(a[PARALLEL], c[PARALLEL]) and same(a[FRICATION], c[FRICATION]), u
        assert same(a[VOICE], bb[VOICE]) and same(a[SOURCE], bb[SOURCE]) and same(a[ASPIRATION], bb[ASPIRATION]), u
        assert not bb[PARALLEL].any() and not bb[FRICATION].any() and not c[CASCADE].any() and not c[SOURCE].any(), u
        assert a[PARALLEL].any() or not a[FRICATION].any(), u
    bp.close()


def utterance_frames(b, u):
    a, e = int(b["frame_start"][u]), int(b["frame_start"][u + 1])
    return np.asarray(b["frames"][a:e], dtype=np.float64)[~np.asarray(b["isnull"][a:e], dtype=bool)]


def noisy(pitch, end=None, depth=0.0, turbulence=0.3, aspiration=0.2, frication=0.4, bypass=0.1, shift=0.0):
    """A voiced frame with every noise gain, both filter branches and the nasal pair in use."""
    f = voiced(pitch, end, depth=depth, amp=0.8, gain=1.0)
    f[3], f[6], f[24], f[43], f[45], f[23] = turbulence, aspiration, frication, bypass, 1.5, 0.3
    f[7:13] = np.array([500.0, 1500.0, 2500.0, 3300.0, 3750.0, 4900.0]) + shift
    f[13], f[14] = 450.0 + shift, 250.0
    f[15:21] = [60.0, 90.0, 150.0, 200.0, 200.0, 1000.0]
    f[21], f[22] = 100.0, 100.0
    f[25:31] = np.array([520.0, 1480.0, 2600.0, 3400.0, 3800.0, 4950.0]) - shift
    f[31:37] = [70.0, 100.0, 160.0, 250.0, 250.0, 900.0]
    f[37:43] = [0.5, 0.4, 0.3, 0.3, 0.2, 0.6]
    return f


# the shortest utterance a request can make is 3 samples long (a fade lasts at least one sample: max(min, fade + 1) + 1); then the
# sizes either side of an 8- and a 16-sample tile, of the 16-sample blocks and of a wavefront's 64 lanes; and an utterance without frames
EDGE_LENGTHS = (3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 0)


@functools.lru_cache(maxsize=None)
def edge_case():
    """-> (the Stemmed batch of EDGE_LENGTHS, its restatement, the float64 packed export of every utterance as [7, L] arrays)."""
    import torch
    import nvspeechplayer_amd as eng
    # (no vibrato: a wavefront whose lanes are all steady, or all fading, for 16 samples runs the branch-free blocks -- a single row of
    # 63 samples or more does both; the random batches cover vibrato)
    a, b = noisy(140.0, 180.0), noisy(210.0, 95.0, frication=0.9, shift=35.0)
    utts = []
    for L in EDGE_LENGTHS:
        if L == 0:
            utts.append([])
        elif L < 10:
            utts.append([(a, L - 1, 1)])
        elif L < 63:
            utts.append([(a, 5, 3), (b, L - 7, 2)])
        else:
            utts.append([(a, 5, 3), (b, 20, 40), (None, 1, 1), (a, L - 52, 2)])
    s = Stemmed(batch_of(utts))
    assert tuple(s.length(u) for u in range(s.n)) == EDGE_LENGTHS
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    want = restated(bp, s)
    flat, offsets = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    base = rows_of(flat, offsets.numpy(), EDGE_LENGTHS, 7)
    bp.close()
    return s, want, base


def export(bp, rows, cols, fmt, padded, lens, offset=0):
    """speechPlayer_batch_exportStems through the C entry point into a buffer with GUARD elements either side, `offset` elements into
    a 16-byte aligned allocation: -> per row [len(cols), L]; asserts the element count, the zeros past each end and the guards."""
    import torch
    from nvspeechplayer_amd import _native
    L = _native.load()
    dtype, np_dtype = (torch.float32, np.float32) if fmt else (torch.float64, np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    row_lens = [int(lens[u]) for u in rows]
    stride = max(row_lens + [0]) if padded else 0
    elements = len(cols) * (len(rows) * stride if padded else sum(row_lens))
    buf = torch.full((elements + 2 * GUARD + offset,), -7.0, dtype=dtype, device="cuda:%d" % bp.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:]
    got = L.speechPlayer_batch_exportStems(bp._h, rows.ctypes.data, len(rows), cols.ctypes.data, len(cols),
                                           out.data_ptr() + GUARD * out.element_size(), fmt, stride, None)
    assert got == elements, (got, elements, L.speechPlayer_lastError())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:GUARD] == -7.0).all() and (host[GUARD + elements:] == -7.0).all() and len(host) == elements + 2 * GUARD
    body = host[GUARD:GUARD + elements]
    result, at = [], 0
    for n in row_lens:
        width = stride if padded else n
        block = body[at:at + len(cols) * width].reshape(len(cols), width)
        assert not block[:, n:].view(np.uint64 if np_dtype is np.float64 else np.uint32).any()      # exact zeros past the end
        result.append(block[:, :n])
        at += len(cols) * width
    assert at == elements
    return result


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 130])
def test_edges_of_the_tile_and_the_wavefront(n_rows):
    """Utterances of EDGE_LENGTHS, shuffled with repeats into 1, 63, 64, 65 and 130 rows; one column, a repeated column and all seven
    (8-sample tiles in float64); float64 and float32 (= the float64 value rounded to nearest); padded and packed; into a guarded buffer."""
    import nvspeechplayer_amd as eng
    s, want, base = edge_case()
    check_rows(base, want, "edge lengths")
    rng = np.random.default_rng(40 + n_rows)
    rows = rng.integers(0, s.n, n_rows)
    if n_rows == 1:
        rows[0] = EDGE_LENGTHS.index(129)                    # alone in its wavefront: steady and fade blocks
    if n_rows >= 63:
        rows[:len(EDGE_LENGTHS)] = rng.permutation(s.n)      # every length at least once
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    for cols in ([6], [2, 2, 0], ALL):
        for fmt in (0, 1):
            for padded in (True, False):
                got = export(bp, rows, cols, fmt, padded, EDGE_LENGTHS)
                for r, u in enumerate(rows):
                    w = base[u][cols]
                    assert same(got[r], w.astype(np.float32) if fmt else w), (cols, fmt, padded, r, int(u))
    bp.close()


@pytest.mark.parametrize("fmt", [0, 1])
def test_an_output_aligned_to_the_element_only(fmt):
    """The same rows into a buffer one element off a 16-byte boundary (element stores): the bits of the aligned export."""
    import nvspeechplayer_amd as eng
    s, want, base = edge_case()
    rows = np.random.default_rng(50).permutation(np.arange(130) % s.n)
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    for cols in ([6], [2, 2, 0], ALL):
        for padded in (True, False):
            aligned = export(bp, rows, cols, fmt, padded, EDGE_LENGTHS)
            shifted = export(bp, rows, cols, fmt, padded, EDGE_LENGTHS, offset=1)
            for r, u in enumerate(rows):
                assert same(shifted[r], aligned[r]) and same(aligned[r], base[u][cols].astype(np.float32) if fmt else base[u][cols]), (cols, padded, r)
    bp.close()


def read_back(bp, seeds, sr=22050):
    """The batch as it is resident on the device (speechPlayer_batch_frames), as a Stemmed."""
    read = [bp.frames(u) for u in range(bp.nUtterances)]
    fs = np.concatenate([[0], np.cumsum([len(r[1]) for r in read])]).astype(np.int64)
    return Stemmed(dict(frame_start=fs, frames=np.concatenate([r[0] for r in read]), min=np.concatenate([r[1] for r in read]),
                        fade=np.concatenate([r[2] for r in read]), index=np.concatenate([r[3] for r in read]),
                        isnull=np.concatenate([r[4] for r in read]), seeds=np.asarray(seeds, np.uint32)), sr)


def test_shared_lists_under_different_seeds():
    """Two lists, each spoken by two utterances with different seeds: without turbulence VOICE does not depend on the seed, with it
    it does, and every row is what the restatement says over the frames read back."""
    import torch
    import nvspeechplayer_amd as eng
    calm, rough = noisy(150.0, 120.0, turbulence=0.0), noisy(150.0, 120.0, turbulence=0.5)
    lists = batch_of([[(calm, 70, 9), (None, 5, 4)], [(rough, 70, 9), (None, 5, 4)]])
    list_of, seeds = np.array([0, 0, 1, 1], np.uint32), np.array([5, 6, 7, 8], np.uint32)
    bp = eng.BatchPlayer(22050)
    bp.setUtterancesShared(lists["frame_start"], lists["frames"], lists["min"], lists["fade"], list_of, lists["index"], lists["isnull"], seeds)
    s = read_back(bp, seeds)
    assert s.n == 4
    want = restated(bp, s)
    padded, lens = bp.stemTensor(ALL, dtype=torch.float64)
    got = [padded[u, :, :int(lens[u])].cpu().numpy() for u in range(4)]
    check_rows(got, want, "shared")
    assert same(got[0][VOICE], got[1][VOICE]) and not same(got[0][ASPIRATION], got[1][ASPIRATION])
    assert not same(got[2][VOICE], got[3][VOICE]) and same(want[0][:, VOICE], want[1][:, VOICE]) and not same(want[2][:, VOICE], want[3][:, VOICE])
    bp.close()


def test_a_batch_set_from_ipa_text():
    """Two short texts through setIpa (records expanded on the device), against the restatement over the frames read back."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    bp.setIpa(["hælou", "sɪti"], clauseType=".", voice="Benjamin", noiseSeed=[3, 4], trailing_silence_ms=10.0)
    s = read_back(bp, [3, 4])
    for u in range(s.n):
        assert in_documented_range(s.cur(u), s.sr), u
    want = restated(bp, s)
    lens = [s.length(u) for u in range(s.n)]
    flat, offsets = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    assert sum(lens) == bp.totalSamples and sum(lens) > 1000
    got = rows_of(flat, offsets.numpy(), lens, 7)
    check_rows(got, want, "ipa")
    assert any(g[FRICATION].any() for g in got) and all(g[VOICE].any() and g[OUTPUT].any() for g in got)
    bp.close()


def test_device_tensor_frames():
    """The plain batch through setUtterancesTensor: held to the restatement like the host set call's."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared("plain")
    lens = [s.length(u) for u in range(s.n)]
    bp = eng.BatchPlayer(s.sr)
    set_tensor(bp, s.b)
    flat, offsets = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    check_rows(rows_of(flat, offsets.numpy(), lens, 7), wanted("plain"), "tensor")
    bp.close()


def test_ordering_on_streams_and_against_set_calls():
    """An export on a side stream beside synthesize(wait=False); seventeen exports in flight; a set call right behind an export."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared("plain")
    lens = [s.length(u) for u in range(s.n)]
    want = wanted("plain")
    plain = eng.BatchPlayer(s.sr)
    set_host(plain, s.b)
    plain.synthesize()
    digests = plain.digest(per_utterance=True)[1].copy()
    plain.close()
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    side = torch.cuda.Stream(bp.device)
    with torch.cuda.stream(side):
        beside, offsets = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    bp.synthesize(wait=False)
    bp.wait()
    side.synchronize()
    check_rows(rows_of(beside, offsets.numpy(), lens, 7), want, "beside a launch")
    assert np.array_equal(bp.digest(per_utterance=True)[1], digests)
    flight = [bp.stemTensor([OUTPUT, SOURCE], dtype=torch.float64, padded=False)[0] for _ in range(17)]
    torch.cuda.synchronize()
    two = torch.cat([torch.from_numpy(np.concatenate([want[u][:, OUTPUT], want[u][:, SOURCE]])) for u in range(s.n)])
    for k, x in enumerate(flight):
        assert same(x.cpu().numpy(), two.numpy()), k
    # a set call right behind an export waits for it on the device
    last, offsets = bp.stemTensor(ALL, dtype=torch.float64, padded=False)
    set_host(bp, compared("wild").b)
    other, _ = bp.stemTensor([OUTPUT], dtype=torch.float64, padded=False)
    torch.cuda.synchronize()
    check_rows(rows_of(last, offsets.numpy(), lens, 7), want, "before a set call")
    assert other.numel() == bp.totalSamples == sum(compared("wild").length(u) for u in range(compared("wild").n))
    bp.close()


def test_refusals_write_nothing_and_leave_the_batch_usable():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("plain")
    lens = np.array([s.length(u) for u in range(s.n)])
    most = int(lens.max())
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    out = torch.full((s.n * most * 2 + 4,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel = out.clone()
    host = np.zeros(s.n * most * 2, np.float32)
    cols = np.array([SOURCE, OUTPUT], np.int32)
    utt = np.arange(s.n, dtype=np.int64)
    # "Too small" is measured against the device allocation, and torch carves its tensors out of larger ones: the end of
    # the allocation that holds `out` is where a packed export of 2 * sum(lens) elements falls one element short.
    seg = next(g for g in torch.cuda.memory_snapshot() if g["address"] <= out.data_ptr() < g["address"] + g["total_size"])
    one_short = seg["address"] + seg["total_size"] - 4 * (2 * int(lens.sum()) - 1)
    assert one_short >= seg["address"]

    def call(batch=bp._h, utterances=utt, n=s.n, columns=cols, ncol=2, ptr=out.data_ptr(), fmt=1, stride=most):
        return L.speechPlayer_batch_exportStems(batch, None if utterances is None else utterances.ctypes.data, n,
                                                None if columns is None else columns.ctypes.data, ncol, ptr, fmt, stride, None)

    refused = dict(
        no_batch=dict(batch=None), column_7=dict(columns=np.array([1, 7], np.int32)), column_negative=dict(columns=np.array([-1, 1], np.int32)),
        no_columns=dict(ncol=0), negative_columns=dict(ncol=-2), null_columns=dict(columns=None), format_2=dict(fmt=2), format_negative=dict(fmt=-1),
        utterance_beyond=dict(utterances=np.array([0, s.n], np.int64), n=2), utterance_negative=dict(utterances=np.array([-1], np.int64), n=1),
        negative_count=dict(n=-1), stride_short=dict(stride=most - 1), stride_negative=dict(stride=-1), host_memory=dict(ptr=host.ctypes.data),
        no_buffer=dict(ptr=None), misaligned=dict(ptr=out.data_ptr() + 2), too_small=dict(stride=1 << 34), too_small_packed=dict(stride=0, ptr=one_short),
        misaligned_f64=dict(ptr=out.data_ptr() + 4, fmt=0, utterances=utt[:1], n=1, stride=0, ncol=1))
    for name, kw in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportStems" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), name
    # nothing to write: 0, and no buffer needed
    assert call(utterances=utt[:0], n=0, ptr=None) == 0 and L.speechPlayer_lastErrorCode() == 0
    # the batch is as usable as before
    assert call() == s.n * most * 2
    torch.cuda.synchronize()
    want = wanted("plain")
    got = out[:s.n * most * 2].view(s.n, 2, most).cpu().numpy()
    for u in range(s.n):
        assert same(got[u, 0, :lens[u]], want[u][:, SOURCE].astype(np.float32)) and same(got[u, 1, :lens[u]], want[u][:, OUTPUT].astype(np.float32)), u
        assert not got[u, :, lens[u]:].any(), u
    assert torch.equal(out[s.n * most * 2:], sentinel[s.n * most * 2:])
    bp.synthesize()
    assert bp.totalSamples == int(lens.sum())
    bp.close()
