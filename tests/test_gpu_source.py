"""The glottal source of a batch (include/speechPlayer_batch.h: speechPlayer_batch_exportSource, _epochCounts, _exportEpochs;
BatchPlayer.sourceTensor / epochCounts / epochTensor; csrc/klatt_source.h) against `source`, the sample-by-sample restatement of the
header's definitions in tests/test_source_host.py.  An utterance without vibrato depth must equal it bit for bit (NaN standing for
NaN; the sign of a zero phase aside); elsewhere the device's sine and the host's may differ in the last bit, which the derived
tolerances below allow for, and CYCLE, OPEN, the epochs' samples and the counts are equal exactly -- tests/test_source_host.py asserts
that the compared batches hold no tie, and the batches built here are asserted tie-free before they are compared.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_gpu_timeline import bits_equal, set_host, set_tensor
from tests.test_source_host import (CYCLE, F0, OPEN, PHASE, VIBRATO_PHASE, WAVE, Sourced, compared, ties, vibrato_free)

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
ALL = list(range(6))
ULP = 2.0 ** -52


def same(got, want):
    """Equality of bits, NaN standing for NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]))


def close(got, want, tol, cyclic=False):
    """NaN where the restatement has NaN, equal where it is infinite, within tol elsewhere (cyclically: phases 0 and 1 are neighbours)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(want)
    if not np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]):
        return False
    d = np.abs(got[fin] - want[fin])
    if cyclic:
        d = np.minimum(d, np.abs(1.0 - d))
    return bool(np.all(d <= np.broadcast_to(tol, want.shape)[fin]))


def check_columns(got, cur, want, sr, tag):
    """All six columns of one utterance at hop 1."""
    L = len(cur)
    assert got.shape == (L, 6), tag
    if vibrato_free(cur):
        g, w = got.copy(), want.copy()
        g[:, [PHASE, VIBRATO_PHASE]] += 0.0; w[:, [PHASE, VIBRATO_PHASE]] += 0.0      # (-0 + 0 = +0: the sign of a zero phase is not compared)
        for c in ALL:
            assert same(g[:, c], w[:, c]), (tag, "column", c)
        return
    assert same(got[:, CYCLE], want[:, CYCLE]) and same(got[:, OPEN], want[:, OPEN]), tag
    assert close(got[:, PHASE], want[:, PHASE], L * ULP, cyclic=True), tag
    assert close(got[:, VIBRATO_PHASE], want[:, VIBRATO_PHASE], L * ULP, cyclic=True), tag
    assert close(got[:, F0], want[:, F0], 2.0 ** -51 * np.abs(want[:, F0])), tag
    with np.errstate(invalid="ignore"):
        assert close(got[:, WAVE], want[:, WAVE], 2 * L * ULP * np.abs(cur[:, 5])), tag


def check_epochs(got, cur, want, sr, tag):
    L = len(cur)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if vibrato_free(cur):
        assert same(got, want), tag
        return
    assert same(got[:, 0], want[:, 0]) and same(got[:, 3], want[:, 3]), tag
    assert close(got[:, 2], want[:, 2], 2.0 ** -51 * np.abs(want[:, 2])), tag
    with np.errstate(all="ignore"):
        tol = L * ULP / np.abs(want[:, 2] / sr) + 4 * np.spacing(np.maximum(want[:, 0], 1.0))
    assert close(got[:, 1], want[:, 1], tol), tag


def check_batch(bp, s, utterances=None):
    """Every column of every sample, every epoch row and the counts of the chosen utterances (None: all), packed float64.
    Returns (samples, epochs) compared."""
    import torch
    order = list(range(s.n)) if utterances is None else list(utterances)
    src, offsets = bp.sourceTensor(ALL, utterances=utterances, dtype=torch.float64, padded=False)
    counts = bp.epochCounts(utterances)
    ep, starts = bp.epochTensor(utterances, padded=False)
    src, offsets, ep, starts = src.cpu().numpy(), offsets.numpy(), ep.cpu().numpy(), starts.numpy()
    assert len(offsets) == len(starts) == len(order) + 1 and offsets[-1] == len(src) and starts[-1] == len(ep)
    assert counts.dtype == np.int64 and np.array_equal(np.diff(starts), counts)
    for r, u in enumerate(order):
        cur, cols, epochs, xs = s.get(u)
        assert offsets[r + 1] - offsets[r] == len(cur), u
        assert counts[r] == len(epochs), (u, counts[r], len(epochs))
        check_columns(src[offsets[r]:offsets[r + 1]], cur, cols, s.sr, ("utterance", u))
        check_epochs(ep[starts[r]:starts[r + 1]], cur, epochs, s.sr, ("utterance", u))
    return int(offsets[-1]), int(starts[-1])


def batch_of(requests_per_utterance):
    """[[(frame or None, min, fade), ...], ...] -> a batch as tests/scenarios.py builds them."""
    frames, mins, fades, nul, start = [], [], [], [], [0]
    for reqs in requests_per_utterance:
        for f, m, fd in reqs:
            frames.append(np.zeros(47) if f is None else f); mins.append(m); fades.append(fd); nul.append(f is None)
        start.append(len(mins))
    n = len(mins)
    return dict(frame_start=np.array(start, np.int64), frames=np.array(frames, np.float64).reshape(n, 47), min=np.array(mins, np.uint32),
                fade=np.array(fades, np.uint32), index=np.full(n, -1, np.int32), isnull=np.array(nul, np.uint8),
                seeds=np.arange(1, len(start), dtype=np.uint32))


def voiced(pitch, end=None, depth=0.0, speed=5.5, oq=0.4, amp=1.0, gain=1.0):
    f = np.zeros(47)
    f[0], f[46], f[1], f[2], f[4], f[5], f[44] = pitch, pitch if end is None else end, depth, speed, oq, amp, gain
    return f


def short_batch():
    utts = []
    for depth in (0.0, 0.7):
        a, b = voiced(2900.0, 3100.0, depth, speed=410.0), voiced(1731.0, 1650.0, depth, speed=97.0, oq=0.6, amp=0.5)
        for m in (3, 63, 64, 127, 128):
            utts.append([(a, m, 1)])
        utts.append([(a, 3, 1), (b, 57, 20), (None, 1, 1), (a, 2, 61), (b, 64, 64), (None, 70, 3)])
        utts.append([(b, 61, 40), (a, 0, 1), (a, 1, 2), (b, 190, 130)])
    return batch_of(utts)


def seventy_lists():
    rng = np.random.default_rng(23)
    utts = []
    for _ in range(70):
        reqs = []
        for _ in range(int(rng.integers(1, 5))):
            f = voiced(float(rng.uniform(60, 4000)), float(rng.uniform(60, 4000)), float(rng.choice([0.0, 0.0, rng.uniform(0, 2)])),
                       float(rng.uniform(0, 300)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 2)))
            reqs.append((None if rng.random() < 0.15 else f, int(rng.integers(0, 120)), int(rng.integers(0, 90))))
        utts.append(reqs)
    return batch_of(utts)


def assert_tie_free(s):
    for u in range(s.n):
        cur, cols, _, xs = s.get(u)
        assert ties(cur, cols, xs) == (0, 0), u


@pytest.mark.parametrize("name", ["plain", "wild"])
def test_random_batches_every_sample_and_every_epoch(name):
    """random_batch(default_rng(21), 24) and random_batch(default_rng(22), 24, wild=True): NaN holds, NULL frames anywhere, zero-length
    real frames with their infinite pitch, 18 and 20 utterances with vibrato, 3 with NaN phases."""
    import nvspeechplayer_amd as eng
    s = compared(name)
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    samples, epochs = check_batch(bp, s)
    assert (samples, epochs) == ((90428, 1215) if name == "plain" else (121150, 1240))
    assert samples == bp.totalSamples
    bp.close()


def test_named_scenarios():
    """hannah_vibrato (vibrato, breathiness, open quotient), nan_hold, duration_edges and the one-second vowel."""
    import nvspeechplayer_amd as eng
    s = compared("named")
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    samples, epochs = check_batch(bp, s)
    assert samples == bp.totalSamples and epochs > 100
    bp.close()


def test_short_utterances_and_pass_edges():
    """One request of 4 samples (min 3, fade 1), utterances of exactly 64 and 65 samples, of 128 and 129, and requests that begin and
    end on either side of a pass's last lane -- with a vibrato depth and without one."""
    import nvspeechplayer_amd as eng
    s = Sourced(short_batch())
    assert [s.length(u) for u in range(5)] == [4, 64, 65, 128, 129]
    assert_tie_free(s)
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    samples, epochs = check_batch(bp, s)
    assert epochs > 100
    bp.close()


def test_shared_lists_and_seventy_lists():
    """70 short lists (more wavefronts than one workgroup's worth of lanes), each spoken once; then two of them spoken by five
    utterances with different noise seeds: rows of one list are equal bit for bit, whatever the seed."""
    import torch
    import nvspeechplayer_amd as eng
    s = Sourced(seventy_lists())
    assert_tie_free(s)
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    check_batch(bp, s)
    b = s.b
    list_of = np.array([7, 31, 7, 7, 31], np.uint32)
    bp.setUtterancesShared(b["frame_start"], b["frames"], b["min"], b["fade"], list_of, b["index"], b["isnull"], np.array([5, 6, 7, 8, 9], np.uint32))
    assert bp.nUtterances == 5
    src, steps = bp.sourceTensor(ALL, dtype=torch.float64)
    ep, counts = bp.epochTensor()
    for r, l in enumerate(list_of):
        first = int(np.flatnonzero(list_of == l)[0])
        assert bits_equal(src[r], src[first]) and bits_equal(ep[r], ep[first]) and steps[r] == steps[first] == s.length(int(l)), r
        check_columns(src[r, :int(steps[r])].cpu().numpy(), *s.get(int(l))[:2], s.sr, ("row", r))
        check_epochs(ep[r, :int(counts[r])].cpu().numpy(), s.get(int(l))[0], s.get(int(l))[2], s.sr, ("row", r))
    assert not bits_equal(src[0], src[1])
    bp.close()


def test_a_batch_set_from_ipa_text():
    """Three texts through setIpa (records expanded on the device), against the restatement over the frames read back."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    bp = eng.BatchPlayer(22050)
    bp.setIpa(**workloads.cfg2_spec(3, first=500))
    read = [bp.frames(u) for u in range(bp.nUtterances)]
    fs = np.concatenate([[0], np.cumsum([len(r[1]) for r in read])]).astype(np.int64)
    s = Sourced(dict(frame_start=fs, frames=np.concatenate([r[0] for r in read]), min=np.concatenate([r[1] for r in read]),
                     fade=np.concatenate([r[2] for r in read]), index=np.concatenate([r[3] for r in read]),
                     isnull=np.concatenate([r[4] for r in read])))
    assert s.n == 3
    assert_tie_free(s)
    samples, epochs = check_batch(bp, s)
    assert samples == bp.totalSamples and epochs > 100
    bp.close()


def test_device_frames_and_another_sample_rate():
    """The first random batch through setUtterancesTensor: the bytes of the host set call.  The same batch at 16 000 Hz: held to the
    restatement at that rate."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared("plain")
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    want, steps = bp.sourceTensor(ALL, dtype=torch.float64, padded=False)
    want_ep, counts = bp.epochTensor(padded=False)
    set_tensor(bp, s.b)
    got, steps2 = bp.sourceTensor(ALL, dtype=torch.float64, padded=False)
    got_ep, counts2 = bp.epochTensor(padded=False)
    assert torch.equal(steps, steps2) and torch.equal(counts, counts2) and bits_equal(got, want) and bits_equal(got_ep, want_ep)
    bp.close()
    s16 = compared("plain16k")
    assert_tie_free(s16)
    bp = eng.BatchPlayer(16000)
    set_host(bp, s16.b)
    samples, epochs = check_batch(bp, s16)
    assert samples == 90428 and epochs != 1215 and not bits_equal(bp.sourceTensor("phase", dtype=torch.float64, padded=False)[0], want[:, 1:2])
    bp.close()


def test_hop_phase_rows_packing_and_dtype():
    """Steps, row selection, padding and float32 against the hop-1 float64 export that the tests above hold to the restatement."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared("wild")
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    lens = np.array([s.length(u) for u in range(s.n)])
    full, offsets = bp.sourceTensor(ALL, dtype=torch.float64, padded=False)
    offsets = offsets.numpy()
    cols = [5, 1, 0, 3, 3, 4, 2]
    chosen = list(range(s.n))[::-1] + [3, 3, 0]                      # out of order, with repeats
    for hop, phase in ((256, 0), (7, 3), (int(lens.max()) + 10, 0), (7, int(lens.min()) + 5), (64, 63), (1, 1)):
        steps_want = np.maximum(0, -(-(lens - phase) // hop))
        assert hop != 7 or phase == 3 or (steps_want == 0).any()     # (a phase beyond a short utterance: 0 steps)
        packed, poff = bp.sourceTensor(cols, hop=hop, phase=phase, utterances=chosen, dtype=torch.float64, padded=False)
        padded, steps = bp.sourceTensor(cols, hop=hop, phase=phase, utterances=chosen, dtype=torch.float64, padded=True)
        single, _ = bp.sourceTensor(cols, hop=hop, phase=phase, utterances=chosen, dtype=torch.float32, padded=True)
        assert list(steps.numpy()) == list(steps_want[chosen]) and list(np.diff(poff.numpy())) == list(steps_want[chosen])
        assert tuple(padded.shape) == (len(chosen), int(steps_want.max()), len(cols)) and single.dtype == torch.float32
        assert bits_equal(single, padded.to(torch.float32))           # rounded to nearest
        for r, u in enumerate(chosen):
            k = int(steps_want[u])
            want = full[offsets[u]:offsets[u + 1]][phase::hop][:, cols]
            assert len(want) == k and bits_equal(padded[r, :k], want) and bits_equal(packed[int(poff[r]):int(poff[r + 1])], want), (u, hop, phase)
            assert not bool(padded[r, k:].view(torch.int64).any()), (u, hop, phase)      # padding: +0
    # one column by name, every utterance, the default dtype
    one, steps = bp.sourceTensor("f0", hop=256)
    assert one.dtype == torch.float32 and tuple(one.shape) == (s.n, int(-(-lens.max() // 256)), 1)
    for u in (0, s.n - 1):
        assert bits_equal(one[u, :int(steps[u]), 0], full[offsets[u]:offsets[u + 1]][::256, 0].to(torch.float32))
    for padded in (True, False):
        none, steps = bp.sourceTensor(cols, utterances=[], padded=padded)
        assert none.numel() == 0 and len(steps) == (0 if padded else 1)
        none, counts = bp.epochTensor(utterances=[], padded=padded)
        assert none.numel() == 0 and len(counts) == (0 if padded else 1)
    # the epoch table: rows out of order and repeated, padded with the caller's value
    ep, starts = bp.epochTensor(padded=False)
    starts = starts.numpy()
    for pad in (-1.0, float("inf")):
        table, counts = bp.epochTensor(chosen, padded=True, pad=pad)
        assert tuple(table.shape) == (len(chosen), int(np.diff(starts).max()), 4) and np.array_equal(counts.numpy(), np.diff(starts)[chosen])
        for r, u in enumerate(chosen):
            k = int(counts[r])
            assert bits_equal(table[r, :k], ep[starts[u]:starts[u + 1]]) and bool((table[r, k:] == pad).all()), (r, u)
    assert np.array_equal(bp.epochCounts(chosen), np.diff(starts)[chosen])
    bp.close()


def test_the_step_table_in_pieces_and_synthesis_change_nothing():
    """"source_table_mb" = 1 (two lists to a piece for the longest utterances), exports before and after synthesize(), MODE_FAST and
    layout 0: the same bytes; and the PCM is what it is without an export."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared("wild")
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    want, _ = bp.sourceTensor(ALL, dtype=torch.float64, padded=False)
    want_ep, _ = bp.epochTensor(padded=False)
    want_hop, _ = bp.sourceTensor([1, 0], hop=7, phase=3, dtype=torch.float64, padded=True)
    bp.setOption("source_table_mb", 1)
    got, _ = bp.sourceTensor(ALL, dtype=torch.float64, padded=False)
    got_hop, _ = bp.sourceTensor([1, 0], hop=7, phase=3, dtype=torch.float64, padded=True)
    assert bits_equal(got, want) and bits_equal(got_hop, want_hop)
    bp.setOption("source_table_mb", 256)
    bp.synthesize()
    digests = bp.digest(per_utterance=True)[1].copy()
    got, _ = bp.sourceTensor(ALL, dtype=torch.float64, padded=False)
    got_ep, _ = bp.epochTensor(padded=False)
    assert bits_equal(got, want) and bits_equal(got_ep, want_ep)
    bp.synthesize(wait=False)
    between, _ = bp.sourceTensor(ALL, dtype=torch.float64, padded=False)
    bp.wait()
    assert bits_equal(between, want) and np.array_equal(bp.digest(per_utterance=True)[1], digests)
    bp.close()
    for kw in (dict(mode=1), dict(layout=0)):
        bp = eng.BatchPlayer(22050, **kw)
        set_host(bp, s.b)
        got, _ = bp.sourceTensor(ALL, dtype=torch.float64, padded=False)
        got_ep, _ = bp.epochTensor(padded=False)
        assert bits_equal(got, want) and bits_equal(got_ep, want_ep), kw
        bp.close()
    plain = eng.BatchPlayer(22050)
    set_host(plain, s.b)
    plain.synthesize()
    assert np.array_equal(plain.digest(per_utterance=True)[1], digests)
    plain.close()


def test_refusals_write_nothing_and_leave_the_batch_usable():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("wild")
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    lens = np.array([s.length(u) for u in range(s.n)])
    most = int(lens.max())
    out = torch.full((s.n * most * 2 + 4,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel = out.clone()
    host = np.zeros(s.n * most * 2, np.float32)
    cols = np.array([1, 3], np.int32)
    utt = np.arange(s.n, dtype=np.int64)

    def call(batch=bp._h, utterances=utt, n=s.n, columns=cols, ncol=2, hop=1, phase=0, ptr=out.data_ptr(), fmt=1, stride=most):
        return L.speechPlayer_batch_exportSource(batch, None if utterances is None else utterances.ctypes.data, n,
                                                 None if columns is None else columns.ctypes.data, ncol, hop, phase, ptr, fmt, stride, None)

    refused = dict(
        no_batch=dict(batch=None), column_6=dict(columns=np.array([1, 6], np.int32)), column_negative=dict(columns=np.array([-1, 1], np.int32)),
        no_columns=dict(ncol=0), negative_columns=dict(ncol=-2), null_columns=dict(columns=None), hop_0=dict(hop=0), hop_negative=dict(hop=-3),
        phase_negative=dict(phase=-1), format_2=dict(fmt=2), format_negative=dict(fmt=-1),
        utterance_beyond=dict(utterances=np.array([0, s.n], np.int64), n=2), utterance_negative=dict(utterances=np.array([-1], np.int64), n=1),
        stride_short=dict(stride=most - 1), stride_negative=dict(stride=-1), host_memory=dict(ptr=host.ctypes.data), no_buffer=dict(ptr=None),
        misaligned=dict(ptr=out.data_ptr() + 2), too_small=dict(stride=1 << 34), misaligned_f64=dict(ptr=out.data_ptr() + 4, fmt=0, utterances=utt[:2], n=2))
    for name, kw in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportSource" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), name
    # the epoch table
    counts = bp.epochCounts()
    widest = int(counts.max())
    table = torch.full((s.n * widest * 4 + 2,), -7.0, dtype=torch.float64, device="cuda:%d" % bp.device)
    keep = table.clone()

    def epochs(batch=bp._h, utterances=utt, n=s.n, ptr=table.data_ptr(), stride=widest, pad=-1.0, capacity=s.n * widest * 4):
        return L.speechPlayer_batch_exportEpochs(batch, None if utterances is None else utterances.ctypes.data, n, ptr, stride, pad, capacity, None)

    refused = dict(
        no_batch=dict(batch=None), utterance_beyond=dict(utterances=np.array([0, s.n], np.int64), n=2),
        utterance_negative=dict(utterances=np.array([-1], np.int64), n=1), stride_short=dict(stride=widest - 1), stride_negative=dict(stride=-2),
        capacity_short=dict(capacity=s.n * widest * 4 - 1), capacity_short_packed=dict(stride=0, capacity=int(counts.sum()) * 4 - 1),
        host_memory=dict(ptr=host.ctypes.data), no_buffer=dict(ptr=None), misaligned=dict(ptr=table.data_ptr() + 4),
        too_small=dict(stride=1 << 34, capacity=1 << 62))
    for name, kw in refused.items():
        assert epochs(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportEpochs" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(table, keep), name
    bad = np.array([s.n], np.int64)
    assert L.speechPlayer_batch_epochCounts(bp._h, bad.ctypes.data, 1, None) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT
    # the batch is as usable as before
    assert call() == s.n * most * 2 and epochs() == s.n * widest * 4
    torch.cuda.synchronize()
    want, offsets = bp.sourceTensor([1, 3], dtype=torch.float32, padded=False)
    want_ep, starts = bp.epochTensor(padded=False)
    got = out[:s.n * most * 2].view(s.n, most, 2)
    got_ep = table[:s.n * widest * 4].view(s.n, widest, 4)
    for u in range(s.n):
        assert bits_equal(got[u, :lens[u]], want[int(offsets[u]):int(offsets[u + 1])]), u
        assert bits_equal(got_ep[u, :counts[u]], want_ep[int(starts[u]):int(starts[u + 1])]) and bool((got_ep[u, counts[u]:] == -1.0).all()), u
    assert torch.equal(out[s.n * most * 2:], sentinel[s.n * most * 2:]) and torch.equal(table[s.n * widest * 4:], keep[s.n * widest * 4:])
    # an output aligned to 8 bytes and not to 16 (element stores): the same entries, nothing before or after them
    odd = torch.full((s.n * widest * 4 + 3,), -7.0, dtype=torch.float64, device="cuda:%d" % bp.device)
    assert epochs(ptr=odd.data_ptr() + 8) == s.n * widest * 4
    torch.cuda.synchronize()
    assert bits_equal(odd[1:-2], table[:s.n * widest * 4]) and float(odd[0]) == -7.0 and bool((odd[-2:] == -7.0).all())
    bp.synthesize()
    assert bp.totalSamples == int(lens.sum())
    bp.close()


def test_one_lane_per_list_gives_the_bits_of_one_wavefront_per_list():
    """Option "source_lane_lists" = 1 sends every walk through the lane-per-list kernel: columns, counts and epochs of the wild batch, of
    the short utterances and of the seventy lists are those of the wavefront-per-list kernel bit for bit, and hold to the restatement."""
    import torch
    import nvspeechplayer_amd as eng
    for s in (compared("wild"), Sourced(short_batch()), Sourced(seventy_lists())):
        got = []
        for lane_lists in (2 ** 31 - 1, 1):
            bp = eng.BatchPlayer(22050)
            bp.setOption("source_lane_lists", lane_lists)
            set_host(bp, s.b)
            if lane_lists == 1:
                check_batch(bp, s)
                bp.setOption("source_table_mb", 1)
            got.append([bp.sourceTensor(ALL, dtype=torch.float64, padded=False)[0], bp.sourceTensor(ALL[::-1], hop=7, phase=3, dtype=torch.float64)[0],
                        bp.sourceTensor(ALL, hop=256, dtype=torch.float64)[0], bp.epochTensor(padded=False)[0], torch.from_numpy(bp.epochCounts())])
            bp.close()
        for a, b in zip(*got):
            assert a.numel() > 0 and (bits_equal(a, b) if a.dtype == torch.float64 else torch.equal(a, b))


def test_the_threshold_between_the_two_walks():
    """12 288 short lists: the whole batch walks one lane per list (the default of option "source_lane_lists"), its first 12 287
    utterances one wavefront per list; the rows both exports hold are equal bit for bit, and a seeded choice of them holds to the restatement."""
    import torch
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(24)
    n = 12288
    utts = [[(voiced(float(rng.uniform(200, 9000)), float(rng.uniform(200, 9000)), float(rng.choice([0.0, 0.5])), float(rng.uniform(0, 900))),
              int(rng.integers(0, 40)), int(rng.integers(0, 30)))] for _ in range(n)]
    s = Sourced(batch_of(utts))
    bp = eng.BatchPlayer(22050)
    set_host(bp, s.b)
    lanes, steps = bp.sourceTensor(ALL, dtype=torch.float64, padded=True)
    waves, steps2 = bp.sourceTensor(ALL, utterances=np.arange(n - 1), dtype=torch.float64, padded=True)
    width = waves.shape[1]
    assert torch.equal(steps[:-1], steps2) and bits_equal(lanes[:-1, :width], waves) and int(steps.sum()) == bp.totalSamples
    ep_lanes, counts = bp.epochTensor()
    ep_waves, counts2 = bp.epochTensor(np.arange(n - 1))
    assert torch.equal(counts[:-1], counts2) and bits_equal(ep_lanes[:-1, :ep_waves.shape[1]], ep_waves) and int(counts.sum()) > n
    chosen = [int(u) for u in rng.choice(n, 24, replace=False)] + [n - 1]
    for u in chosen:
        cur, cols, _, xs = s.get(u)
        assert ties(cur, cols, xs) == (0, 0), u
    check_batch(bp, s, chosen)
    bp.close()
