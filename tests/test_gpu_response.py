"""The vocal-tract frequency response of a batch (include/speechPlayer_batch.h: speechPlayer_batch_exportResponse;
BatchPlayer.responseTensor; csrc/klatt_response.h) against the host's statement of the definition, speechPlayer_frameResponse applied
to the frames trackTensor returns for the same steps -- bit for bit for the real part, the imaginary part and the magnitude (the same
operations on the same operands in the same order, the same host-made twiddles), within 4 ulp for the dB kinds (the device's log10 and
the host's differ) -- and against the independent restatement of tests/test_response_host.py within its forward error bounds.
Needs a GPU."""
import numpy as np
import pytest

from tests import scenarios
from tests.test_gpu_source import batch_of
from tests.test_gpu_timeline import bits_equal, busy, same, set_host, set_tensor
from tests.test_response_host import LEFT_OUT_MOST, bounded_response, random_frames, within

pytestmark = pytest.mark.gpu
SR = 22050
ERR_ARGUMENT = 1
ALL = list(range(8))
PARAMS = list(range(47))
FIVE = np.array([0.0, 437.5, 1000.0, 2961.3, SR / 2.0])      # an odd number of bins: float32 blocks that are not 16-byte aligned


def ragged_batch():
    """40 seeded utterances of 1 .. 5 requests: NULL requests anywhere, fades of zero length (clamped to 1), of one sample and longer than
    their frame, zero-length frames; finite parameters inside klatt_math.h's validated range (|pi bw / sr| <= 700, |2 pi f / sr| <= 1e4),
    a few far outside what speech uses: no formant at all, bandwidths of 1e5 .. 1e6 Hz and a negative one, frequencies beyond Nyquist and
    up to 1e6 Hz (range reductions of exp and cos that ordinary formants never reach)."""
    rng = np.random.default_rng(41)
    pool = random_frames(rng, 60, floor=30.0)
    pool[3, 7:23] = 0.0; pool[3, 25:37] = 0.0                       # no resonator at all: every a == 0
    pool[5, 13] = 0.0; pool[5, 23] = 1.0                            # cfN0 == 0 with caNP == 1: the FIR form
    pool[7, 15:18] = [1.0e5, 3.0e5, 1.0e6]; pool[7, 31] = 2.5e5
    pool[9, 7:10] = [12000.0, 40000.0, 1.0e6]; pool[9, 25] = 7.0e5
    pool[11, 16] = -60.0; pool[11, 32] = -35.0                      # a pole outside the unit circle
    pool[13, 13] = 9000.0; pool[13, 14] = 15000.0
    utts = []
    for u in range(40):
        reqs = []
        for _ in range(int(rng.integers(1, 6))):
            f = None if rng.random() < 0.2 else pool[int(rng.integers(0, 14)) if rng.random() < 0.25 else int(rng.integers(0, 60))]
            mode = int(rng.integers(0, 5))
            if mode == 0: m, fd = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            elif mode == 1: m, fd = int(rng.integers(1, 60)), int(rng.integers(60, 300))
            else: m, fd = int(rng.integers(20, 500)), int(rng.choice([0, 1, 1, int(rng.integers(2, 200))]))
            reqs.append((f, max(m, 1) if f is not None else m, fd))
        utts.append(reqs)
    utts[0] = [(pool[3], 70, 1), (None, 10, 4), (pool[5], 90, 33)]
    utts[1] = [(pool[7], 50, 20), (pool[9], 64, 64), (pool[11], 40, 0), (pool[13], 30, 1)]
    utts[2] = [(pool[20], 1, 1)]                                    # 3 samples: shorter than a phase of 3
    return batch_of(utts)


def set_ipa(bp):
    """Two sampleIpa sentences, each in two voices, at three times the speed (utterances of a few thousand samples)."""
    from nvspeechplayer_amd import ipa, workloads
    spec = workloads.cfg2_spec(1)
    voices = [ipa.voiceIndex(ipa.voices()[1]), ipa.voiceIndex(ipa.voices()[3])]
    bp.setIpa([spec["texts"][0], spec["texts"][4]], speed=3.0, basePitch=[100.0, 130.0, 100.0, 130.0], clauseType=".", textOf=[0, 1, 0, 1],
              voice=[voices[0], voices[0], voices[1], voices[1]], noiseSeed=[1, 2, 3, 4])


SETTERS = {"ipa": set_ipa, "ragged": lambda bp: set_host(bp, ragged_batch())}


def frames_at(bp, hop=1, phase=0, utterances=None):
    """cur(t) at the steps: the 47 parameters, float64, packed.  -> (frames [steps, 47], offsets)."""
    import torch
    t, off = bp.trackTensor(PARAMS, hop=hop, phase=phase, utterances=utterances, dtype=torch.float64, padded=False)
    return t.cpu().numpy(), off.numpy()


def host_equal(got, frames, freqs, kinds, gain=False, sr=SR):
    """got [steps, nKinds, K] (float64) against speechPlayer_frameResponse of the frames: RE, IM and MAG bit for bit, DB within 4 ulp."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd.speechPlayer import check_response_request
    _, ks = check_response_request(freqs, kinds, sr)
    want = eng.frameResponse(frames, sr, freqs, kinds, gain=gain)
    got = np.asarray(got)
    if got.shape != want.shape:
        return False
    ok = True
    for q, kind in enumerate(ks):
        g, w = got[:, q], want[:, q]
        if kind & 3 != 3:
            ok = ok and same(g, w)
        else:
            fin = np.isfinite(w)
            with np.errstate(invalid="ignore"):
                ok = ok and np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[np.isinf(w)], w[np.isinf(w)]) \
                    and bool(np.all(np.abs(g[fin] - w[fin]) <= 4 * np.spacing(np.abs(w[fin]))))
    return bool(ok)


@pytest.fixture(scope="module", params=["ipa", "ragged"])
def compared(request):
    """A set batch, its frames at hop 1 and its response at five bins, all eight kinds, float64, packed -- with and without the gains."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(SR)
    SETTERS[request.param](bp)
    frames, offsets = frames_at(bp)
    got = {gain: bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False, gain=gain) for gain in (False, True)}
    for gain in got:
        assert np.array_equal(got[gain][1].numpy(), offsets) and tuple(got[gain][0].shape) == (len(frames), 8, 5)
    yield request.param, bp, frames, {gain: got[gain][0].cpu().numpy() for gain in got}
    bp.close()


def test_device_equals_the_host_bit_for_bit(compared):
    name, bp, frames, got = compared
    assert len(frames) == bp.totalSamples > 5000 and np.isfinite(frames[:, 1:46]).all()
    if name == "ragged":       # (the batch does hold what the test is about)
        assert (frames[:, 15:18] >= 1.0e5).any() and (frames[:, 7:10] >= 4.0e4).any() and (frames[:, 16] < 0).any()
        assert (~frames[:, 7:23].any(axis=1) & frames[:, 37:43].any(axis=1)).any()
    for gain in (False, True):
        assert host_equal(got[gain], frames, FIVE, ALL, gain), (name, gain)
    assert not np.array_equal(got[False], got[True])


def test_device_is_within_the_forward_error_bounds_of_the_restatement(compared):
    """tests/test_response_host.py's closed form and bound, on the distinct frames of the batch (a hold repeats its frame; voicePitch and
    endVoicePitch, which glide through it, do not enter the response)."""
    name, bp, frames, got = compared
    keyed = frames.copy()
    keyed[:, [0, 46]] = 0.0
    distinct, first = np.unique(keyed, axis=0, return_index=True)[:2]
    assert 100 < len(distinct) < len(frames)
    for gain in (False, True):
        miss = left_out = total = 0
        for i in range(0, len(first), 4096):
            pick = first[i:i + 4096]
            value, bound, rel = bounded_response(frames[pick], SR, FIVE, gain)
            m, l, t = within(got[gain][pick], value, bound, rel)
            miss, left_out, total = miss + m, left_out + l, total + t
        print("%s, gain %d: %d distinct frames, %d of %d elements left out, %d miss their bound" % (name, gain, len(first), left_out, total, miss))
        assert miss == 0 and left_out <= LEFT_OUT_MOST * total, (name, gain, miss, left_out, total)


@pytest.fixture(scope="module")
def ragged():
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(SR)
    b = ragged_batch()
    set_host(bp, b)
    lens = np.array([bp.utteranceSamples(u) for u in range(bp.nUtterances)], np.int64)
    yield bp, b, lens
    bp.close()


SHUFFLED = [6, 3, 0, 3, 7, 1, 5, 2, 2, 4, 7]
CHOSEN = list(range(40))[::-3] + [1, 1, 0, 2]      # out of order, with repeats, the 3-sample utterance among them


@pytest.mark.parametrize("K, hops", [(1, ((1, 0), (7, 3))), (3, ((1, 3), (256, 0))), (64, ((64, 0), (7, 3))), (65, ((64, 3), (256, 0))),
                                     (129, ((64, 0), (256, 3), (100000, 0)))])
def test_bins_kinds_hops_rows_packing_and_dtype(ragged, K, hops):
    """Every K with one kind, all eight and a shuffled list with repeats; padded and packed; float64 against the host, float32 = the
    float64 export rounded; a choice of rows with repeats; a phase beyond a short utterance."""
    import torch
    bp, b, lens = ragged
    freqs = np.linspace(0.0, SR / 2.0, K) if K > 1 else np.array([1234.5])
    for hop, phase in hops:
        steps_want = np.maximum(0, -(-(lens - phase) // hop))
        assert phase != 3 or (steps_want == 0).any()
        for kinds, chosen in ((ALL, None), (SHUFFLED, CHOSEN), (["parallel_db"], CHOSEN)):
            order = list(range(len(lens))) if chosen is None else chosen
            frames, offsets = frames_at(bp, hop, phase, chosen)
            packed, poff = bp.responseTensor(K if K > 1 else freqs, kinds, hop=hop, phase=phase, utterances=chosen, dtype=torch.float64, padded=False)
            padded, steps = bp.responseTensor(freqs, kinds, hop=hop, phase=phase, utterances=chosen, dtype=torch.float64, padded=True)
            single, _ = bp.responseTensor(freqs, kinds, hop=hop, phase=phase, utterances=chosen, padded=True)
            lone, _ = bp.responseTensor(freqs, kinds, hop=hop, phase=phase, utterances=chosen, dtype=torch.float32, padded=False)
            tag = (K, hop, phase, len(kinds))
            assert np.array_equal(poff.numpy(), offsets) and list(steps.numpy()) == list(steps_want[order]), tag
            assert tuple(packed.shape) == (len(frames), len(kinds), K) and tuple(padded.shape) == (len(order), int(steps_want[order].max()), len(kinds), K), tag
            assert host_equal(packed.cpu().numpy(), frames, freqs, kinds), tag
            assert single.dtype == torch.float32 and bits_equal(single, padded.to(torch.float32)) and bits_equal(lone, packed.to(torch.float32)), tag
            for r in range(len(order)):
                k = int(steps[r])
                assert bits_equal(padded[r, :k], packed[int(poff[r]):int(poff[r + 1])]), (tag, r)
                assert not bool(padded[r, k:].view(torch.int64).any()), (tag, r)      # padding: +0
    for pad in (True, False):
        none, steps = bp.responseTensor(freqs, ALL, utterances=[], padded=pad)
        assert none.numel() == 0 and len(steps) == (0 if pad else 1) and none.shape[-2:] == (8, K)


def test_the_default_arguments_and_an_output_that_is_not_16_byte_aligned(ragged):
    import torch
    from nvspeechplayer_amd import _native
    bp, b, lens = ragged
    L = _native.load()
    got, steps = bp.responseTensor(33, hop=128)
    want, _ = bp.responseTensor(np.linspace(0.0, SR / 2.0, 33), ["cascade_db", "parallel_db"], hop=128, phase=0, dtype=torch.float64)
    assert got.dtype == torch.float32 and tuple(got.shape) == (40, int(-(-lens.max() // 128)), 2, 33) and bits_equal(got, want.to(torch.float32))
    # element stores only: the same values, nothing before or after them
    n = want.numel()
    freqs, kinds = np.linspace(0.0, SR / 2.0, 33), np.array([3, 7], np.int32)
    for dtype, fmt, shift in ((torch.float64, 0, 1), (torch.float32, 1, 1), (torch.float32, 1, 3)):
        odd = torch.full((n + 8,), -7.0, dtype=dtype, device=want.device)
        got = L.speechPlayer_batch_exportResponse(bp._h, None, 40, freqs.ctypes.data, 33, kinds.ctypes.data, 2, 0, 128, 0,
                                                  odd.data_ptr() + shift * odd.element_size(), fmt, want.shape[1], None)
        assert got == n
        torch.cuda.synchronize()
        assert bits_equal(odd[shift:shift + n], want.to(dtype).reshape(-1)) and bool((odd[:shift] == -7.0).all()) and bool((odd[shift + n:] == -7.0).all())


def test_gain_is_the_product_with_the_two_track_columns(ragged):
    import torch
    bp, b, lens = ragged
    plain, off = bp.responseTensor(FIVE, [0, 1, 4, 5], hop=3, dtype=torch.float64, padded=False)
    gained, _ = bp.responseTensor(FIVE, [0, 1, 4, 5], hop=3, dtype=torch.float64, padded=False, gain=True)
    cols, _ = bp.trackTensor(["preFormantGain", "outputGain"], hop=3, dtype=torch.float64, padded=False)
    g = (cols[:, 0] * cols[:, 1])[:, None, None]
    assert bits_equal(gained + 0.0, plain * g + 0.0) and bool((g != 1).any())      # (+ 0.0: the sign of a zero is not compared)


def test_rows_that_share_a_list_are_bit_equal(ragged):
    import torch
    bp0, b, lens = ragged
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(SR)
    list_of = np.array([7, 31, 7, 7, 31, 1], np.uint32)
    bp.setUtterancesShared(b["frame_start"], b["frames"], b["min"], b["fade"], list_of, b["index"], b["isnull"], np.array([5, 6, 7, 8, 9, 10], np.uint32))
    got, steps = bp.responseTensor(FIVE, ALL, dtype=torch.float64)
    want, wsteps = bp0.responseTensor(FIVE, ALL, utterances=list_of.astype(np.int64), dtype=torch.float64)
    assert torch.equal(steps, wsteps) and bits_equal(got, want)
    assert bits_equal(got[0], got[2]) and bits_equal(got[0], got[3]) and bits_equal(got[1], got[4]) and not bits_equal(got[0, :50], got[1, :50])
    # 597 rows of one list (more than the 256 whose places a workgroup stages at a time), two of another, three of a third
    list_of = np.array([7] * 300 + [31, 1, 31] + [7] * 297 + [1, 1], np.uint32)
    bp.setUtterancesShared(b["frame_start"], b["frames"], b["min"], b["fade"], list_of, b["index"], b["isnull"], np.arange(len(list_of), dtype=np.uint32))
    for kw in (dict(padded=True), dict(padded=False)):
        got, steps = bp.responseTensor(3, SHUFFLED, hop=5, phase=1, dtype=torch.float64, **kw)
        for l in (7, 31, 1):
            want, wsteps = bp0.responseTensor(3, SHUFFLED, hop=5, phase=1, utterances=[l], dtype=torch.float64)
            k = int(wsteps[0])
            for r in np.flatnonzero(list_of == l):
                mine = got[r] if kw["padded"] else got[int(steps[r]):int(steps[r + 1])]
                assert bits_equal(mine[:k], want[0]) and (not kw["padded"] or not bool(mine[k:].view(torch.int64).any())), (kw, l, int(r))
                assert len(mine) == k or kw["padded"]
    bp.close()


def test_a_nan_parameter_scenario_exports_and_its_finite_steps_agree():
    """nan_hold of tests/scenarios.py (seven NaN parameters, among them cf2, cb2, pf2 and parallelBypass, which hold the values before)
    beside two other scenarios: no error, and every step whose frame is finite agrees with the host."""
    import torch
    import nvspeechplayer_amd as eng
    from tests.test_gpu_parity import make_batch
    sel = [s for s in scenarios.build_scenarios(scenarios.Ref()) if s.name in ("nan_hold", "duration_edges", "vowel_00_p0")]
    assert len(sel) == 3
    b = make_batch(sel)
    assert np.isnan(b["frames"]).any()
    bp = eng.BatchPlayer(SR)
    set_host(bp, b)
    frames, offsets = frames_at(bp, hop=2)
    got, off = bp.responseTensor(FIVE, ALL, hop=2, dtype=torch.float64, padded=False)
    single, _ = bp.responseTensor(FIVE, ALL, hop=2, padded=False)
    torch.cuda.synchronize()
    assert np.array_equal(off.numpy(), offsets) and bits_equal(single, got.to(torch.float32))
    finite = np.isfinite(frames[:, 1:46]).all(axis=1)
    assert 100 < finite.sum() and len(frames) == sum(-(-bp.utteranceSamples(u) // 2) for u in range(3))
    assert host_equal(got.cpu().numpy()[finite], frames[finite], FIVE, ALL)
    bp.synthesize()
    bp.close()


def test_synthesis_mode_and_layout_change_nothing():
    import torch
    import nvspeechplayer_amd as eng
    b = ragged_batch()
    bp = eng.BatchPlayer(SR)
    set_host(bp, b)
    want, _ = bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)
    want_hop, _ = bp.responseTensor(65, SHUFFLED, hop=64, phase=3)
    bp.synthesize()
    digests = bp.digest(per_utterance=True)[1].copy()
    got, _ = bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)
    assert bits_equal(got, want)
    bp.synthesize(wait=False)
    between, _ = bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)
    bp.wait()
    assert bits_equal(between, want) and np.array_equal(bp.digest(per_utterance=True)[1], digests)
    bp.close()
    for kw in (dict(mode=1), dict(layout=0)):
        other = eng.BatchPlayer(SR, **kw)
        set_tensor(other, b)
        got, _ = other.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)
        got_hop, _ = other.responseTensor(65, SHUFFLED, hop=64, phase=3)
        assert bits_equal(got, want) and bits_equal(got_hop, want_hop), kw
        other.close()
    plain = eng.BatchPlayer(SR)
    set_host(plain, b)
    plain.synthesize()
    assert np.array_equal(plain.digest(per_utterance=True)[1], digests)      # (and the PCM is what it is without an export)
    plain.close()


def test_ordering_against_streams_and_set_calls():
    """An export on a side stream behind a busy kernel, a set call with other frames straight after it, a second export: each holds its
    own batch's answer; seventeen exports in flight."""
    import torch
    import nvspeechplayer_amd as eng
    b = ragged_batch()
    other = dict(b)
    other["frames"] = b["frames"] * 0.75
    bp = eng.BatchPlayer(SR)
    set_host(bp, other)
    want_other, _ = bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)
    set_host(bp, b)
    want, _ = bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)
    torch.cuda.synchronize()
    assert not bits_equal(want, want_other)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        busy()
        first, _ = bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)
        set_tensor(bp, other)
        second, _ = bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)
        total = second.view(torch.int64).sum()       # consumed on the same stream, behind the export
    torch.cuda.synchronize()
    assert bits_equal(first, want) and bits_equal(second, want_other) and int(total) == int(want_other.view(torch.int64).sum())
    set_host(bp, b)
    with torch.cuda.stream(side):
        busy()
        many = [bp.responseTensor(FIVE, ALL, dtype=torch.float64, padded=False)[0] for _ in range(17)]
    torch.cuda.synchronize()
    for got in many:
        assert bits_equal(got, want)
    bp.close()


def test_refusals_write_nothing_and_leave_the_batch_usable(ragged):
    import torch
    from nvspeechplayer_amd import _native
    bp, b, lens = ragged
    L = _native.load()
    n, most = len(lens), int(lens.max())
    out = torch.full((n * most * 2 * 5 + 4,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel = out.clone()
    host = np.zeros(n * most * 2 * 5, np.float32)
    kinds = np.array([3, 7], np.int32)
    utt = np.arange(n, dtype=np.int64)

    def call(batch=bp._h, utterances=utt, nu=n, fq=FIVE, nf=5, ks=kinds, nk=2, gain=0, hop=1, phase=0, ptr=out.data_ptr(), fmt=1, stride=most):
        return L.speechPlayer_batch_exportResponse(batch, None if utterances is None else utterances.ctypes.data, nu, None if fq is None else fq.ctypes.data, nf,
                                                   None if ks is None else ks.ctypes.data, nk, gain, hop, phase, ptr, fmt, stride, None)

    refused = dict(
        no_batch=dict(batch=None), kind_8=dict(ks=np.array([3, 8], np.int32)), kind_negative=dict(ks=np.array([-1, 3], np.int32)), no_kinds=dict(nk=0),
        negative_kinds=dict(nk=-2), null_kinds=dict(ks=None), no_frequencies=dict(nf=0), too_many_frequencies=dict(fq=np.zeros(4097), nf=4097),
        null_frequencies=dict(fq=None), nan_frequency=dict(fq=np.array([0.0, 1.0, np.nan, 2.0, 3.0])), infinite_frequency=dict(fq=np.array([np.inf, 1.0, 2.0, 3.0, 4.0])),
        hop_0=dict(hop=0), hop_negative=dict(hop=-3), phase_negative=dict(phase=-1), format_2=dict(fmt=2), format_negative=dict(fmt=-1),
        utterance_beyond=dict(utterances=np.array([0, n], np.int64), nu=2), utterance_negative=dict(utterances=np.array([-1], np.int64), nu=1),
        stride_short=dict(stride=most - 1), stride_negative=dict(stride=-1), host_memory=dict(ptr=host.ctypes.data), no_buffer=dict(ptr=None),
        misaligned=dict(ptr=out.data_ptr() + 2), too_small=dict(stride=1 << 30), misaligned_f64=dict(ptr=out.data_ptr() + 4, fmt=0, utterances=utt[:2], nu=2))
    for name, kw in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportResponse" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), name
    # the Python checks, before any library call
    for bad, err in ((dict(frequencies=0), ValueError), (dict(frequencies=[float("inf")]), ValueError), (dict(kinds=[9]), ValueError), (dict(kinds="db"), KeyError),
                     (dict(hop=0), ValueError), (dict(phase=-1), ValueError), (dict(dtype=torch.float16), TypeError), (dict(utterances=[n]), ValueError)):
        kw = dict(frequencies=5)
        kw.update(bad)
        with pytest.raises(err):
            bp.responseTensor(**kw)
    # the batch is as usable as before
    assert call() == n * most * 2 * 5
    torch.cuda.synchronize()
    want, offsets = bp.responseTensor(FIVE, [3, 7], padded=False)
    got = out[:n * most * 10].view(n, most, 2, 5)
    for u in range(n):
        assert bits_equal(got[u, :lens[u]], want[int(offsets[u]):int(offsets[u + 1])]), u
    assert torch.equal(out[n * most * 10:], sentinel[n * most * 10:])
    bp.synthesize()
    assert bp.totalSamples == int(lens.sum())
