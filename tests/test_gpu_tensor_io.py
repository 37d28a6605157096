"""Batches in from torch tensors and PCM out as torch tensors (include/speechPlayer_batch.h: speechPlayer_batch_setUtterancesDevice,
speechPlayer_batch_exportPcm; BatchPlayer.setUtterancesTensor / pcmTensor).  A batch set from a device tensor must be the batch set
from host frames -- PCM, lengths, index marks, frames read back, plan --; the export must equal the host read paths; both must be ordered
against torch's streams by events alone; what is refused leaves the previous batch in place.  Needs a GPU."""
import numpy as np
import pytest

from tests import scenarios, whole_batch
from tests.test_gpu_parity import compare, make_batch, random_batch

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1


@pytest.fixture(scope="module")
def scenario_batch():
    sel = [s for s in scenarios.build_scenarios(scenarios.Ref()) if s.batchable and s.sr == 22050]
    batch = make_batch(sel)
    k = np.arange(len(batch["index"]))
    batch["index"] = np.where((batch["index"] == -1) & (k % 5 == 2), (k % 997).astype(np.int32), batch["index"]).astype(np.int32)
    return batch


def set_host(bp, b):
    bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])


def set_tensor(bp, b):
    import torch
    frames = torch.from_numpy(np.ascontiguousarray(b["frames"], dtype=np.float64)).to("cuda:%d" % bp.device)
    bp.setUtterancesTensor(b["frame_start"], frames, b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
    del frames      # (the engine copied it: the tensor may go at once)


def plan_of(info):
    keys = ("tracked_utterances", "tracks", "track_mbytes", "direct_utterances", "direct_mbytes", "lane_pipelined_utterances",
            "nasal_free_utterances", "wavefronts", "noisy_group")
    return {k: info[k] for k in keys}


def state_of(bp):
    """Everything a caller sees of a synthesised batch: PCM (bytes), starts, index marks, frames read back, plan."""
    bp.synthesize()
    pcm, starts = bp.readAll()
    marks = [bp.getLastIndex(u) for u in range(bp.nUtterances)]
    frames = [bp.frames(u) for u in range(bp.nUtterances)]
    return pcm.copy(), starts, marks, frames, plan_of(bp.kernelInfo())


def assert_same_state(a, b, name):
    assert np.array_equal(a[1], b[1]), name
    assert a[0].tobytes() == b[0].tobytes(), name
    assert a[2] == b[2], name
    for u, (x, y) in enumerate(zip(a[3], b[3])):
        for i in range(5):
            assert x[i].tobytes() == y[i].tobytes(), (name, u, i)
    assert a[4] == b[4], (name, a[4], b[4])


@pytest.mark.parametrize("mode", [0, 1])
def test_tensor_set_equals_host_set(scenario_batch, mode):
    """Every batchable scenario (vowels, the sampleIpa cases, vibrato, NaN holds, duration edges) and random ragged batches (NaN holds,
    NULL frames, zero-length real frames, vibrato): the batch set from a device tensor and from host frames give the same bytes of PCM,
    starts, index marks, frames read back and plan; in MODE_EXACT the scenario batch also against the oracle."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(7 + mode)
    batches = [("scenarios", scenario_batch), ("ragged", random_batch(rng, 600)), ("ragged wild", random_batch(rng, 600, wild=True))]
    bp = eng.BatchPlayer(22050, mode=mode)
    for name, b in batches:
        set_host(bp, b)
        want = state_of(bp)
        set_tensor(bp, b)
        got = state_of(bp)
        assert_same_state(want, got, "%s mode %d" % (name, mode))
        if mode == 0 and name == "scenarios":
            per = bp.digest(per_utterance=True)[1]
            n, differ = whole_batch.check_against_oracle(bp, b, per, compare, "tensor " + name, threads=8)
            assert n == len(b["frame_start"]) - 1
    bp.close()


def digests_of(bp):
    bp.synthesize()
    return bp.digest(per_utterance=True)[1]


def test_full_size_cfg2_from_a_tensor_gets_the_host_plan():
    """BASELINE configs[2] at full size: the plan (tracked, direct, nasal-free, quiet counts) and every utterance's digest are those of
    the batch set from host frames -- the planner, fed by one downloaded row per distinct shape, walked the same batch."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    b = workloads.make("cfg2", 65536)
    bp = eng.BatchPlayer(22050)
    set_host(bp, b)
    want, plan = digests_of(bp), plan_of(bp.kernelInfo())
    assert plan["tracked_utterances"] > 0
    set_tensor(bp, b)
    assert plan_of(bp.kernelInfo()) == plan
    assert np.array_equal(digests_of(bp), want)
    bp.close()


def test_all_different_subset_from_a_tensor():
    """A batch in which nothing is shared and nothing is aligned (workloads.all_different on a cfg2 slice): every frame is its own row
    of the shape table; the same direct-stage counts and digests as from host frames, in both modes."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    b = workloads.all_different(workloads.make("cfg2", 2048, first=512))
    for mode in (0, 1):
        bp = eng.BatchPlayer(22050, mode=mode)
        set_host(bp, b)
        want, plan = digests_of(bp), plan_of(bp.kernelInfo())
        set_tensor(bp, b)
        assert plan_of(bp.kernelInfo()) == plan, mode
        assert np.array_equal(digests_of(bp), want), mode
        bp.close()


def test_hash_collisions_of_tensor_frames_are_caught():
    """With the planner looking at 6 bits of a shape's hash, frames of different shapes share a row of the shape table: the device-side
    verification catches it, the batch runs without tracks and gives the PCM it always has."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads, _native
    b = workloads.make("cfg2", 1024, first=64)
    bp = eng.BatchPlayer(22050)
    set_tensor(bp, b)
    want = digests_of(bp)
    tracked = bp.kernelInfo()["tracked_utterances"]
    assert tracked >= 512 and _native.last_error_code() == 0
    L = _native.load()
    try:
        assert L.speechPlayer_setGlobalOption(b"plan_hash_bits", 6) == 0
        set_tensor(bp, b)
        assert "one 128-bit shape hash and different values" in _native.last_error() and _native.last_error_code() == 0
        assert bp.kernelInfo()["tracked_utterances"] == 0
        assert np.array_equal(digests_of(bp), want)
    finally:
        L.speechPlayer_setGlobalOption(b"plan_hash_bits", 128)
    set_tensor(bp, b)
    assert bp.kernelInfo()["tracked_utterances"] == tracked
    assert np.array_equal(digests_of(bp), want)
    bp.close()


def busy(stream_cycles=200_000_000):
    """Keep torch's current stream busy for a while (so that anything not ordered behind it would run first)."""
    import torch
    torch.cuda._sleep(stream_cycles)


def test_frames_from_a_side_stream_without_host_sync():
    """Frames computed by torch ops on a side stream (behind a long busy kernel) and handed over at once: the engine's copy waits for
    them on the device."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    b = workloads.make("cfg2", 512, first=1000)
    bp = eng.BatchPlayer(22050)
    set_host(bp, b)
    want = digests_of(bp)
    src = torch.from_numpy(b["frames"]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        busy()
        frames = torch.empty_like(src)
        frames.copy_(src * 2.0)
        frames.mul_(0.5)                      # exact: the frames hold no NaN, nothing near overflow
        bp.setUtterancesTensor(b["frame_start"], frames, b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
        frames.fill_(float("nan"))            # the engine copied the frames before this runs
    torch.cuda.synchronize()
    assert np.array_equal(digests_of(bp), want)
    bp.close()


def test_frames_from_the_default_stream_without_host_sync():
    """The same on torch's DEFAULT stream (the NULL stream, whose handle the C entry would read as "ready now"): frames written there
    behind a long busy kernel and handed over at once are copied only once they are written."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    b = workloads.make("cfg2", 512, first=1000)
    bp = eng.BatchPlayer(22050)
    set_host(bp, b)
    want = digests_of(bp)
    src = torch.from_numpy(b["frames"]).cuda()
    torch.cuda.synchronize()
    for rep in range(2):                      # (the second time through the player's own waiting stream again)
        busy()
        frames = torch.empty_like(src)
        frames.copy_(src * 2.0)
        frames.mul_(0.5)
        bp.setUtterancesTensor(b["frame_start"], frames, b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
        frames.fill_(float("nan"))
        assert np.array_equal(digests_of(bp), want), rep
    bp.close()


def test_exported_pcm_consumed_on_the_current_stream():
    """pcmTensor right behind an asynchronous synthesis, then a torch op on the current stream: no host wait anywhere until the
    result is read.  The pool holds another batch's PCM (same lengths, other noise seeds) when the synthesis is queued, so an export
    that did not wait for it would hand that out."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    b = workloads.make("cfg2", 256)
    other = workloads.Batch(b)
    other["seeds"] = b["seeds"] + np.uint32(777)
    bp = eng.BatchPlayer(22050)
    set_host(bp, b)
    bp.synthesize()
    want = [bp.readFloat(u) for u in range(bp.nUtterances)]
    set_host(bp, other)
    bp.synthesize()
    assert any(not np.array_equal(bp.readFloat(u), want[u]) for u in range(bp.nUtterances))
    set_host(bp, b)                           # the pool keeps `other`'s PCM until the synthesis below has run
    bp.synthesize(wait=False)
    pcm, lens = bp.pcmTensor()
    twice = (pcm * 2.0).cpu().numpy()
    assert pcm.device.index == bp.device and pcm.dtype == torch.float32
    for u in range(bp.nUtterances):
        n = int(lens[u])
        assert n == len(want[u])
        assert np.array_equal(twice[u, :n], want[u] * 2.0), u
        assert not twice[u, n:].any()
    bp.close()


@pytest.mark.parametrize("grow", [False, True])
def test_export_then_reuse_the_batch_at_once(grow):
    """Export, then immediately set and synthesize a different batch on the same player (its pool reused in place, or grown): the
    exported tensor still holds the first batch's PCM -- the export was delayed on its stream and the batch's next launch waited."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    first = workloads.make("cfg2", 512)
    if grow:
        second = workloads.make("cfg2", 2048, first=3)
    else:                                     # the same lengths, other noise: the pool is overwritten in place
        second = workloads.Batch(first)
        second["seeds"] = first["seeds"] + np.uint32(12345)
    bp = eng.BatchPlayer(22050)
    set_host(bp, first)
    bp.synthesize()
    want, starts = bp.readAll()
    want = want.copy()
    busy()
    pcm, offsets = bp.pcmTensor(dtype=torch.int16, padded=False)
    set_host(bp, second)
    bp.synthesize(wait=False)
    got = pcm.cpu().numpy()
    assert np.array_equal(offsets.numpy(), starts)
    assert np.array_equal(got, want)
    bp.synthesize()
    other, _ = bp.readAll()
    assert not np.array_equal(other[:len(want)], want[:len(other)])
    bp.close()


def test_export_against_the_host_read_paths():
    """padded int16 = read(u) zero-padded, float32 = readFloat(u), packed = readAll; unordered index lists with repeats, a row stride
    that is not a multiple of 8, an output that is not 16-byte aligned, zero-sample utterances, n = 0; a row stride below the longest
    chosen utterance is refused."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    rng = np.random.default_rng(3)
    b = random_batch(rng, 300)
    fs = b["frame_start"]
    # utterances 0, 17 and the last one of zero samples (no frames)
    for u in (0, 17, 299):
        cut = fs[u + 1] - fs[u]
        for key in ("frames", "min", "fade", "index", "isnull"):
            b[key] = np.delete(b[key], np.s_[fs[u]:fs[u + 1]], axis=0)
        fs = fs.copy(); fs[u + 1:] -= cut
    b["frame_start"] = fs
    bp = eng.BatchPlayer(22050)
    set_tensor(bp, b)
    bp.synthesize()
    n_utt = bp.nUtterances
    host16 = [bp.read(u) for u in range(n_utt)]
    hostf = [bp.readFloat(u) for u in range(n_utt)]
    assert len(host16[0]) == 0 and len(host16[17]) == 0 and len(host16[299]) == 0
    all16, starts = bp.readAll()
    # packed, everything
    p16, off = bp.pcmTensor(dtype=torch.int16, padded=False)
    assert np.array_equal(off.numpy(), starts) and np.array_equal(p16.cpu().numpy(), all16)
    sel = np.concatenate([rng.permutation(n_utt)[:120], [5, 5, 0, 17, 299, 5, 42]])
    for dtype, host in ((torch.int16, host16), (torch.float32, hostf)):
        pad, lens = bp.pcmTensor(sel, dtype=dtype)
        pad = pad.cpu().numpy()
        assert pad.shape == (len(sel), max(len(host[u]) for u in sel))
        for i, u in enumerate(sel):
            n = len(host[u])
            assert int(lens[i]) == n
            assert pad[i, :n].tobytes() == host[u].tobytes(), (dtype, i, u)
            assert not pad[i, n:].any()
        flat, off = bp.pcmTensor(sel, dtype=dtype, padded=False)
        assert flat.cpu().numpy().tobytes() == np.concatenate([host[u] for u in sel]).tobytes()
        assert np.array_equal(np.diff(off.numpy()), [len(host[u]) for u in sel])
    empty, lens = bp.pcmTensor([], dtype=torch.float32)
    assert empty.shape == (0, 0) and len(lens) == 0
    # the C entry itself: a row stride that is no multiple of 8 into an output 2 bytes off a 16-byte boundary, and a refusal
    L = _native.load()
    sel64 = np.ascontiguousarray(sel, np.int64)
    longest = max(len(host16[u]) for u in sel)
    stride = longest + 3
    for fmt, dtype, host in ((0, torch.int16, host16), (1, torch.float32, hostf)):
        buf = torch.full((len(sel) * stride + 16,), 7, dtype=dtype, device="cuda:%d" % bp.device)
        el = buf.element_size()
        got = L.speechPlayer_batch_exportPcm(bp._h, sel64.ctypes.data, len(sel), buf.data_ptr() + el, fmt, stride,
                                             torch.cuda.current_stream().cuda_stream)
        assert got == len(sel) * stride
        out = buf.cpu().numpy()
        assert out[0] == 7 and (out[1 + got:] == 7).all()       # nothing written outside the rows
        rows = out[1:1 + got].reshape(len(sel), stride)
        for i, u in enumerate(sel):
            n = len(host[u])
            assert rows[i, :n].tobytes() == host[u].tobytes() and not rows[i, n:].any(), (fmt, i)
        assert L.speechPlayer_batch_exportPcm(bp._h, sel64.ctypes.data, len(sel), buf.data_ptr(), fmt, longest - 1, None) == -1
        assert _native.last_error_code() == ERR_ARGUMENT and "rowStride" in _native.last_error()
    assert L.speechPlayer_batch_exportPcm(bp._h, sel64.ctypes.data, 0, None, 1, 0, None) == 0          # n = 0: nothing, no buffer
    bad = np.array([n_utt], np.int64)
    assert L.speechPlayer_batch_exportPcm(bp._h, bad.ctypes.data, 1, buf.data_ptr(), 1, 0, None) == -1
    assert _native.last_error_code() == ERR_ARGUMENT
    bp.close()


def test_refusals_leave_the_previous_batch():
    """Frames in page-locked or pageable host memory, frames that run past their allocation, a CPU or float32 tensor, a tensor on
    another device: refused with SPEECHPLAYER_ERR_ARGUMENT (or TypeError / ValueError before the library is called), the batch set
    before still there and readable."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, host_array, workloads
    b = workloads.make("cfg2", 64, first=8)
    bp = eng.BatchPlayer(22050)
    set_tensor(bp, b)
    bp.synthesize()
    want = [bp.read(u) for u in range(bp.nUtterances)]
    L = _native.load()
    fs = np.ascontiguousarray(b["frame_start"], np.int64)
    m = np.ascontiguousarray(b["min"], np.uint32)
    f = np.ascontiguousarray(b["fade"], np.uint32)
    pinned = host_array(b["frames"].shape, np.float64)
    pinned[...] = b["frames"]
    pageable = np.ascontiguousarray(b["frames"])
    short = torch.from_numpy(b["frames"][:4].copy()).cuda()
    huge = np.array([0, 1 << 40], np.int64)
    attempts = [(fs, pinned.ctypes.data), (fs, pageable.ctypes.data), (huge, short.data_ptr()), (fs, short.data_ptr() + 4)]
    for starts, ptr in attempts:
        rc = L.speechPlayer_batch_setUtterancesDevice(bp._h, len(starts) - 1, starts.ctypes.data, ptr, m.ctypes.data, f.ctypes.data,
                                                      None, None, None, None)
        assert rc == -1 and _native.last_error_code() == ERR_ARGUMENT, _native.last_error()
        assert "setUtterancesDevice" in _native.last_error()
    for bad, exc in ((torch.from_numpy(b["frames"]), TypeError), (torch.from_numpy(b["frames"]).float().cuda(), TypeError)):
        with pytest.raises(exc):
            bp.setUtterancesTensor(b["frame_start"], bad, b["min"], b["fade"])
    if torch.cuda.device_count() > 1:
        other = 1 if bp.device != 1 else 0
        elsewhere = torch.from_numpy(b["frames"]).to("cuda:%d" % other)
        with pytest.raises(ValueError):
            bp.setUtterancesTensor(b["frame_start"], elsewhere, b["min"], b["fade"])
        rc = L.speechPlayer_batch_setUtterancesDevice(bp._h, len(fs) - 1, fs.ctypes.data, elsewhere.data_ptr(), m.ctypes.data,
                                                      f.ctypes.data, None, None, None, None)
        assert rc == -1 and _native.last_error_code() == ERR_ARGUMENT
    assert bp.nUtterances == 64
    for u in range(64):
        assert np.array_equal(bp.read(u), want[u]), u
    bp.synthesize()
    pcm, lens = bp.pcmTensor(dtype=torch.int16)
    pcm = pcm.cpu().numpy()
    for u in range(64):
        assert np.array_equal(pcm[u, :int(lens[u])], want[u]), u
    bp.close()

