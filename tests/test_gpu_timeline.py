"""Per-sample parameter tracks and index-mark timelines of a batch (include/speechPlayer_batch.h: speechPlayer_batch_exportTracks,
speechPlayer_batch_timeline; BatchPlayer.trackTensor / timeline / marks; csrc/klatt_timeline.h) against `walk`, the sample-by-sample
restatement of the reference's frame manager in tests/test_timeline_host.py: float64 results for equality of bits (NaN standing for
NaN, the sign of zeros included), float32 results against walk.astype(float32); no utterance and no column is left out.  Needs a GPU."""
import numpy as np
import pytest

from tests import scenarios
from tests.test_gpu_parity import make_batch, random_batch
from tests.test_timeline_host import plan_timeline, utterance, walk

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
ALL = list(range(49))


def with_marks(batch):
    """Index marks as tests/test_gpu_tensor_io.py::scenario_batch adds them."""
    batch = dict(batch)
    k = np.arange(len(batch["index"]))
    batch["index"] = np.where((batch["index"] == -1) & (k % 5 == 2), (k % 997).astype(np.int32), batch["index"]).astype(np.int32)
    return batch


class Walked:
    """A batch and, per utterance, the walk's [L, 49] table (the 47 parameters, mark, frame), computed when first asked for."""

    def __init__(self, batch):
        self.b = batch
        self.n = len(batch["frame_start"]) - 1
        self._t = {}

    def table(self, u):
        if u not in self._t:
            cur, mark, number = walk(*utterance(self.b, u))
            self._t[u] = np.concatenate([cur, mark[:, None].astype(np.float64), number[:, None].astype(np.float64)], axis=1)
        return self._t[u]

    def length(self, u):
        return len(self.table(u))

    def expected(self, u, cols, hop=1, phase=0, dtype=np.float64):
        return np.ascontiguousarray(self.table(u)[phase::hop][:, cols]).astype(dtype)


@pytest.fixture(scope="module")
def scen():
    sel = [s for s in scenarios.build_scenarios(scenarios.Ref()) if s.batchable and s.sr == 22050]
    return Walked(with_marks(make_batch(sel)))


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(11)
    return Walked(with_marks(random_batch(rng, 150))), Walked(with_marks(random_batch(rng, 150, wild=True)))


@pytest.fixture(scope="module")
def small():
    """A wild batch small enough for many exports: NaN holds, NULL frames anywhere, zero-length real frames."""
    return Walked(with_marks(random_batch(np.random.default_rng(12), 40, wild=True)))


def set_host(bp, b):
    bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])


def set_tensor(bp, b):
    import torch
    frames = torch.from_numpy(np.ascontiguousarray(b["frames"], dtype=np.float64)).to("cuda:%d" % bp.device)
    bp.setUtterancesTensor(b["frame_start"], frames, b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])


def same(got, want):
    """Equality of bits, NaN standing for NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(bits)[~gn], want.view(bits)[~wn]))


def bits_equal(a, b):
    """Two device tensors hold the same bytes."""
    import torch
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def check_packed(bp, w, cols, hop=1, phase=0, dtype=None, pieces=200000, utterances=None):
    """Packed exports of `utterances` (None: all), in pieces small enough to download, against the walk.  Returns the samples compared."""
    import torch
    order = list(range(w.n)) if utterances is None else list(utterances)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    compared, i = 0, 0
    while i < len(order):
        j, load = i, 0
        while j < len(order) and (j == i or load + w.length(order[j]) <= pieces):
            load += w.length(order[j]); j += 1
        tracks, offsets = bp.trackTensor(cols, hop=hop, phase=phase, utterances=order[i:j], dtype=dtype, padded=False)
        got, offsets = tracks.cpu().numpy(), offsets.numpy()
        assert len(offsets) == j - i + 1 and offsets[-1] == len(got)
        for r, u in enumerate(order[i:j]):
            want = w.expected(u, cols, hop, phase, np_dtype)
            assert offsets[r + 1] - offsets[r] == len(want) == max(0, -(-(w.length(u) - phase) // hop)), (u, hop, phase)
            assert same(got[offsets[r]:offsets[r + 1]], want), "utterance %d hop %d phase %d" % (u, hop, phase)
            compared += len(want)
        i = j
    return compared


def test_all_columns_of_every_scenario_at_hop_1(scen):
    """The 190 batchable scenarios at 22 050 Hz as one batch: all 49 columns of every sample, float64, packed."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    set_host(bp, scen.b)
    assert scen.n == 190
    n = check_packed(bp, scen, ALL, dtype=torch.float64)
    assert n == sum(scen.length(u) for u in range(scen.n)) == bp.totalSamples
    # the voicePitch table in pieces (two lists at a time for the longest utterances): the same values
    bp.setOption("pitch_table_mb", 1)
    longest = sorted(range(scen.n), key=scen.length)[-5:]
    check_packed(bp, scen, [0, 46, 0, 48], dtype=torch.float64, utterances=longest + longest[:2])
    bp.close()


def test_all_columns_of_ragged_batches_at_hop_1(ragged):
    """Random ragged batches, plain and wild (NaN holds, NULL frames anywhere, zero-length real frames with their infinite pitch), with
    the voicePitch table whole and in pieces."""
    import torch
    import nvspeechplayer_amd as eng
    for w in ragged:
        bp = eng.BatchPlayer(22050)
        set_host(bp, w.b)
        check_packed(bp, w, ALL, dtype=torch.float64)
        whole, _ = bp.trackTensor(ALL, dtype=torch.float64, padded=False)
        bp.setOption("pitch_table_mb", 1)
        pieces, _ = bp.trackTensor(ALL, dtype=torch.float64, padded=False)
        assert bits_equal(whole, pieces)
        bp.close()
    wild = ragged[1]
    pitch = np.concatenate([wild.table(u)[:, 0] for u in range(wild.n)])
    assert np.isnan(pitch).any() or np.isinf(pitch).any()      # (the batch does hold what the test is about)
    assert any(np.isnan(wild.table(u)[:, 1:46]).any() for u in range(wild.n))


@pytest.mark.parametrize("hop", [1, 7, 64, 256, 100000])
def test_hop_phase_layout_and_dtype(small, hop):
    import torch
    import nvspeechplayer_amd as eng
    w = small
    bp = eng.BatchPlayer(22050)
    set_host(bp, w.b)
    lens = np.array([w.length(u) for u in range(w.n)])
    cols = ALL[::-1] + [7, 7, 0, 47]                      # in reverse order, with repeats
    chosen = list(range(w.n))[::-1] + [3, 3, 0]           # in reverse order, with repeats
    for phase in (0, 3, int(lens.min()) + 5):
        steps_want = np.maximum(0, -(-(lens - phase) // hop))
        for dtype, npd in ((torch.float64, np.float64), (torch.float32, np.float32)):
            check_packed(bp, w, cols, hop, phase, dtype, pieces=1 << 40, utterances=chosen)
            tracks, steps = bp.trackTensor(cols, hop=hop, phase=phase, utterances=chosen, dtype=dtype, padded=True)
            assert tracks.dtype == dtype and list(steps.numpy()) == list(steps_want[chosen])
            assert tuple(tracks.shape) == (len(chosen), int(steps_want.max()), len(cols))
            got = tracks.cpu().numpy()
            for r, u in enumerate(chosen):
                k = int(steps_want[u])
                assert same(got[r, :k], w.expected(u, cols, hop, phase, npd)), (u, hop, phase)
                assert not got[r, k:].view(np.uint64 if npd is np.float64 else np.uint32).any(), (u, hop, phase)      # padding: +0
        # all utterances in order, one column by name, the default dtype
        tracks, steps = bp.trackTensor("cf2", hop=hop, phase=phase)
        assert tracks.dtype == torch.float32 and list(steps.numpy()) == list(steps_want)
        got = tracks.cpu().numpy()
        for u in range(w.n):
            assert same(got[u, :int(steps_want[u])], w.expected(u, [8], hop, phase, np.float32)), (u, hop, phase)
    # no utterances: nothing to write
    for padded in (True, False):
        tracks, steps = bp.trackTensor(cols, hop=hop, utterances=[], padded=padded)
        assert tracks.numel() == 0 and len(steps) == (0 if padded else 1)
    bp.close()


def test_every_way_to_set_the_batch_gives_the_same_bytes(scen):
    """Host frames, a device tensor, shared lists (every list spoken by three utterances), MODE_FAST, layout 0: the same tracks."""
    import torch
    import nvspeechplayer_amd as eng
    b = scen.b
    bp = eng.BatchPlayer(22050)
    set_host(bp, b)
    want, steps = bp.trackTensor(ALL, hop=7, phase=2, dtype=torch.float64, padded=False)
    first = check_packed(bp, scen, ALL, hop=7, phase=2, dtype=torch.float64, utterances=range(0, scen.n, 19))
    assert first > 0
    set_tensor(bp, b)
    got, steps2 = bp.trackTensor(ALL, hop=7, phase=2, dtype=torch.float64, padded=False)
    assert torch.equal(steps, steps2) and bits_equal(got, want)
    nl = scen.n
    bp.setUtterancesShared(b["frame_start"], b["frames"], b["min"], b["fade"], np.tile(np.arange(nl), 3), b["index"], b["isnull"])
    got, steps3 = bp.trackTensor(ALL, hop=7, phase=2, dtype=torch.float64, padded=False)
    total = int(steps[-1])
    assert int(steps3[-1]) == 3 * total
    for rep in range(3):
        assert bits_equal(got[rep * total:(rep + 1) * total], want), rep
    bp.close()
    for kw in (dict(mode=1), dict(layout=0)):
        bp = eng.BatchPlayer(22050, **kw)
        set_host(bp, b)
        got, _ = bp.trackTensor(ALL, hop=7, phase=2, dtype=torch.float64, padded=False)
        assert bits_equal(got, want), kw
        bp.close()


def test_records_synthesis_and_marks(scen):
    """A setIpa batch (records expanded on the device) against the walk of the frames read back; exports before and after synthesize()
    give the same bytes; an export between synthesize(wait=False) and wait() leaves the PCM digests unchanged; track(MARK, L - 1) is
    getLastIndex after synthesis, for every utterance."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    bp = eng.BatchPlayer(22050)
    spec = workloads.cfg2_spec(24, first=500)
    bp.setIpa(**spec)
    read = [bp.frames(u) for u in range(bp.nUtterances)]
    fs = np.concatenate([[0], np.cumsum([len(r[1]) for r in read])]).astype(np.int64)
    w = Walked(dict(frame_start=fs, frames=np.concatenate([r[0] for r in read]), min=np.concatenate([r[1] for r in read]),
                    fade=np.concatenate([r[2] for r in read]), index=np.concatenate([r[3] for r in read]),
                    isnull=np.concatenate([r[4] for r in read])))
    check_packed(bp, w, ALL, hop=3, phase=1, dtype=torch.float64)
    bp.close()

    bp = eng.BatchPlayer(22050)
    set_host(bp, scen.b)
    before, _ = bp.trackTensor(ALL, hop=5, dtype=torch.float64, padded=False)
    bp.synthesize()
    digests = bp.digest(per_utterance=True)[1].copy()
    after, _ = bp.trackTensor(ALL, hop=5, dtype=torch.float64, padded=False)
    assert bits_equal(before, after)
    bp.synthesize(wait=False)
    between, _ = bp.trackTensor(ALL, hop=5, dtype=torch.float64, padded=False)
    bp.wait()
    assert bits_equal(before, between)
    assert np.array_equal(bp.digest(per_utterance=True)[1], digests)
    # the last sample's mark
    lens = np.array([scen.length(u) for u in range(scen.n)])
    last, offsets = bp.trackTensor("mark", dtype=torch.float64, padded=False)
    last = last.cpu().numpy()[:, 0]
    offsets = offsets.numpy()
    for u in range(scen.n):
        assert last[offsets[u + 1] - 1] == bp.getLastIndex(u) == scen.table(u)[-1, 47], u
    # timeline / marks against speechPlayer_planTimeline and the walk
    first, length = plan_timeline(scen.b["frame_start"], scen.b["min"], scen.b["fade"])
    assert np.array_equal(length, lens)
    for u in range(scen.n):
        a, e = int(scen.b["frame_start"][u]), int(scen.b["frame_start"][u + 1])
        t, ix = bp.timeline(u)
        assert t.dtype == np.int64 and ix.dtype == np.int32
        assert np.array_equal(t, np.concatenate([first[a:e], [lens[u]]])) and np.array_equal(ix, scen.b["index"][a:e]), u
        number = scen.table(u)[:, 48]
        assert np.array_equal(t[:-1], [int(np.flatnonzero(number == k)[0]) for k in range(e - a)]), u      # the sample a request is first in effect on
        sample, index = bp.marks(u)
        assert np.array_equal(sample, t[:-1][ix != -1]) and np.array_equal(index, ix[ix != -1]), u
        for s, i in zip(sample, index):
            assert scen.table(u)[s, 47] == i, (u, s)
    bp.close()


def test_cfg2_at_full_size():
    """BASELINE configs[2] from shared lists, 65 536 utterances, eight columns at hop 256 as float32, padded: on the device every
    utterance's rows are those of utterance u % 512; 16 of the first 512 rows (a seeded choice) against the walk."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    lists, list_of, seeds = workloads.shared("cfg2")
    bp = eng.BatchPlayer(22050)
    bp.setUtterancesShared(lists["frame_start"], lists["frames"], lists["min"], lists["fade"], list_of, lists["index"], lists["isnull"], seeds)
    assert bp.nUtterances == 65536
    names = ["voicePitch", "cf1", "cf2", "cf3", "voiceAmplitude", "fricationAmplitude", "mark", "frame"]
    cols = [0, 7, 8, 9, 5, 24, 47, 48]
    tracks, steps = bp.trackTensor(names, hop=256, dtype=torch.float32, padded=True)
    assert tuple(tracks.shape[::2]) == (65536, 8)
    blocks = tracks.view(128, 512, tracks.shape[1], 8).view(torch.int32)
    assert bool((blocks == blocks[:1]).all())
    assert torch.equal(steps.view(128, 512), steps[:512].expand(128, 512))
    head = tracks[:512].cpu().numpy()
    w = Walked(lists)
    for u in np.random.default_rng(3).choice(512, 16, replace=False):
        want = w.expected(int(u), cols, 256, 0, np.float32)
        assert int(steps[u]) == len(want)
        assert same(head[u, :len(want)], want), u
        assert not head[u, len(want):].any(), u
    bp.close()


def busy(stream_cycles=200_000_000):
    import torch
    torch.cuda._sleep(stream_cycles)


def test_ordering_against_streams_and_set_calls(small):
    import torch
    import nvspeechplayer_amd as eng
    w = small
    b = w.b
    bp = eng.BatchPlayer(22050)
    set_host(bp, b)
    want, _ = bp.trackTensor(ALL, dtype=torch.float64, padded=False)
    torch.cuda.synchronize()
    want = want.clone()
    # frames produced and tracks consumed on a side stream, nothing synchronised from the host
    src = torch.from_numpy(np.ascontiguousarray(b["frames"])).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        busy()
        frames = torch.empty_like(src)
        frames.copy_(src)
        bp.setUtterancesTensor(b["frame_start"], frames, b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
        frames.fill_(float("nan"))
        busy()
        got, _ = bp.trackTensor(ALL, dtype=torch.float64, padded=False)
        total = got.view(torch.int64).sum()       # consumed on the same stream, behind the export
    torch.cuda.synchronize()
    assert bits_equal(got, want) and int(total) == int(want.view(torch.int64).sum())
    # a set call straight after an export, with a batch of another size (pool and frame buffer grow)
    bigger = with_marks(random_batch(np.random.default_rng(13), 300))
    with torch.cuda.stream(side):
        busy()
        got, _ = bp.trackTensor(ALL, dtype=torch.float64, padded=False)
        set_host(bp, bigger)
    torch.cuda.synchronize()
    assert bits_equal(got, want)
    assert bp.nUtterances == 300
    # ... and of the same size (the buffers are reused: the set call waits on the device)
    other = dict(b)
    other["frames"] = b["frames"] * 0.5
    set_host(bp, b)
    with torch.cuda.stream(side):
        busy()
        got, _ = bp.trackTensor(ALL, dtype=torch.float64, padded=False)
        set_tensor(bp, other)
        halved, _ = bp.trackTensor(ALL[1:47], dtype=torch.float64, padded=False)
    torch.cuda.synchronize()
    assert bits_equal(got, want)
    assert not bits_equal(halved, want[:, 1:47])
    # seventeen exports in flight
    set_host(bp, b)
    with torch.cuda.stream(side):
        busy()
        many = [bp.trackTensor(ALL, dtype=torch.float64, padded=False)[0] for _ in range(17)]
    torch.cuda.synchronize()
    for got in many:
        assert bits_equal(got, want)
    bp.close()


def test_refusals_write_nothing_and_leave_the_batch_usable(small):
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    w = small
    bp = eng.BatchPlayer(22050)
    set_host(bp, w.b)
    lens = np.array([w.length(u) for u in range(w.n)])
    most = int(lens.max())
    out = torch.full((w.n * most * 2 + 4,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel = out.clone()
    host = np.zeros(w.n * most * 2, np.float32)
    cols = np.array([7, 47], np.int32)
    utt = np.arange(w.n, dtype=np.int64)

    def call(batch=bp._h, utterances=utt, n=w.n, columns=cols, ncol=2, hop=1, phase=0, ptr=out.data_ptr(), fmt=1, stride=most):
        return L.speechPlayer_batch_exportTracks(batch, None if utterances is None else utterances.ctypes.data, n,
                                                 None if columns is None else columns.ctypes.data, ncol, hop, phase, ptr, fmt, stride, None)

    refused = dict(
        no_batch=dict(batch=None), column_49=dict(columns=np.array([7, 49], np.int32)), column_negative=dict(columns=np.array([-1, 7], np.int32)),
        no_columns=dict(ncol=0), negative_columns=dict(ncol=-2), hop_0=dict(hop=0), hop_negative=dict(hop=-3), phase_negative=dict(phase=-1),
        format_2=dict(fmt=2), format_negative=dict(fmt=-1), utterance_beyond=dict(utterances=np.array([0, w.n], np.int64), n=2),
        utterance_negative=dict(utterances=np.array([-1], np.int64), n=1), stride_short=dict(stride=most - 1),
        host_memory=dict(ptr=host.ctypes.data), misaligned=dict(ptr=out.data_ptr() + 2), too_small=dict(stride=1 << 34),
        misaligned_f64=dict(ptr=out.data_ptr() + 4, fmt=0, utterances=utt[:2], n=2))
    for name, kw in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportTracks" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), name
    if torch.cuda.device_count() > 1:
        far = torch.zeros(w.n * most * 2, dtype=torch.float32, device="cuda:%d" % ((bp.device + 1) % torch.cuda.device_count()))
        assert call(ptr=far.data_ptr()) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT
    # the batch is as usable as before
    assert call() == w.n * most * 2
    torch.cuda.synchronize()
    got = out[:w.n * most * 2].view(w.n, most, 2).cpu().numpy()
    for u in range(w.n):
        assert same(got[u, :lens[u]], w.expected(u, [7, 47], 1, 0, np.float32)), u
    assert torch.equal(out[w.n * most * 2:], sentinel[w.n * most * 2:])
    bp.synthesize()
    assert bp.getLastIndex(0) == w.table(0)[-1, 47]
    bp.close()


def test_export_kinds_share_the_slot_ring_across_streams_and_a_set_call():
    """Every kind of export of the batch as set takes its staging slot from one ring of 16 (csrc/klatt_engine.hip: the export path), and
    each test file drives one kind.  Here 2 * 16 + 1 = 33 exports cycle through tracks (with column 0: the voicePitch table), alignment,
    units, source, epochs, response and stems on two streams that are never synchronised with the host, so the ring wraps twice with
    exports in flight; a set call with a longer batch follows at once (the per-request records grow), then the same 33.  After one final
    synchronise every tensor holds the bits the same call gives when made alone on a fresh BatchPlayer.  The batch: three utterances
    from IPA text, one of an empty text, two of one list."""
    import torch
    import nvspeechplayer_amd as eng
    kinds = [
        lambda bp: bp.trackTensor([0, 5, "mark"], hop=16, dtype=torch.float64, padded=False)[0],
        lambda bp: bp.alignmentTensor(["phoneme", "position"], hop=16)[0],
        lambda bp: bp.unitTensor(hop=16, padded=False)[0],
        lambda bp: bp.sourceTensor(["f0", "wave"], hop=16, phase=3400, padded=False)[0],
        lambda bp: bp.epochTensor(padded=False)[0],
        lambda bp: bp.responseTensor(8, hop=16, padded=False)[0],
        lambda bp: bp.stemTensor(["voice", "output"])[0],
    ]
    # utterances 0 and 2 speak one list; utterance 1 is the 150 ms of silence behind an empty text: 3307 samples, no epochs, and no
    # step at phase 3400 (a row without entries in the epoch table and in the source export)
    specs = [dict(texts=[text, ""], textOf=[0, 1, 0], speed=4, noiseSeed=[5, 6, 7]) for text in ("ha", "hælou wɜːld")]

    def bits(t):
        return t.contiguous().view({8: torch.int64, 4: torch.int32}[t.element_size()])

    want = []       # [batch][kind]: the call alone on a fresh player
    for spec in specs:
        row = []
        for kind in kinds:
            fresh = eng.BatchPlayer(22050)
            fresh.setIpa(**spec)
            row.append(kind(fresh))
            torch.cuda.synchronize()
            fresh.close()
        want.append(row)
    assert all(t.numel() > 0 for row in want for t in row)
    assert want[1][0].shape[0] > want[0][0].shape[0]       # (the second batch is the longer one)

    bp = eng.BatchPlayer(22050)
    dev = "cuda:%d" % bp.device
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    got = []
    for spec in specs:
        bp.setIpa(**spec)       # (the second: straight behind 33 exports in flight)
        row = []
        for k in range(33):
            with torch.cuda.stream(streams[k % 2]):
                if k < 2:
                    busy(20_000_000)       # the stream's exports queue up behind this
                row.append(kinds[k % len(kinds)](bp))
        got.append(row)
    torch.cuda.synchronize()
    for b, row in enumerate(got):
        for k, t in enumerate(row):
            w = want[b][k % len(kinds)]
            assert t.shape == w.shape and t.dtype == w.dtype and torch.equal(bits(t), bits(w)), "batch %d export %d" % (b, k)
    bp.close()
