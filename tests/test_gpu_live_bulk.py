"""Bulk queueing into live handles and a pull's PCM in caller-owned device tensors (include/speechPlayer_batch.h:
speechPlayer_queueFramesMany, speechPlayer_queueFramesManyDevice, speechPlayer_synthesizeManyExport; LiveGroup.queue / queueTensor /
pullTensor).  A bulk call must be the per-frame calls it stands for: handles fed one way and the other, with the same seeds, give
byte-equal PCM, equal call lengths and equal index marks after every pull, and each handle equals its own oracle player.  A refused call
changes no handle; the export equals the host pull and is ordered against torch's streams by events alone.  Needs a GPU."""
import ctypes

import numpy as np
import pytest

from tests import oracle, scenarios
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
NAN = float("nan")


@pytest.fixture(scope="module")
def ref():
    return scenarios.Ref()


def make_script(ref, n, seed):
    """What n handles are told, step by step: a step may close handles (a new one, with another seed, takes the freed slot over), queues
    rows into some handles (a row: frame | None, min, fade, index; `purge` on the handle's first row of the step) and ends with a pull.
    Handles speak ref.ipa_case streams (NULL frames, index marks); every fifth gets 700-1500 short frames (4-40 samples, some NULL, some
    of length 0), so that its ring (256 frames) overflows and pulls go in pieces; some are purged mid-stream, every third gets the rest of
    its sentence between uneven pulls."""
    rng = np.random.default_rng(seed)
    shapes = [scenarios.vowel_frame(ref, nm, 110.0 + 7 * k, 100.0 + 5 * k) for k, nm in enumerate(["a", "i", "u", "s", "z", "m", "n", "f"])]
    fz = scenarios.vowel_frame(ref, "z", 130.0, 90.0)

    def speech(base):
        case = ref.ipa_case(int(rng.integers(0, len(ref.ipa_meta))))
        return [(fr, m, f, base + j) for j, (fr, m, f) in enumerate(case)]

    def short(count, base):
        rows = []
        for j in range(count):
            r = rng.random()
            fr = None if r < 0.03 else shapes[int(rng.integers(0, len(shapes)))]
            rows.append((fr, 0 if r > 0.97 else int(rng.integers(4, 41)), int(rng.integers(0, 30)), base + j))
        return rows

    long_ = [k for k in range(n) if k % 5 == 3]
    first, later = {}, {}
    for k in range(n):
        rows = short(int(rng.integers(700, 1500)), 0) if k in long_ else speech(0)
        if k % 3 == 0 and k not in long_:
            first[k], later[k] = rows[:len(rows) // 2], rows[len(rows) // 2:]
        else:
            first[k] = rows
    purged = [k for k in range(n) if k % 7 == 1 or n == 1]
    replaced = list(range(5, n, 40))
    more = {k: (r, False) for k, r in later.items()}
    more.update({k: (short(300, 7000), False) for k in long_})
    return [{"queue": {k: (r, False) for k, r in first.items()}, "pull": 1},
            {"queue": {}, "pull": 777},
            {"queue": {k: ([(fz, 900, 300, 99)] + short(40, 5000), True) for k in purged}, "pull": 8192},
            {"queue": more, "pull": 3000},
            {"replace": [(k, 4242 + k) for k in replaced], "queue": {k: (speech(0), False) for k in replaced}, "pull": 8192},
            {"queue": {}, "pull": 4096}] + [{"queue": {}, "pull": 8192}] * 4


def pack(n, q):
    """A step's rows as a bulk call takes them: frameStart over all n handles (no rows for the others), frames [F, 47] (NaN in the NULL
    rows, which are never read), min, fade, index, isNull, purge."""
    rows, counts, purge = [], [], np.zeros(n, np.uint8)
    for k in range(n):
        r, p = q.get(k, ([], False))
        rows += r
        counts.append(len(r))
        purge[k] = 1 if p else 0
    fs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    frames = np.array([np.full(47, NAN) if fr is None else fr for fr, _, _, _ in rows], np.float64).reshape(-1, 47)
    return (fs, frames, np.array([r[1] for r in rows], np.uint32), np.array([r[2] for r in rows], np.uint32),
            np.array([r[3] for r in rows], np.int32), np.array([r[0] is None for r in rows], np.uint8), purge)


def queue_tensor(group, fs, frames, m, f, ix, nu, pg):
    """queueTensor with the frames written by a torch op on a side stream just before the call (behind a busy kernel) and overwritten
    with NaN right after it returns."""
    import torch
    dev = group.device
    src = torch.from_numpy(frames).to("cuda:%d" % dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        t = torch.empty_like(src)
        t.copy_(src)
        group.queueTensor(fs, t, m, f, ix, nu, pg)
        t.fill_(NAN)
    torch.cuda.synchronize(dev)


class Side:
    """One set of live handles fed one way: "frame" (a speechPlayer_queueFrame call per frame), "host" (LiveGroup.queue), "device"
    (LiveGroup.queueTensor)."""

    def __init__(self, how, seeds):
        import nvspeechplayer_amd as eng
        self.eng, self.how, self.n = eng, how, len(seeds)
        self.players = [eng.SpeechPlayer(22050, noiseSeed=s) for s in seeds]
        self.group = eng.LiveGroup(self.players)

    def step(self, st):
        for k, seed in st.get("replace", []):
            self.players[k].close()
            self.players[k] = self.eng.SpeechPlayer(22050, noiseSeed=seed)
            self.group = self.eng.LiveGroup(self.players)
        q = st["queue"]
        if not q:
            return
        if self.how == "frame":
            for k, (rows, purge) in q.items():
                for j, (fr, m, f, ix) in enumerate(rows):
                    self.players[k].queueFrameSamples(None if fr is None else self.eng.Frame.from_array(fr), m, f, ix, purge and j == 0)
        elif self.how == "host":
            self.group.queue(*pack(self.n, q))
        else:
            queue_tensor(self.group, *pack(self.n, q))

    def pull(self, count):
        out = np.zeros((self.n, count), np.int16)
        produced = self.group.pull(count, out).copy()
        return [out[k, :produced[k]].copy() for k in range(self.n)], [p.getLastIndex() for p in self.players]

    def close(self):
        for p in self.players:
            p.close()


class OracleSide:
    """One oracle player per handle, fed the same script."""

    def __init__(self, seeds):
        self.players = [oracle.OraclePlayer(22050, seed=s) for s in seeds]

    def step(self, st):
        for k, seed in st.get("replace", []):
            self.players[k].close()
            self.players[k] = oracle.OraclePlayer(22050, seed=seed)
        for k, (rows, purge) in st["queue"].items():
            for j, (fr, m, f, ix) in enumerate(rows):
                self.players[k].queue(fr, m, f, ix, purge and j == 0)

    def pull(self, count):
        return [o.synthesize(count) for o in self.players], [o.last_index() for o in self.players]

    def close(self):
        for o in self.players:
            o.close()


def same(want, got, what):
    """Byte-equal PCM, equal call lengths, equal index marks."""
    for k, (w, g) in enumerate(zip(want[0], got[0])):
        assert len(g) == len(w), (what, k, len(g), len(w))
        assert g.tobytes() == w.tobytes(), (what, k)
    assert got[1] == want[1], what


def play(ref, sides, orc, steps, L):
    """Every step on every side; after every pull, the sides equal the first one and (lengths, marks) the oracle.  -> (per handle the
    PCM of the second side over all pulls, the oracle's; launches of the pulls)"""
    n = sides[0].n
    got, exp, launches = [[] for _ in range(n)], [[] for _ in range(n)], []
    dev = sides[0].group.device
    for i, st in enumerate(steps):
        for s in sides + ([orc] if orc else []):
            s.step(st)
        want = sides[0].pull(st["pull"])
        for s in sides[1:]:
            g = s.pull(st["pull"])
            launches.append(L.speechPlayer_lastLiveLaunches(dev))
            same(want, g, "%s step %d" % (s.how, i))
        if orc:
            e = orc.pull(st["pull"])
            assert [len(x) for x in e[0]] == [len(x) for x in want[0]] and e[1] == want[1], i
            for k in range(n):
                got[k].append(g[0][k])
                exp[k].append(e[0][k])
    return got, exp, launches


@pytest.mark.parametrize("policy", ["alone", "shared", "single"])
def test_host_bulk_equals_per_frame(ref, policy):
    """130 handles (one for "single": the replicate path of a handle pulled alone) fed per frame and through LiveGroup.queue, with NULL
    frames, zero-length frames, index marks, rings that overflow, purges mid-stream, frames queued between uneven pulls and a closed
    handle's slot reused; "live_alone" 1536 ("alone", "single") and 1 ("shared").  The bulk set also against one oracle player each."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    n = 1 if policy == "single" else 130
    seeds = [500 + k for k in range(n)]
    sides, orc = [Side("frame", seeds), Side("host", seeds)], OracleSide(seeds)
    try:
        assert L.speechPlayer_setGlobalOption(b"live_alone", 1 if policy == "shared" else 1536) == 0
        got, exp, launches = play(ref, sides, orc, make_script(ref, n, 11), L)
    finally:
        L.speechPlayer_setGlobalOption(b"live_alone", 1536)
        for s in sides + [orc]:
            s.close()
    for k in range(n):
        compare(np.concatenate(got[k]), np.concatenate(exp[k]), "bulk live stream %d" % k)
    if n > 1:
        assert max(launches) > 1, launches          # some pull went in pieces


@pytest.mark.parametrize("mode", [0, 1])
def test_device_bulk_equals_host_bulk(ref, mode):
    """The same script through LiveGroup.queueTensor (frames written on a side stream right before the call, NaN right after it; NaN in
    the NULL rows) and through LiveGroup.queue, handles created under "live_mode" 0 and 1; frames beyond the rings reach the host by the
    download.  In mode 0 the device set against the oracle too."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    n = 130
    seeds = [900 + k for k in range(n)]
    assert L.speechPlayer_setGlobalOption(b"live_mode", mode) == 0
    sides, orc = [], None
    try:
        sides = [Side("host", seeds), Side("device", seeds)]
        orc = OracleSide(seeds) if mode == 0 else None
        got, exp, launches = play(ref, sides, orc, make_script(ref, n, 12), L)
    finally:
        L.speechPlayer_setGlobalOption(b"live_mode", 0)
        for s in sides + ([orc] if orc else []):
            s.close()
    if mode == 0:
        for k in range(n):
            compare(np.concatenate(got[k]), np.concatenate(exp[k]), "device bulk live stream %d" % k)
    assert max(launches) > 1, launches


def test_refusals_change_nothing(ref):
    """Refused with SPEECHPLAYER_ERR_ARGUMENT: page-locked and pageable host memory as deviceFrames, a misaligned pointer, a range past
    the allocation, a duplicated handle, a purge on an empty row, a decreasing frameStart (the last three through the host call too).
    After each, the next pull equals that of a twin set that never saw the call; the call with the same frames, accepted, then changes
    both alike."""
    import torch
    from nvspeechplayer_amd import _native, host_array
    L = _native.load()
    n = 12
    seeds = [300 + k for k in range(n)]
    a, twin = Side("device", seeds), Side("host", seeds)
    try:
        st = make_script(ref, n, 13)[0]
        for s in (a, twin):
            s.step(st)
        same(twin.pull(500), a.pull(500), "before")
        fa = scenarios.vowel_frame(ref, "a", 140.0, 120.0)
        fs, frames, m, f, ix, nu, pg = pack(n, {k: ([(fa, 300, 40, 77)] * 4 + [(None, 50, 0, 78)], k == 2) for k in range(n)})
        dev = a.group.device
        good = torch.from_numpy(frames).to("cuda:%d" % dev)
        pinned = host_array(frames.shape, np.float64)
        pinned[...] = frames
        pageable = np.ascontiguousarray(frames)
        huge = np.array([0] + [1 << 30] * n, np.int64)
        H = a.group._handles
        dup = (ctypes.c_void_p * n)(*([H[0], H[0]] + list(H[2:])))
        empty = fs.copy()
        empty[1] = 0                                 # handle 0 gets no frames ...
        purge0 = pg.copy()
        purge0[0] = 1                                # ... and a purge
        down = fs.copy()
        down[2] = fs[1] - 1
        P = lambda x: x.ctypes.data

        def on_device(handles, starts, ptr, purge=pg):
            return L.speechPlayer_queueFramesManyDevice(handles, n, P(starts), ptr, P(m), P(f), P(ix), P(nu), P(purge), None)

        def on_host(handles, starts, purge=pg):
            return L.speechPlayer_queueFramesMany(handles, n, P(starts), P(frames), P(m), P(f), P(ix), P(nu), P(purge))

        attempts = [("page-locked host memory", lambda: on_device(H, fs, pinned.ctypes.data)),
                    ("pageable host memory", lambda: on_device(H, fs, pageable.ctypes.data)),
                    ("misaligned", lambda: on_device(H, fs, good.data_ptr() + 4)),
                    ("past the allocation", lambda: on_device(H, huge, good.data_ptr())),
                    ("duplicated handle", lambda: on_device(dup, fs, good.data_ptr())),
                    ("purge on an empty row", lambda: on_device(H, empty, good.data_ptr(), purge0)),
                    ("decreasing frameStart", lambda: on_device(H, down, good.data_ptr())),
                    ("host: duplicated handle", lambda: on_host(dup, fs)),
                    ("host: purge on an empty row", lambda: on_host(H, empty, purge0)),
                    ("host: decreasing frameStart", lambda: on_host(H, down))]
        for name, call in attempts:
            assert call() == -1, name
            assert _native.last_error_code() == ERR_ARGUMENT, (name, _native.last_error())
            same(twin.pull(700), a.pull(700), name)
        assert on_device(H, fs, good.data_ptr()) == 0 and on_host(twin.group._handles, fs) == 0, _native.last_error()
        same(twin.pull(8192), a.pull(8192), "accepted")
    finally:
        a.close()
        twin.close()


def busy(cycles=100_000_000):
    """Keep torch's current stream busy for a while (so that anything not ordered behind it would run first)."""
    import torch
    torch.cuda._sleep(cycles)


def test_export_equals_host_pull(ref):
    """LiveGroup.pullTensor against LiveGroup.pull of twin sets over the script (pulls in pieces included: the joined rows): int16 rows
    are the host rows with zeros past produced; float32 into an `out` wider than the pull (rowStride > sampleCount) is int16 / 32767 bit
    for bit with zeros in the extra columns; a torch op queued on the same stream behind the export reads the right values without a
    synchronise; the tensor exported by pull k is unchanged after pull k + 1; "live_trim" with an export in flight does not corrupt it."""
    import torch
    from nvspeechplayer_amd import _native
    L = _native.load()
    n = 40
    seeds = [100 + k for k in range(n)]
    R, E, F = Side("host", seeds), Side("host", seeds), Side("host", seeds)
    try:
        dev = E.group.device
        launches, prev = [], None
        for i, st in enumerate(make_script(ref, n, 14)):
            for s in (R, E, F):
                s.step(st)
            cnt = st["pull"]
            want, marks = R.pull(cnt)
            launches.append(L.speechPlayer_lastLiveLaunches(dev))
            busy()                                   # the export is queued behind this on torch's stream
            pcm16, p16 = E.group.pullTensor(cnt, dtype=torch.int16)
            p16 = p16.copy()
            twice = pcm16.to(torch.int32) * 2        # on the same stream, no synchronise in between
            outf = torch.full((n, cnt + 5), 7.0, dtype=torch.float32, device="cuda:%d" % dev)
            pcmf, pf = F.group.pullTensor(cnt, out=outf)
            pf = pf.copy()
            assert pcm16.shape == (n, cnt) and pcmf.shape == (n, cnt) and pcmf.data_ptr() == outf.data_ptr()
            assert [p.getLastIndex() for p in E.players] == marks and [p.getLastIndex() for p in F.players] == marks, i
            rows = np.zeros((n, cnt + 5), np.int16)
            for k in range(n):
                assert p16[k] == len(want[k]) and pf[k] == len(want[k]), (i, k)
                rows[k, :len(want[k])] = want[k]
            got16 = pcm16.cpu().numpy()
            assert got16.tobytes() == rows[:, :cnt].tobytes(), i
            assert np.array_equal(twice.cpu().numpy(), rows[:, :cnt].astype(np.int32) * 2), i
            assert outf.cpu().numpy().tobytes() == (rows.astype(np.float32) / np.float32(32767)).tobytes(), i
            if prev is not None:
                assert prev[0].cpu().numpy().tobytes() == prev[1], i
            prev = (pcm16, got16.tobytes())
        assert max(launches) > 1, launches          # some pull went in pieces: its export read the joined rows
        # "live_trim" while an export waits behind a busy stream: the device's last handles close, the pull buffers go
        extra = {k: ([(fr, m, f, 9000 + j) for j, (fr, m, f) in enumerate(ref.ipa_case(k % 8))], False) for k in range(n)}
        for s in (R, E):
            s.step({"queue": extra})
        want, _ = R.pull(8192)
        busy()
        last, pl = E.group.pullTensor(8192, dtype=torch.int16)
        pl = pl.copy()
        F.close()
        R.close()
        assert L.speechPlayer_setGlobalOption(b"live_trim", 1) == 0
        E.close()
        rows = np.zeros((n, 8192), np.int16)
        for k in range(n):
            assert pl[k] == len(want[k]), k
            rows[k, :len(want[k])] = want[k]
        assert last.cpu().numpy().tobytes() == rows.tobytes()
    finally:
        L.speechPlayer_setGlobalOption(b"live_trim", 0)
        for s in (R, E, F):
            s.close()


def test_options_set_from_another_thread_while_pulls_run(ref):
    """speechPlayer_setGlobalOption from a second thread while the first pulls: a pull takes one snapshot of the live options on entry
    and finishes under it (a control block laid out for one kernel is never launched on another).  Six handles, one ref.ipa_case and
    one seed each; the second thread turns "live_alone" 1 / 1536, "live_replicate" 0 / 1 and "live_layout" 0 / 1 over and over; 1000
    samples per pull until every handle has run dry.  PCM and index marks against one oracle player each, sample for sample."""
    import threading
    import nvspeechplayer_amd as eng
    n = 6
    players = [eng.SpeechPlayer(22050, noiseSeed=900 + k) for k in range(n)]
    oracles = [oracle.OraclePlayer(22050, seed=900 + k) for k in range(n)]
    for k in range(n):
        for j, (fr, m, f) in enumerate(ref.ipa_case(3 * k + 1)):
            players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, j)
            oracles[k].queue(fr, m, f, j)
    stop = threading.Event()

    def set_options():
        i = 0
        while not stop.is_set():
            eng.setGlobalOption("live_alone", 1536 if i & 1 else 1)
            eng.setGlobalOption("live_replicate", (i >> 1) & 1)
            eng.setGlobalOption("live_layout", (i >> 2) & 1)
            i += 1

    t = threading.Thread(target=set_options)
    got, exp, dry = [[] for _ in range(n)], [[] for _ in range(n)], [False] * n
    try:
        t.start()
        group = eng.LiveGroup(players)
        out = np.zeros((n, 1000), np.int16)
        for pull in range(60):
            produced = group.pull(1000, out).copy()
            for k in range(n):
                got[k].append(out[k, :produced[k]].copy())
                exp[k].append(oracles[k].synthesize(1000))
                assert players[k].getLastIndex() == oracles[k].last_index(), (pull, k)
                dry[k] = dry[k] or produced[k] < 1000
            if all(dry):
                break
    finally:
        stop.set()
        t.join()
        eng.setGlobalOption("live_alone", 1536)
        eng.setGlobalOption("live_replicate", 1)
        eng.setGlobalOption("live_layout", 1)
        for p in players:
            p.close()
        for o in oracles:
            o.close()
    assert all(dry), dry
    for k in range(n):
        g, e = np.concatenate(got[k]), np.concatenate(exp[k])
        assert len(g) == len(e) and len(g) > 0 and np.array_equal(g, e), (k, len(g), len(e), int(np.count_nonzero(g[:len(e)] != e[:len(g)])))
