"""Several BatchPlayers busy at the same time (tests/test_concurrent_players_host.py, tests/test_gpu_concurrent_players.py): the batches,
the thread skeleton and what a launch leaves behind.  include/speechPlayer_batch.h, "Threads", is the contract the two modules hold:
distinct batch objects, stages and live handles from distinct threads at once; one batch object by one thread at a time, handed on
under the caller's order; the last error per calling thread; "plan_hash_bits" read once per set call.

Six kinds of batch at 22 050 Hz, each built from an index k so that no two batches of a run are equal:

    S   workloads.make("cfg2", 2048, first=2048 k), both pitches times 1 + 0.01 k                    setUtterances         tracked flat stages
    I   workloads.cfg2_spec(1536, first=1536 k), the base pitches times 1 + 0.01 k                    setIpa                producer inside the call,
                                                                                                                            records, device expansion, labels
    W   random_batch(default_rng(100 + k), 600, wild=True)                                            setUtterances         every class, NaN holds, untracked
                                                                                                                            and direct groups side by side
    V   the 70 quiet nasal-free vowels of tests/player_script.py step A, both pitches plus k Hz       setUtterances         lane-pipelined kernel, replicas
    L   the 6 shared lists under 65 seeds of tests/player_script.py step F, seeds plus k              setUtterancesShared   shared frame lists
    P   workloads.make("cfg2", 16384, first=16384 k), both pitches times 1 + 0.01 k: 395 000 frames   setUtterances         above the 200 000 frames from
                                                                                                                            which a set call plans in parts
                                                                                                                            on the process-wide pool

(512 utterances are one period of the cfg2 recipe: batches of S, I and P that differ in k alone differ in their noise seeds -- which a
sentence without noise does not hear: one of the eight sampleIpa lines is such --, so S, I and P are given other pitches too, as
bench.py's `pipeline` extra gives its batches of either source.)  The runs of tests/test_gpu_concurrent_players.py's tests 2 to 5 take S and I at SMALL counts, no multiple of a wavefront.

This module imports neither torch nor the engine when it is imported: a builder imports what it needs when it is called."""
import collections
import functools
import threading
import time

import numpy as np

SR = 22050
KINDS = ("S", "I", "W", "V", "L", "P")
ENTRY = dict(S="setUtterances", I="setIpa", W="setUtterances", V="setUtterances", L="setUtterancesShared", P="setUtterances")
COUNTS = dict(S=2048, I=1536, W=600, V=70, L=65, P=16384)
SMALL = dict(S=520, I=392)                      # tests 2 to 5: a wavefront holds 64 utterances; 520 = 8 x 64 + 8, 392 = 6 x 64 + 8
PART_FRAMES = 200000                            # klatt_engine.hip: a set call of at least this many frames plans in parts
# test 1, the pipeline: batch j of the run is (kind, k = j); the two P are neighbours, so that two set calls above the threshold overlap
PIPELINE = tuple((kind, k) for k, kind in enumerate("SIWPPVLSIWVL"))
# tests 2, 3 and 5: thread t walks four batches of different kinds, none of them P; (kind, k, count)
WALK_KINDS = "SIWVL"
WALKS = tuple(tuple((WALK_KINDS[(t + j) % 5], 20 + 4 * t + j, SMALL.get(WALK_KINDS[(t + j) % 5])) for j in range(4)) for t in range(6))
# what routing decides (BatchPlayer.kernelInfo())
ROUTING = ("tracked_utterances", "direct_utterances", "lane_pipelined_utterances", "nasal_free_utterances", "tracked", "direct", "lane_pipelined",
           "nasal_free", "stage_parallel_chunk")


# ---- the batches ------------------------------------------------------------------------------------------------------------------------

def _frozen(b):
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _frozen(v)
    return b


def batch(kind, k, count=None):
    """Batch k of a kind (count None: of COUNTS[kind] utterances), built once per process; nobody writes to it.  A dict as
    tests/player_script.py's _flat makes it -- what tests/oracle.batch_synthesize takes, every array of the dtype the set calls take --
    with `kind`, `k`, and by entry point `call` (setIpa's keywords) or `lists` and `list_of` (setUtterancesShared's)."""
    n = COUNTS[kind] if count is None else int(count)
    assert kind in ("S", "I", "P") or n == COUNTS[kind], (kind, count)
    return _batch(kind, int(k), n)


@functools.lru_cache(maxsize=None)
def _batch(kind, k, n):
    from nvspeechplayer_amd import workloads
    from tests import player_script as ps
    more = {}
    if kind in ("S", "P"):
        b = dict(workloads.make("cfg2", n, first=n * k))
        fr = b["frames"].copy()
        fr[:, 0] *= 1.0 + 0.01 * k; fr[:, 46] *= 1.0 + 0.01 * k
        b["frames"] = fr
    elif kind == "I":
        from nvspeechplayer_amd import ipa
        spec = workloads.cfg2_spec(n, first=n * k)
        spec["basePitch"] = spec["basePitch"] * (1.0 + 0.01 * k)
        # what the call sets, frame for frame: the producer's frames through speechPlayer_ipa_pack (tests/test_gpu_compact.py holds setIpa to them)
        b = ipa.frames_for_batch(sampleRate=SR, **{key: v for key, v in spec.items() if key != "noiseSeed"})
        b.update(index=np.full(len(b["min"]), -1, np.int32), seeds=spec["noiseSeed"])
        more["call"] = spec
    elif kind == "W":
        b = ps.random_batch(np.random.default_rng(100 + k), n, wild=True)
    elif kind == "V":
        b = dict(ps.build_a())
        fr = b["frames"].copy()
        real = b["isnull"] == 0
        fr[real, 0] += k; fr[real, 46] += k
        b["frames"] = fr
    elif kind == "L":
        b = dict(ps.build_f())
        b["seeds"] = (b["seeds"] + np.uint32(k)).astype(np.uint32)
        more.update(lists=b["lists"], list_of=b["list_of"])
    else:
        raise KeyError(kind)
    flat = ps._flat({key: b[key] for key in ("frame_start", "frames", "min", "fade", "index", "isnull", "seeds")}, kind=kind, k=k, **more)
    return _frozen(flat)


def set_batch(bp, b):
    """The batch's set call on player bp."""
    entry = ENTRY[b["kind"]]
    if entry == "setUtterances":
        bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
    elif entry == "setIpa":
        bp.setIpa(**b["call"])
    else:
        l = b["lists"]
        bp.setUtterancesShared(l["frame_start"], l["frames"], l["min"], l["fade"], b["list_of"], l["index"], l["isnull"], b["seeds"])


def fingerprint(bp, kind, read=None, routing=True):
    """What a launch leaves behind: readAll()'s bytes and starts (`read`: a (pcm, starts) pair read some other way, taken instead), or
    digest(per_utterance=True) alone for kind P, whose PCM is 0.76 GB; getLastIndex of every utterance; totalSamples and totalFrames;
    the kernelInfo() entries that routing decides (routing=False: without them).  An ordered dict of plain values: == compares two."""
    out = collections.OrderedDict()
    if kind == "P":
        whole, per = bp.digest(per_utterance=True)
        out["digest"] = (whole, per.tobytes())
    else:
        pcm, starts = bp.readAll() if read is None else read
        out["pcm"], out["starts"] = np.ascontiguousarray(pcm).tobytes(), np.ascontiguousarray(starts, np.int64).tobytes()
    out["lastIndex"] = [bp.getLastIndex(u) for u in range(bp.nUtterances)]
    out["totals"] = (int(bp.totalSamples), int(bp.totalFrames))
    if routing:
        info = bp.kernelInfo()
        out["routing"] = tuple((key, info[key]) for key in ROUTING)
    return out


def differing(got, want):
    """The entries of two fingerprints (or any two dicts of plain values) that are not equal."""
    return [key for key in want if key not in got or got[key] != want[key]] + [key for key in got if key not in want]


# ---- the thread skeleton ----------------------------------------------------------------------------------------------------------------

class StillRunning(AssertionError):
    """Threads that had not finished when the limit passed."""


class Cancelled(RuntimeError):
    """A wait given up because another thread of the run raised, or the limit passed."""


def limit_for(sequential_s):
    """The limit of a concurrent pass: a liveness guard, not a speed bar."""
    return max(30.0, 20.0 * sequential_s)


class Run:
    """run_threads' hand to its targets: `cancel` is set once a thread has raised or the limit has passed, and the waits below give
    up then, so that no thread outlives the run waiting for another that will never come."""

    def __init__(self):
        self.cancel = threading.Event()
        self._lock, self._meetings = threading.Lock(), {}

    def wait(self, event):
        while not event.wait(0.02):
            if self.cancel.is_set():
                raise Cancelled("waiting for an event")

    def acquire(self, semaphore):
        while not semaphore.acquire(timeout=0.02):
            if self.cancel.is_set():
                raise Cancelled("waiting for a semaphore")

    def meet(self, key, parties):
        """A rendezvous of `parties` threads under the name `key`: returns once all have arrived."""
        with self._lock:
            m = self._meetings.setdefault(key, [threading.Event(), 0])
            m[1] += 1
            if m[1] >= parties:
                m[0].set()
        self.wait(m[0])


def run_threads(targets, limit_s, run=None):
    """targets: (name, callable) pairs, each run on a daemon thread of that name.  -> {name: what the callable returned}.  The first
    exception raised in a thread is raised again here (a Cancelled that followed it is not the first); threads still alive limit_s
    seconds after the start fail the run by name (StillRunning) -- nothing here waits without a limit, and no step is tried twice.
    run: the Run whose `cancel` the targets' waits watch."""
    run = run or Run()
    results, errors, lock = {}, [], threading.Lock()

    def body(name, fn):
        def go():
            try:
                results[name] = fn()
            except BaseException as e:      # noqa: BLE001 -- raised again by the caller
                with lock:
                    errors.append((name, e))
                run.cancel.set()
        return go
    threads = [threading.Thread(target=body(name, fn), name=name, daemon=True) for name, fn in targets]
    assert len({t.name for t in threads}) == len(threads)
    deadline = time.monotonic() + limit_s
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [t.name for t in threads if t.is_alive()]
    if alive:
        run.cancel.set()
    with lock:
        first = next((e for e in errors if not isinstance(e[1], Cancelled)), errors[0] if errors else None)
    if first is not None:
        if alive:
            print("still alive after %.1f s: %s" % (limit_s, ", ".join(alive)))
        raise first[1]
    if alive:
        raise StillRunning("still alive after %.1f s: %s" % (limit_s, ", ".join(alive)))
    return results


def overlaps(a, b):
    """Two (start, end) intervals of one clock share a moment."""
    return a[0] < b[1] and b[0] < a[1]


# ---- the planning views and the producer's, as bytes ------------------------------------------------------------------------------------

def planning_views(b, eligible=None, budget_mb=16384):
    """speechPlayer_planTracks, speechPlayer_planTrackKinds, speechPlayer_planDirect and speechPlayer_planTimeline on a batch (or on the
    lists of a shared one): an ordered dict of every output array's bytes and every count."""
    import ctypes
    from nvspeechplayer_amd import _native
    L = _native.load()
    b = b.get("lists", b)
    nu, nf = len(b["frame_start"]) - 1, len(b["min"])
    frames = np.ascontiguousarray(b["frames"], np.float64)
    fs, fade, minimum, nul = b["frame_start"], b["fade"], b["min"], b["isnull"]
    el = None if eligible is None else np.ascontiguousarray(eligible, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data
    out = collections.OrderedDict()
    for name in ("planTracks", "planTrackKinds"):
        off, mask, tracked = np.zeros(max(nf, 1), np.uint64), np.zeros(max(nf, 1), np.uint32), np.zeros(max(nu, 1), np.uint8)
        entries, kinds = ctypes.c_ulonglong(0), np.zeros(max(nu, 1), np.uint32)
        args = (nu, p(fs), p(frames), p(fade), p(nul), p(el), budget_mb, p(off), p(mask), p(tracked), ctypes.byref(entries))
        got = L.speechPlayer_planTracks(*args) if name == "planTracks" else L.speechPlayer_planTrackKinds(*args, p(kinds))
        assert got >= 0, _native.last_error()
        out[name] = (int(got), int(entries.value), off.tobytes(), mask.tobytes(), tracked.tobytes(), kinds.tobytes())
    frm, to, flags = (np.zeros(max(nf, 1), np.uint32) for _ in range(3))
    got = L.speechPlayer_planDirect(nu, p(fs), p(nul), p(frm), p(to), p(flags))
    assert got == nf, _native.last_error()
    out["planDirect"] = (int(got), frm.tobytes(), to.tobytes(), flags.tobytes())
    first, length = np.zeros(max(nf, 1), np.int64), np.zeros(max(nu, 1), np.int64)
    got = L.speechPlayer_planTimeline(nu, p(fs), p(minimum), p(fade), p(first), p(length))
    assert got == nf, _native.last_error()
    out["planTimeline"] = (int(got), first.tobytes(), length.tobytes())
    return out


def producer_views(spec, sample_rates=(22050, 16000)):
    """speechPlayer_ipa_records, speechPlayer_ipa_pack (at two sample rates) and speechPlayer_ipa_labels on the texts of a setIpa call:
    an ordered dict of every output array's bytes."""
    from nvspeechplayer_amd import ipa
    kw = dict(texts=spec["texts"], speed=spec["speed"], basePitch=spec["basePitch"], inflection=spec["inflection"], clauseType=spec["clauseType"],
              trailing_silence_ms=spec["trailing_silence_ms"], textOf=spec["textOf"])
    out = collections.OrderedDict()
    pk = ipa.records_for_batch(sampleRate=SR, **kw)
    out["ipa_records"] = tuple(pk[key].tobytes() for key in ("shapes", "list_start", "records", "list_of", "labels"))
    for rate in sample_rates:
        pk = ipa.frames_for_batch(sampleRate=rate, **kw)
        out["ipa_pack at %d" % rate] = tuple(pk[key].tobytes() for key in ("frame_start", "frames", "min", "fade", "isnull"))
    out["ipa_labels"] = tuple(ipa.labels(t).tobytes() for t in spec["texts"])
    return out
