"""The script one long-lived BatchPlayer is walked through (tests/test_player_script_host.py, tests/test_gpu_player_script.py): small
batches at 22 050 Hz that differ in class, entry point and size from one to the next, so that every device buffer of the engine's Batch
is at some point reused in place under the tail of a larger batch and at some point freed and allocated again, and every freshness
flag and cached table has a batch before it to be stale from.  Host only: nothing here touches a device; `apply` calls the set entry
of whatever player it is handed.

    A   70 quiet nasal-free vowels of one timing: a full wavefront and a tail of 6 whose empty lanes get replicas    setUtterances
    B   three IPA texts in four voices at several pitches, 42 utterances: records expanded on the device, labels     setIpa
    C   a wild random batch of 37: NaN holds, NULL frames, M = 0 frames; fewer frames than B                        setUtterances
    D   edge_batch, 101 utterances, under tracks = 0, direct = 2                                                     setUtterances
    E   the mixed batch, 130 utterances of every class, under tracks = 1, direct = 1, track_budget_mb = 1            setUtterances
    F   6 lists spoken by 64 + 1 utterances under seeds of their own; two lists spoken by nobody, one empty          setUtterancesShared
    G   C's frames as a device tensor on a side stream, under other noise seeds                                      setUtterancesTensor
    H0  no utterance at all                                                                                          setUtterances
    H3  three utterances of which two have no frames                                                                 setUtterances
    A'  A again                                                                                                      setUtterances

A step is a record of five things: the builder of its batch, the set entry, the options in force at its set call (every option a
step does not name is at its default: `set_options`), the launch walk it has in tests/test_gpu_player_script.py's second test (None: none)
and the routing predicate over (kernelInfo(), hasLabels, the classes of the batch).
"""
import collections
import ctypes
import functools

import numpy as np

from nvspeechplayer_amd import _native, ipa, workloads
from tests import oracle
from tests.scenarios import random_batch
from tests.test_gpu_rates import edge_batch
from tests.test_gpu_source import batch_of
from tests.test_gpu_stems import noisy

SR = 22050
THREADS = 16
K_TILE = 32                     # the pool holds every utterance padded to whole PCM tiles (klatt_consts.h: kTile)
MIN_SAMPLES = 25                # tests/test_one_at_a_time_host.py's floor: samples that differ by more than 1 LSB

# every option of speechPlayer_batch_setOption at its default (include/speechPlayer_batch.h)
DEFAULTS = collections.OrderedDict(mode=0, sort=1, layout=-1, tracks=1, track_budget_mb=4096, direct=1, direct_lean=-1, quiet_last=1,
                                   pitch_table_mb=256, source_table_mb=256, source_lane_lists=12288)

# frame facts (speechPlayer_frameFacts) and the classes of an utterance that the routing knows (klatt_batchplan.h: classify_list)
FACT_NOISE, FACT_NONFINITE, FACT_NASAL, FACT_UNBOUNDED = 1, 2, 4, 8
CLASSES = ("no_nasal", "quiet", "noisy_finite", "non_finite")

Step = collections.namedtuple("Step", "name build entry options walk routed")

# the launch walks of test_options_between_set_and_launch: the options changed before each further launch of a batch set once
WALK_E = (dict(), dict(tracks=0), dict(tracks=1), dict(layout=0), dict(layout=2), dict(layout=1), dict(layout=-1), dict(mode=1),
          dict(mode=1, direct_lean=0), dict(mode=1, direct_lean=1), dict(mode=0), dict(quiet_last=0), dict(quiet_last=1))
WALK_A = (dict(layout=-1, mode=0), dict(layout=1, mode=1), dict(layout=0, mode=0), dict(layout=2, mode=0), dict(layout=2, mode=1), dict(layout=-1, mode=0))


def set_options(bp, options):
    """Every option back to its default, then the step's own."""
    for k, v in DEFAULTS.items():
        bp.setOption(k, options.get(k, v))


# ---- the batches ------------------------------------------------------------------------------------------------------------------------

def _flat(b, **more):
    """A batch as tests/oracle.batch_synthesize takes it, every array of the dtype the set calls take."""
    out = dict(frame_start=np.ascontiguousarray(b["frame_start"], np.int64), frames=np.ascontiguousarray(b["frames"], np.float64).reshape(-1, 47),
               min=np.ascontiguousarray(b["min"], np.uint32), fade=np.ascontiguousarray(b["fade"], np.uint32),
               index=np.ascontiguousarray(b["index"], np.int32), isnull=np.ascontiguousarray(b["isnull"], np.uint8),
               seeds=np.ascontiguousarray(b["seeds"], np.uint32))
    out["n_lists"] = len(out["frame_start"]) - 1
    out["list_frames"] = len(out["min"])
    out.update(more)
    return out


def _vowel(u, seconds):
    """Utterance u of BASELINE configs[1] (a steady vowel and the silence after it), `seconds` long."""
    return workloads.cfg1_steady_vowels(1, seconds=seconds, first=u)


def build_a():
    b = workloads.cfg1_steady_vowels(70, seconds=0.2)
    b["seeds"] = (b["seeds"] + 1000).astype(np.uint32)
    b["index"] = (np.arange(140) * 3 % 401).astype(np.int32)
    return _flat(b)


def build_b():
    lines = [x.decode("utf8") for x in workloads._load()["ipa_lines"]]
    texts = [lines[0], lines[4].split()[0] + " " + lines[4].split()[1], lines[6].split()[2]]
    n = 42
    text_of = np.arange(n) % 3
    voice = (np.arange(n) // 3 % 4).astype(np.int32)
    pitch = 90.0 + 7.0 * (np.arange(n) // 12)
    seeds = (np.arange(n) * 7919 + 5).astype(np.uint32)
    kw = dict(texts=texts, speed=1.6, basePitch=pitch, inflection=0.5, clauseType=".", voice=voice, trailing_silence_ms=12.0, textOf=text_of)
    pk = ipa.records_for_batch(sampleRate=SR, **kw)
    ex = ipa.expand_records(pk)
    lo = pk["list_of"]
    idx = np.concatenate([np.arange(pk["list_start"][l], pk["list_start"][l + 1]) for l in lo])
    ex["index"] = pk["records"]["index"][idx]
    ex["seeds"] = seeds
    return _flat(ex, call=dict(kw, noiseSeed=seeds), records=pk, n_lists=len(pk["list_start"]) - 1, list_frames=len(pk["records"]))


def build_c():
    b = random_batch(np.random.default_rng(1203), 37, wild=True)
    b["index"] = np.where(np.arange(len(b["min"])) % 4 != 2, 7000 + np.arange(len(b["min"])), -1).astype(np.int32)
    return _flat(b)


def build_d():
    return _flat(edge_batch(np.random.default_rng(404), SR, 101))


def build_e():
    """40 quiet nasal-free vowels of one timing and 34 quiet nasal ones of another (runs the quiet kernels keep), 44 noisy utterances
    with finite parameters and timings of their own -- under a 1 MB budget the tracks run out after forty of them --, 12 that hold a NaN."""
    rng = np.random.default_rng(77)
    utts, seeds = [], []
    for u in range(40):
        v = _vowel(3 * u + 1, 0.15)
        utts.append([(v["frames"][0], int(v["min"][0]), int(v["fade"][0])), (None, int(v["min"][1]), int(v["fade"][1]))])
    for u in range(34):
        v = _vowel(5 * u + 2, 0.1)
        f = v["frames"][0].copy()
        f[23], f[13], f[14], f[21], f[22] = 0.4 + 0.01 * u, 420.0 + u, 260.0, 90.0, 110.0
        g = f.copy(); g[7] *= 1.1; g[23] = 0.1
        utts.append([(f, 1500, 300), (g, 900, 410), (None, 200, 150)])
    for u in range(44):
        # forty share eight sets of shapes and their fade lengths -- and so their tracks (a shape holds every parameter but the two pitches) -- under
        # pitches and durations of their own; the last four have shapes of their own and fades too long for what the budget has left
        own = u >= 40
        shift, long = (4.0 * u, 4000) if own else (6.0 * (u % 8), 0)
        a = noisy(110.0 + 3 * u, 150.0 - u, shift=shift)
        b = noisy(170.0 - u, 90.0 + u, frication=0.7, shift=-shift - 30.0)
        c = noisy(130.0, 131.0 + u, turbulence=0.1, aspiration=0.5, shift=1.5 * shift + 11.0)
        utts.append([(a, 700 + 13 * u, 150 + long), (None, 40 + u, 30), (b, 900 - 11 * u, 333), (c, 500 + 7 * u + long, 250 + long), (None, 100 + u, 60)])
    for u in range(12):
        a = noisy(120.0 + 5 * u, 100.0, shift=10.0 * u)
        h = noisy(140.0, 160.0 + u, shift=-20.0)
        h[[8 + u % 4, 16, 40]] = np.nan
        utts.append([(a, 800 + 31 * u, 200), (h, 1100, 377 + u), (a, 300, 100 + u), (None, 90, 50)])
    order = rng.permutation(len(utts))
    b = batch_of([utts[i] for i in order])
    b["seeds"] = rng.integers(0, 2 ** 32, len(utts)).astype(np.uint32)
    b["index"] = np.where(np.arange(len(b["min"])) % 3 == 1, np.arange(len(b["min"])) % 911, -1).astype(np.int32)
    return _flat(b)


def build_f():
    """Lists 0, 1 and 3 spoken by 64 utterances, list 4 (empty) by one; lists 2 and 5 by nobody."""
    src = random_batch(np.random.default_rng(66), 6, quiet_fraction=0.0)
    fs = src["frame_start"]
    keep = [l for l in range(6) if l != 4]
    rows = np.concatenate([np.arange(fs[l], fs[l + 1]) for l in keep])
    counts = [0 if l == 4 else int(fs[l + 1] - fs[l]) for l in range(6)]
    lists = dict(frame_start=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), frames=src["frames"][rows], min=src["min"][rows],
                 fade=src["fade"][rows], index=(np.arange(len(rows)) % 50).astype(np.int32), isnull=src["isnull"][rows])
    list_of = np.array([(0, 1, 3)[u % 3] for u in range(64)] + [4], np.uint32)
    list_of[40] = 4; list_of[64] = 3                # (the empty list's utterance sits among the others)
    seeds = (np.arange(65) * 104729 + 11).astype(np.uint32)
    ls = lists["frame_start"]
    rows_u = [np.arange(ls[l], ls[l + 1]) for l in list_of]
    take = np.concatenate(rows_u).astype(np.int64)
    flat = dict(frame_start=np.concatenate([[0], np.cumsum([len(r) for r in rows_u])]), frames=lists["frames"][take], min=lists["min"][take],
                fade=lists["fade"][take], index=lists["index"][take], isnull=lists["isnull"][take], seeds=seeds)
    return _flat(flat, lists=_flat(dict(lists, seeds=np.zeros(6, np.uint32))), list_of=list_of, n_lists=6, list_frames=len(rows))


def build_g():
    b = dict(build_c())
    b["seeds"] = (b["seeds"] ^ np.uint32(0x5A5A5A5A)).astype(np.uint32)
    return _flat(b)


def build_h0():
    return _flat(batch_of([]))


def build_h3():
    b = batch_of([[], [(noisy(200.0, 180.0), 421, 77), (None, 33, 20)], []])
    b["seeds"] = np.array([9, 8, 7], np.uint32)
    b["index"] = np.array([31, 32], np.int32)
    return _flat(b)


def _classes_present(c, *names):
    return all(c[n] > 0 for n in names)


def routed_a(info, has_labels, classes):
    return info["lane_pipelined"] and info["lane_pipelined_utterances"] == 70 and info["tracked_utterances"] == 0 and info["direct_utterances"] == 0 and not has_labels


def routed_b(info, has_labels, classes):
    return info["tracked_utterances"] > 0 and has_labels


def routed_untracked(info, has_labels, classes):
    """The untracked noisy group is not empty: utterances with a non-finite parameter get neither tracks nor the direct stages."""
    n = sum(classes.values())
    return classes["non_finite"] > 0 and info["tracked_utterances"] + info["direct_utterances"] <= n - classes["non_finite"] and not has_labels


def routed_d(info, has_labels, classes):
    return info["direct_utterances"] > 0 and info["tracked_utterances"] == 0 and not has_labels


def routed_e(info, has_labels, classes):
    """(kernelInfo() counts the nasal-free group under the kernel that runs it: the lane-pipelined one for a batch this small)"""
    return (info["nasal_free_utterances"] + info["lane_pipelined_utterances"] > 0 and info["tracked_utterances"] > 0 and info["direct_utterances"] > 0 and
            routed_untracked(info, has_labels, classes))


def routed_none(info, has_labels, classes):
    return all(info[k] == 0 for k in ("lane_pipelined_utterances", "nasal_free_utterances", "tracked_utterances", "direct_utterances")) and not has_labels


def routed_any(info, has_labels, classes):
    return not has_labels


SCRIPT = (
    Step("A", build_a, "setUtterances", {}, WALK_A, routed_a),
    Step("B", build_b, "setIpa", {}, None, routed_b),
    Step("C", build_c, "setUtterances", {}, None, routed_untracked),
    Step("D", build_d, "setUtterances", dict(tracks=0, direct=2), None, routed_d),
    Step("E", build_e, "setUtterances", dict(tracks=1, direct=1, track_budget_mb=1), WALK_E, routed_e),
    Step("F", build_f, "setUtterancesShared", {}, None, routed_any),
    Step("G", build_g, "setUtterancesTensor", {}, None, routed_untracked),
    Step("H0", build_h0, "setUtterances", {}, None, routed_none),
    Step("H3", build_h3, "setUtterances", {}, None, routed_any),
    Step("A'", build_a, "setUtterances", {}, None, routed_a),
)
NAMES = tuple(s.name for s in SCRIPT)


@functools.lru_cache(maxsize=None)
def built(name):
    """The batch of a step, built once per process; nobody writes to it."""
    b = SCRIPT[NAMES.index(name)].build()
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


def apply(bp, step, stream=None):
    """The step's options and its set call on player bp.  stream: the torch stream a device tensor's upload is queued on."""
    b = built(step.name)
    set_options(bp, step.options)
    if step.entry == "setUtterances":
        bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
    elif step.entry == "setIpa":
        bp.setIpa(**b["call"])
    elif step.entry == "setUtterancesShared":
        l = b["lists"]
        bp.setUtterancesShared(l["frame_start"], l["frames"], l["min"], l["fade"], b["list_of"], l["index"], l["isnull"], b["seeds"])
    elif step.entry == "setUtterancesTensor":
        import torch
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(bp.device)):
            frames = torch.from_numpy(np.array(b["frames"])).to("cuda:%d" % bp.device, non_blocking=True)
            bp.setUtterancesTensor(b["frame_start"], frames, b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
    else:
        raise ValueError(step.entry)


# ---- what the host knows of a batch -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (oracle PCM, starts, index mark per utterance after its end) of a step's batch."""
    b = built(name)
    if len(b["frame_start"]) == 1:
        return np.zeros(0, np.int16), np.zeros(1, np.int64), np.zeros(0, np.int32)
    pcm, start, _ = oracle.batch_synthesize(SR, b, threads=THREADS)
    return pcm, start, oracle.batch_last_index(SR, b, threads=THREADS)


def timeline(b):
    """speechPlayer_planTimeline's tables: (first sample of every request, length of every utterance)."""
    n = len(b["frame_start"]) - 1
    first, length = np.zeros(max(len(b["min"]), 1), np.int64), np.zeros(max(n, 1), np.int64)
    got = _native.load().speechPlayer_planTimeline(n, b["frame_start"].ctypes.data, b["min"].ctypes.data, b["fade"].ctypes.data, first.ctypes.data, length.ctypes.data)
    assert got == len(b["min"]), _native.last_error()
    return first[:len(b["min"])], length[:n]


def frame_facts(b):
    """The flags word speechPlayer_frameFacts gives every frame."""
    n = len(b["min"])
    raw = np.zeros((max(n, 1), 3), np.uint64)
    if n:
        frames = np.ascontiguousarray(b["frames"])
        assert _native.load().speechPlayer_frameFacts(frames.ctypes.data, n, SR, 0, raw.ctypes.data) == n
    return (raw[:n, 2] & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def utterance_classes(b):
    """The class of every utterance by the rule of classify_list over speechPlayer_frameFacts' flags (NULL frames carry no
    parameters; speechPlayer_planDirect says which frames a fade ends on, and a frame no fade ends on reaches nothing): an array of
    indices into CLASSES."""
    n, nf = len(b["frame_start"]) - 1, len(b["min"])
    flags = frame_facts(b)
    to = np.zeros(max(nf, 1), np.uint32); frm = np.zeros(max(nf, 1), np.uint32); fl = np.zeros(max(nf, 1), np.uint32)
    got = _native.load().speechPlayer_planDirect(n, b["frame_start"].ctypes.data, b["isnull"].ctypes.data if nf else None,
                                                frm.ctypes.data, to.ctypes.data, fl.ctypes.data)
    assert got == nf, _native.last_error()
    out = np.zeros(n, np.int64)
    for u in range(n):
        a, e = int(b["frame_start"][u]), int(b["frame_start"][u + 1])
        word = 0
        for k in range(a, e):
            if not b["isnull"][k]:
                assert to[k] == k, (u, k, to[k])       # a real frame is its own fade's end
                word |= int(flags[k])
        if word & FACT_NONFINITE:
            out[u] = 3
        elif word & FACT_NOISE:
            out[u] = 2
        else:
            out[u] = 1 if word & FACT_NASAL else 0
    return out


def class_counts(b):
    c = utterance_classes(b)
    return {name: int(np.count_nonzero(c == i)) for i, name in enumerate(CLASSES)}


def track_entries(step):
    """The 16-byte track entries speechPlayer_planTracks plans for the step's lists under the step's options: the noisy lists with
    finite parameters are eligible, as in the engine."""
    b = built(step.name)
    opts = dict(DEFAULTS, **step.options)
    lists = b.get("lists", b)
    if step.entry == "setIpa":
        pk = b["records"]
        silent = pk["records"]["shape"] == ipa.RECORD_SILENCE
        fr = np.zeros((len(silent), 47))
        fr[~silent] = pk["shapes"][pk["records"]["shape"][~silent]]
        fr[~silent, 0] = pk["records"]["voicePitch"][~silent]; fr[~silent, 46] = pk["records"]["endVoicePitch"][~silent]
        lists = _flat(dict(frame_start=pk["list_start"], frames=fr, min=pk["records"]["min"], fade=pk["records"]["fade"],
                           index=pk["records"]["index"], isnull=silent, seeds=np.zeros(len(pk["list_start"]) - 1)))
    n = len(lists["frame_start"]) - 1
    if not opts["tracks"] or not len(lists["min"]):
        return 0
    spoken = np.ones(n, bool) if "list_of" not in b else np.isin(np.arange(n), b["list_of"])
    eligible = ((utterance_classes(lists) == 2) & spoken).astype(np.uint8)
    tracked, entries = np.zeros(n, np.uint8), ctypes.c_ulonglong(0)
    frames = np.ascontiguousarray(lists["frames"])
    got = _native.load().speechPlayer_planTracks(n, lists["frame_start"].ctypes.data, frames.ctypes.data, lists["fade"].ctypes.data, lists["isnull"].ctypes.data,
                                                 eligible.ctypes.data, opts["track_budget_mb"], None, None, tracked.ctypes.data, ctypes.byref(entries))
    assert got >= 0, _native.last_error()
    return int(entries.value) if tracked.any() else 0


def counted(step):
    """The quantities the engine's buffers are sized by."""
    b = built(step.name)
    _, length = timeline(b)
    return dict(frames=int(b["list_frames"]), utterances=len(b["frame_start"]) - 1, lists=int(b["n_lists"]),
                pool_samples=int(((length + K_TILE - 1) // K_TILE * K_TILE).sum()), track_entries=track_entries(step))


def rows_differing(pcm_a, start_a, pcm_b, start_b):
    """Per row both batches have: the samples that differ by more than 1 LSB, a sample only one of the two has counting as one."""
    n = min(len(start_a), len(start_b)) - 1
    out = np.zeros(n, np.int64)
    for u in range(n):
        x, y = pcm_a[start_a[u]:start_a[u + 1]].astype(np.int32), pcm_b[start_b[u]:start_b[u + 1]].astype(np.int32)
        m = min(len(x), len(y))
        out[u] = np.count_nonzero(np.abs(x[:m] - y[:m]) > 1) + abs(len(x) - len(y))
    return out
