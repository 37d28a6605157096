"""Timelines of a batch on the host (include/speechPlayer_batch.h: speechPlayer_planTimeline, speechPlayer_batch_timeline,
speechPlayer_batch_exportTracks): declarations and bindings, speechPlayer_planTimeline against the oracle pulled one sample at a time,
the argument checks of BatchPlayer.trackTensor -- and `walk`, the comparand of tests/test_gpu_timeline.py: the reference's frame manager
(src/frame.cpp:41-80, with src/speechPlayer.cpp:36 and src/frame.cpp:98) restated sample by sample, itself held to the oracle here.
No GPU."""
import ctypes
import os
from collections import deque

import numpy as np
import pytest

from tests import oracle, scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
NEW_ENTRIES = ("speechPlayer_planTimeline", "speechPlayer_batch_timeline", "speechPlayer_batch_exportTracks")


def walk(frames, mins, fades, index, isnull):
    """One utterance through the reference's frame manager: every request queued into a fresh manager, getCurrentFrame() called until
    it answers NULL.  -> (cur [L, 47]: the frame each sample was computed from, mark [L]: getLastIndex() after the sample,
    frame [L]: the number of the request most recently dequeued).  Written the way src/frame.cpp states it: a queue, an old and a new
    request, a sample counter; no closed form."""
    with np.errstate(all="ignore"):
        queue = deque()
        for k in range(len(mins)):                                   # queueFrame, :90-101 (fade >= 1: speechPlayer.cpp:36)
            r = dict(min=int(mins[k]), fade=max(int(fades[k]), 1), null=bool(isnull[k]), frame=np.zeros(47), inc=np.float64(0.0),
                     index=int(index[k]))
            if not r["null"]:
                r["frame"] = np.array(frames[k], dtype=np.float64)
                r["inc"] = (r["frame"][46] - r["frame"][0]) / np.float64(r["min"])      # :98
            queue.append(r)
        old = dict(min=0, fade=0, null=True, frame=np.zeros(47), inc=np.float64(0.0), index=0)      # :85-88
        new = None
        cur = np.zeros(47)
        counter, last_index, taken = 0, -1, 0
        rows, marks, numbers = [], [], []
        while True:
            cur_is_null = False
            counter += 1                                             # :42
            if new is not None:
                if counter > new["fade"]:                            # :44-47
                    old, new = new, None
                else:                                                # :49-52
                    ratio = np.float64(counter) / np.float64(new["fade"])
                    o, t = old["frame"], new["frame"]
                    cur = np.where(np.isnan(t), o, o + ((t - o) * ratio))      # utils.h:20-23
            elif counter > old["min"]:                               # :54
                if queue:
                    new = queue.popleft()
                    if new["null"]:                                  # :59-63
                        new["frame"] = old["frame"].copy()
                        new["frame"][44] = 0.0
                        new["frame"][0] = cur[0]
                        new["inc"] = np.float64(0.0)
                    elif old["null"]:                                # :64-67
                        old["frame"] = new["frame"].copy()
                        old["frame"][44] = 0.0
                    if new["index"] != -1:                           # :69
                        last_index = new["index"]
                    counter = 0
                    new["frame"][0] = new["frame"][0] + (new["inc"] * new["fade"])      # :71
                    taken += 1
                else:
                    cur_is_null = True                               # :74
            else:                                                    # :77-78
                cur = cur.copy()
                cur[0] = cur[0] + old["inc"]
                old["frame"][0] = cur[0]
            if cur_is_null:
                break
            rows.append(cur); marks.append(last_index); numbers.append(taken - 1)
        out = np.array(rows, dtype=np.float64).reshape(len(rows), 47)
        return out, np.array(marks, dtype=np.int64), np.array(numbers, dtype=np.int64)


def marked(batch):
    """The batch with an index mark on every third frame."""
    k = np.arange(len(batch["index"]))
    batch = dict(batch)
    batch["index"] = np.where(k % 3 == 0, (k % 997).astype(np.int32), np.int32(-1)).astype(np.int32)
    return batch


def utterance(batch, u):
    a, e = int(batch["frame_start"][u]), int(batch["frame_start"][u + 1])
    return batch["frames"][a:e], batch["min"][a:e], batch["fade"][a:e], batch["index"][a:e], batch["isnull"][a:e]


def oracle_marks(batch, u, sr=22050):
    """Utterance u through an OraclePlayer pulled ONE sample at a time: (its sample count, last_index() after every sample)."""
    fr, m, f, ix, nu = utterance(batch, u)
    o = oracle.OraclePlayer(sr, seed=int(batch["seeds"][u]))
    for k in range(len(m)):
        o.queue(None if nu[k] else fr[k], int(m[k]), int(f[k]), int(ix[k]))
    marks = []
    while len(o.synthesize(1)) == 1:
        marks.append(o.last_index())
    o.close()
    return len(marks), np.array(marks, dtype=np.int64)


@pytest.fixture(scope="module")
def batches():
    return [marked(scenarios.random_batch(np.random.default_rng(5), 60)), marked(scenarios.random_batch(np.random.default_rng(5), 60, wild=True))]


@pytest.fixture(scope="module")
def pulled(batches):
    """[(batch, [(length, marks per sample) per utterance])]: 0.49 M one-sample pulls of the oracle."""
    return [(b, [oracle_marks(b, u) for u in range(len(b["frame_start"]) - 1)]) for b in batches]


def plan_timeline(frame_start, mins, fades):
    from nvspeechplayer_amd import _native
    L = _native.load()
    fs = np.ascontiguousarray(frame_start, dtype=np.int64)
    m = np.ascontiguousarray(mins, dtype=np.uint32)
    f = np.ascontiguousarray(fades, dtype=np.uint32)
    first = np.full(int(fs[-1]), -7, np.int64)
    length = np.full(len(fs) - 1, -7, np.int64)
    n = L.speechPlayer_planTimeline(len(fs) - 1, fs.ctypes.data, m.ctypes.data, f.ctypes.data, first.ctypes.data, length.ctypes.data)
    assert n == fs[-1]
    return first, length


def test_entry_points_are_declared_exported_and_bound():
    from nvspeechplayer_amd import _native
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name in NEW_ENTRIES:
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and fn.argtypes, name
    assert "#define SPEECHPLAYER_TRACK_MARK  47" in header and "#define SPEECHPLAYER_TRACK_FRAME 48" in header
    assert len(L.speechPlayer_batch_exportTracks.argtypes) == 11 and len(L.speechPlayer_batch_timeline.argtypes) == 5
    assert len(L.speechPlayer_planTimeline.argtypes) == 6


def test_a_null_batch_is_an_argument_error():
    from nvspeechplayer_amd import _native
    L = _native.load()
    cols = np.array([7], np.int32)
    assert L.speechPlayer_batch_exportTracks(None, None, 0, cols.ctypes.data, 1, 1, 0, None, 1, 0, None) == -1
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"exportTracks" in L.speechPlayer_lastError()
    assert L.speechPlayer_batch_timeline(None, 0, None, None, 0) == -1
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT


def test_plan_timeline_equals_the_oracle_pulled_sample_by_sample(pulled):
    """The samples after which last_index() changes, and the sample count at which the pull comes back empty, equal firstSample of the
    marked requests and length -- exactly, for every utterance."""
    samples = 0
    for b, per in pulled:
        first, length = plan_timeline(b["frame_start"], b["min"], b["fade"])
        for u, (n, marks) in enumerate(per):
            a, e = int(b["frame_start"][u]), int(b["frame_start"][u + 1])
            assert length[u] == n == oracle.utterance_length(b["min"][a:e], b["fade"][a:e]), u
            before = np.concatenate([[-1], marks[:-1]])
            changes = np.flatnonzero(marks != before)
            ks = [k for k in range(a, e) if b["index"][k] != -1]
            # (a mark equal to the one before it changes nothing the oracle shows: such requests are left out on both sides)
            shown, prev = [], -1
            for k in ks:
                if b["index"][k] != prev:
                    shown.append(k)
                prev = b["index"][k]
            assert list(changes) == [int(first[k]) for k in shown], u
            assert list(marks[changes]) == [int(b["index"][k]) for k in shown], u
            samples += n
    assert samples > 400000


def test_plan_timeline_refuses_bad_arguments():
    from nvspeechplayer_amd import _native
    L = _native.load()
    m = np.array([3, 4], np.uint32)
    for fs in ([0, 2, 1], [1, 2]):
        fs = np.array(fs, np.int64)
        assert L.speechPlayer_planTimeline(len(fs) - 1, fs.ctypes.data, m.ctypes.data, m.ctypes.data, None, None) == -1
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT
    fs = np.array([0, 2], np.int64)
    assert L.speechPlayer_planTimeline(1, fs.ctypes.data, None, m.ctypes.data, None, None) == -1
    assert L.speechPlayer_planTimeline(1, fs.ctypes.data, m.ctypes.data, None, None, None) == -1
    assert L.speechPlayer_planTimeline(1, None, m.ctypes.data, m.ctypes.data, None, None) == -1
    assert L.speechPlayer_planTimeline(-1, fs.ctypes.data, m.ctypes.data, m.ctypes.data, None, None) == -1
    assert L.speechPlayer_planTimeline(1, fs.ctypes.data, m.ctypes.data, m.ctypes.data, None, None) == 2      # (both outputs may be NULL)
    # fade 0 counts as 1 (speechPlayer.cpp:36)
    first, length = plan_timeline([0, 2], [0, 5], [0, 9])
    assert list(first) == [0, 3] and list(length) == [3 + 11]


def test_the_walk_is_held_to_the_oracle(pulled):
    """The comparand of the GPU tests: its length and its getLastIndex after every single sample are the oracle's."""
    for b, per in pulled:
        first, length = plan_timeline(b["frame_start"], b["min"], b["fade"])
        for u, (n, marks) in enumerate(per):
            cur, mark, number = walk(*utterance(b, u))
            assert len(cur) == len(mark) == len(number) == n, u
            assert np.array_equal(mark, marks), u
            a, e = int(b["frame_start"][u]), int(b["frame_start"][u + 1])
            assert np.array_equal(number, np.searchsorted(first[a:e], np.arange(n), side="right") - 1), u
            assert not cur[0].any()                                  # sample 0 sees the zeroed frame of a fresh handle


def test_walk_quirks_by_hand():
    """A vowel of 5 samples with a fade of 2, then silence: the dequeue samples repeat the frame before, the hold glides the pitch."""
    f = np.zeros(47); f[0] = 100.0; f[46] = 110.0; f[7] = 500.0; f[44] = 1.0
    cur, mark, number = walk(np.stack([f, np.zeros(47)]), [5, 2], [2, 1], [4, -1], [0, 1])
    # request 0: samples 0 .. 5 (max(5, 3) + 1), request 1: samples 6 .. 8 (max(2, 2) + 1)
    assert len(cur) == 9 and list(number) == [0] * 6 + [1] * 3 and list(mark) == [4] * 9
    inc = (110.0 - 100.0) / 5
    assert list(cur[:6, 7]) == [0.0, 500.0, 500.0, 500.0, 500.0, 500.0]          # from its own values: the old side was silence
    assert list(cur[:6, 44]) == [0.0, 0.5, 1.0, 1.0, 1.0, 1.0]                   # ... with the gain gated off
    top = 100.0 + inc * 2
    assert list(cur[:6, 0]) == [0.0, 100.0 + (top - 100.0) * 0.5, top, top, top + inc, top + inc + inc]
    assert list(cur[6:, 44]) == [1.0, 0.0, 0.0] and list(cur[6:, 7]) == [500.0] * 3 and list(cur[6:, 0]) == [top + inc + inc] * 3


def test_track_request_checks():
    import torch
    from nvspeechplayer_amd.speechPlayer import FRAME_FIELDS, check_track_request
    cols, hop, phase, fmt = check_track_request(["voicePitch", "cf1", 46, "mark", "frame", "cf1"], 256, 3, None)
    assert list(cols) == [0, 7, 46, 47, 48, 7] and cols.dtype == np.int32 and (hop, phase, fmt) == (256, 3, 1)
    assert check_track_request("endVoicePitch", 1, 0, torch.float64)[0].tolist() == [FRAME_FIELDS.index("endVoicePitch")]
    assert check_track_request(range(49), 1, 0, torch.float64)[3] == 0
    with pytest.raises(KeyError):
        check_track_request(["cf7"], 1, 0, None)
    with pytest.raises(ValueError):
        check_track_request([49], 1, 0, None)
    with pytest.raises(ValueError):
        check_track_request([-1], 1, 0, None)
    with pytest.raises(ValueError):
        check_track_request([], 1, 0, None)
    with pytest.raises(ValueError):
        check_track_request([0], 0, 0, None)
    with pytest.raises(ValueError):
        check_track_request([0], 1, -1, None)
    with pytest.raises(TypeError):
        check_track_request([0], 1, 0, torch.int16)
