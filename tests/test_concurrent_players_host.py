"""tests/concurrent_players.py on the host, no GPU needed: that the batches of tests/test_gpu_concurrent_players.py hold what they claim
-- a player that handed out another player's batch would pass unnoticed if two batches of a run were alike --, and the half of the
threads contract of include/speechPlayer_batch.h that needs no device: the planning views and the producer's calls from several threads
at once give, byte for byte, what the same calls give alone (the views plan on the process-wide worker pool the set calls share, two
of them above the 200 000 frames from which planning goes in parts), the last error is per calling thread, and run_threads itself
reports what its threads raise and names the ones that do not finish."""
import threading
import time

import numpy as np
import pytest

from tests import concurrent_players as cp

ROWS = 12                      # the rows of a batch whose PCM is compared: the first that have samples
MIN_SAMPLES = 25               # tests/test_player_script_host.py's floor: samples that differ by more than 1 LSB


def runs():
    """The batches of every run of the GPU module, as (kind, k, count)."""
    yield "the pipeline", [(kind, k, None) for kind, k in cp.PIPELINE]
    yield "the walks", [b for walk in cp.WALKS for b in walk]


def first_rows(b):
    """The oracle's PCM of the first ROWS utterances of a batch that have samples: -> (pcm, starts)."""
    from tests import oracle
    pcm, start, _ = oracle.batch_synthesize(cp.SR, b, first=0, count=min(4 * ROWS, len(b["frame_start"]) - 1), threads=8)
    rows = [u for u in range(min(4 * ROWS, len(start) - 1)) if start[u + 1] > start[u]][:ROWS]
    assert len(rows) == ROWS, (b["kind"], b["k"])
    parts = [pcm[start[u]:start[u + 1]] for u in rows]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])])


def test_the_batches_of_a_run_differ():
    """Any two batches of a run: of different kinds they have other utterance counts; of one kind, the oracle's PCM of the first twelve
    rows with samples differs by more than 1 LSB in at least 25 samples in every row (S, I, V, L, W and P).  Kind P has at least 200 000
    frames, and its two batches carry other seeds and other pitches; the trimmed S and I are no multiple of a wavefront; no walk holds a P or a kind twice."""
    from tests import player_script as ps
    for name, batches in runs():
        assert len(set(batches)) == len(batches), name
        by_kind = {}
        for kind, k, count in batches:
            by_kind.setdefault(kind, []).append(cp.batch(kind, k, count))
        sizes = {kind: {len(b["frame_start"]) - 1 for b in bs} for kind, bs in by_kind.items()}
        assert all(len(s) == 1 for s in sizes.values()) and len({min(s) for s in sizes.values()}) == len(sizes), (name, sizes)
        for kind, bs in by_kind.items():
            pcm = [first_rows(b) for b in bs]
            weakest = None
            for i in range(len(bs)):
                for j in range(i + 1, len(bs)):
                    d = ps.rows_differing(*pcm[i], *pcm[j])
                    assert len(d) == ROWS and d.min() >= MIN_SAMPLES, (name, kind, bs[i]["k"], bs[j]["k"], d)
                    weakest = int(d.min()) if weakest is None else min(weakest, int(d.min()))
            print("%s, kind %s: %d batches, the weakest row of any pair differs in %s samples" % (name, kind, len(bs), weakest))
    p = [cp.batch("P", k) for kind, k in cp.PIPELINE if kind == "P"]
    assert len(p) == 2 and all(len(b["min"]) >= cp.PART_FRAMES for b in p) and not np.array_equal(p[0]["seeds"], p[1]["seeds"])
    assert not (p[0]["frames"][:, 0] == p[1]["frames"][:, 0])[p[0]["isnull"] == 0].any()      # (no real frame of the two has one pitch)
    assert abs(cp.PIPELINE.index(("P", 3)) - cp.PIPELINE.index(("P", 4))) == 1
    assert all(n % 64 for n in cp.SMALL.values())
    for walk in cp.WALKS:
        assert len({kind for kind, _, _ in walk}) == len(walk) == 4 and all(kind != "P" for kind, _, _ in walk)


def test_the_wild_batch_holds_every_class():
    """Kind W holds utterances of every class the routing knows, by the classification the planning views report (speechPlayer_frameFacts'
    flags over speechPlayer_planDirect's fade ends: tests/player_script.py, utterance_classes), NaN holds and NULL frames among them."""
    from tests import player_script as ps
    for k in sorted({k for _, batches in runs() for kind, k, _ in batches if kind == "W"} | {0}):
        b = cp.batch("W", k)
        counts = ps.class_counts(b)
        print("W %d: %s" % (k, counts))
        assert all(counts[c] > 0 for c in ps.CLASSES) and sum(counts.values()) == cp.COUNTS["W"], (k, counts)
        real = b["isnull"] == 0
        assert np.isnan(b["frames"][real]).any() and (~real).any()


def view_jobs():
    """Per thread the batches whose planning views it takes; threads 0 and 1 begin with a P-sized one each, at the same time."""
    from tests import player_script as ps
    w = cp.batch("W", 2)
    eligible_w = (ps.utterance_classes(w) == 2).astype(np.uint8)
    return [[(cp.batch("P", 3), None), (cp.batch("S", 0), None)],
            [(cp.batch("P", 4), None), (w, eligible_w)],
            [(cp.batch("I", 1), None), (cp.batch("L", 6), None), (cp.batch("S", 7), None)],
            [(w, eligible_w), (cp.batch("I", 8), None), (cp.batch("L", 11), None)]]


@pytest.mark.parametrize("plan_threads", [None, "3"])
def test_planning_views_from_four_threads(monkeypatch, plan_threads):
    """Four threads take speechPlayer_planTracks, planTrackKinds, planDirect and planTimeline on batches of their own -- two of 395 000
    frames at the same time (asserted by their recorded times), planned in parts on the pool the other threads' sections share -- while a fifth takes
    speechPlayer_ipa_records, speechPlayer_ipa_pack at two sample rates and speechPlayer_ipa_labels: every output array equals, byte
    for byte, the one the same call gives alone.  Under the default SPEECHPLAYER_PLAN_THREADS and under 3 (set before any thread runs:
    the planner reads it per call)."""
    if plan_threads is None:
        monkeypatch.delenv("SPEECHPLAYER_PLAN_THREADS", raising=False)
    else:
        monkeypatch.setenv("SPEECHPLAYER_PLAN_THREADS", plan_threads)
    jobs = view_jobs()
    spec = cp.batch("I", 1)["call"]
    t0 = time.perf_counter()
    alone = [[cp.planning_views(b, el) for b, el in job] for job in jobs]
    alone_producer = cp.producer_views(spec)
    sequential = time.perf_counter() - t0
    run = cp.Run()
    spans = {}

    def planner(t):
        def go():
            out = []
            run.meet("start", len(jobs) + 1)
            for i, (b, el) in enumerate(jobs[t]):
                a = time.perf_counter()
                out.append(cp.planning_views(b, el))
                spans[t, i] = (a, time.perf_counter())
            return out
        return go

    def producer():
        run.meet("start", len(jobs) + 1)
        return [cp.producer_views(spec) for _ in range(2)]
    t0 = time.perf_counter()
    got = cp.run_threads([("planner %d" % t, planner(t)) for t in range(len(jobs))] + [("producer", producer)], cp.limit_for(sequential), run)
    concurrent = time.perf_counter() - t0
    for t, job in enumerate(jobs):
        for i, (b, _) in enumerate(job):
            assert cp.differing(got["planner %d" % t][i], alone[t][i]) == [], (t, b["kind"], b["k"])
    for views in got["producer"]:
        assert cp.differing(views, alone_producer) == []
    assert cp.overlaps(spans[0, 0], spans[1, 0]), (spans[0, 0], spans[1, 0])      # the two P-sized views were in flight together
    assert alone[0][0]["planTracks"][0] > 0 and alone[0][0]["planTracks"] != alone[1][1]["planTracks"]
    print("SPEECHPLAYER_PLAN_THREADS %s: alone %.2f s, from five threads %.2f s; the two P-sized views %s" % (
        plan_threads or "unset", sequential, concurrent, "overlapped" if cp.overlaps(spans[0, 0], spans[1, 0]) else "did not overlap"))


def test_errors_per_thread():
    """One thread makes refused calls in a loop, each with a message of its own (speechPlayer_planTimeline: frameStart not monotone at
    u), with a call that succeeds now and then; another makes only calls that succeed.  The refusing thread reads the message and code
    of ITS last refusal after every one, and code 0 after its successes; the other reads code 0 and an empty message throughout."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    n, rounds = 40, 300
    good = np.arange(n + 1, dtype=np.int64)
    dur = np.full(n, 5, np.uint32)
    first, length = np.zeros(n, np.int64), np.zeros(n, np.int64)
    run = cp.Run()

    def refusing():
        for r in range(rounds):
            u = r % (n - 1)
            bad = good.copy()
            bad[u + 1] = bad[u] - 1
            if r % 50 == 0:      # (the two loops stay side by side)
                run.meet(("round", r // 50), 2)
            assert L.speechPlayer_planTimeline(n, bad.ctypes.data, dur.ctypes.data, dur.ctypes.data, None, None) == -1
            assert _native.last_error() == "planTimeline: frameStart not monotone at %d" % u and _native.last_error_code() == 1, (r, _native.last_error())
            if r % 7 == 3:
                assert L.speechPlayer_planTimeline(n, good.ctypes.data, dur.ctypes.data, dur.ctypes.data, None, None) == n
                assert _native.last_error_code() == 0, r
        return rounds

    def succeeding():
        f, l = first.copy(), length.copy()
        for r in range(rounds):
            if r % 50 == 0:
                run.meet(("round", r // 50), 2)
            assert L.speechPlayer_planTimeline(n, good.ctypes.data, dur.ctypes.data, dur.ctypes.data, f.ctypes.data, l.ctypes.data) == n
            assert _native.last_error_code() == 0 and _native.last_error() == "", (r, _native.last_error())
        assert len(set(l.tolist())) == 1 and l[0] > 0
        return rounds
    got = cp.run_threads([("refusing", refusing), ("succeeding", succeeding)], 30.0, run)
    assert got == dict(refusing=rounds, succeeding=rounds)


def test_run_threads_reports_and_does_not_hang():
    """run_threads: what the targets return comes back by name; a target that raises is raised again, and a thread waiting for it gives
    up; a target that outlives the limit fails the run by its name within the limit, not after its own sleep."""
    assert cp.run_threads([("a", lambda: 1), ("b", lambda: "two")], 5.0) == dict(a=1, b="two")
    run, never = cp.Run(), threading.Event()

    def waits():
        run.wait(never)
    with pytest.raises(ZeroDivisionError):
        cp.run_threads([("raises", lambda: 1 // 0), ("waits", waits)], 20.0, run)
    assert run.cancel.is_set()
    release = threading.Event()
    t0 = time.monotonic()
    with pytest.raises(cp.StillRunning, match="sleeper") as e:
        cp.run_threads([("sleeper", lambda: release.wait(60.0)), ("quick", lambda: None)], 0.3)
    took = time.monotonic() - t0
    release.set()
    assert "quick" not in str(e.value) and took < 10.0, (str(e.value), took)
    assert cp.limit_for(0.1) == 30.0 and cp.limit_for(4.0) == 80.0
    assert cp.overlaps((0, 2), (1, 3)) and not cp.overlaps((0, 1), (1, 2))
