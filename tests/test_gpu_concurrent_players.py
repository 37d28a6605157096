"""Several BatchPlayers busy at the same time, in one process (needs a GPU): the threads contract of include/speechPlayer_batch.h --
distinct batch objects, signal stages and live handles from distinct threads at once; one batch object by one thread at a time, handed
from thread to thread under the caller's order; the last error per calling thread; "plan_hash_bits" read once per set call -- held the
way bench.py's `pipeline` extra and a serving process use it.  The anchor everywhere is the same batch on a player used alone, computed
first and sequentially in the same test: every fingerprint (tests/concurrent_players.py) and every export of the concurrent pass holds
the lone pass's bytes.  The rest of the suite holds the lone player to the oracle; test_the_anchor_is_the_oracles grounds it here.
MODE_EXACT unless said.  tests/test_concurrent_players_host.py holds the batches to what they claim and the thread skeleton to its word.
Every pass is timed, and a thread that has not finished after max(30 s, 20 x the sequential pass) fails its test by name."""
import collections
import threading
import time

import numpy as np
import pytest

from tests import concurrent_players as cp
from tests.test_gpu_parity import compare
from tests.test_gpu_player_script import same_bits

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
PLAYERS, SETTERS = 4, 3


def device_memory_in_use():
    """Bytes of the device in use, by anybody: the engine allocates beside torch."""
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


def report(name, sequential, concurrent, peak, more=""):
    print("%s: sequential pass %.2f s, concurrent pass %.2f s, device memory in use at most %.2f GB%s" % (name, sequential, concurrent, peak / 2.0 ** 30, more))


def lone_fingerprint(b, mode=0, routing=True):
    """The batch on a fresh player used alone: -> its fingerprint."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(cp.SR, mode=mode)
    cp.set_batch(bp, b)
    bp.synthesize()
    out = cp.fingerprint(bp, b["kind"], routing=routing)
    bp.close()
    return out


def test_the_anchor_is_the_oracles():
    """Kind W, k = 0, on a player used alone against tests/oracle.batch_synthesize at the usual bar of compare, utterance by utterance;
    starts and index marks exactly."""
    import nvspeechplayer_amd as eng
    from tests import oracle
    b = cp.batch("W", 0)
    exp, exp_start, _ = oracle.batch_synthesize(cp.SR, b, threads=16)
    marks = oracle.batch_last_index(cp.SR, b, threads=16)
    bp = eng.BatchPlayer(cp.SR)
    cp.set_batch(bp, b)
    bp.synthesize()
    pcm, starts = bp.readAll()
    assert np.array_equal(starts, exp_start)
    assert [bp.getLastIndex(u) for u in range(bp.nUtterances)] == marks.tolist()
    flips = sum(compare(pcm[starts[u]:starts[u + 1]], exp[exp_start[u]:exp_start[u + 1]], "W 0 utterance %d" % u) for u in range(len(starts) - 1))
    info = bp.kernelInfo()
    assert info["tracked_utterances"] > 0 and info["direct_utterances"] + info["tracked_utterances"] < bp.nUtterances, info
    print("W 0 alone: %d samples against the oracle, %d one-LSB differences" % (len(exp), flips))
    bp.close()


# ---- 1. the pipeline as bench.py runs it -------------------------------------------------------------------------------------------------

def pipeline(batches, mode):
    """bench.py's pipeline_extra with copy_out and pinned buffers, fingerprints taken where it adds up totalSamples: PLAYERS players,
    SETTERS setter threads that take the next batch, wait for its player (a semaphore per player) and run its set call, and a launcher
    that waits for each batch in order (an event per batch), calls synthesize(wait=False) and readAllAsync into the player's page-locked
    buffer, and retires with one launch in flight.  -> (players, run, targets, fingerprints, set spans, the moment each launch had
    been submitted -- synthesize(wait=False) had returned --, peak memory)."""
    import nvspeechplayer_amd as eng
    n = len(batches)
    bps = [eng.BatchPlayer(cp.SR, mode=mode) for _ in range(PLAYERS)]
    longest = max(int(b["_samples"]) for b in batches if b["kind"] != "P")
    outs = [eng.host_array(longest + 64, np.int16) for _ in range(PLAYERS)]
    ready = [threading.Event() for _ in range(n)]
    free = [threading.Semaphore(1) for _ in range(PLAYERS)]
    set_span, submitted, got = [None] * n, [None] * n, [None] * n
    nxt, lock, run = [0], threading.Lock(), cp.Run()
    peak = [0]

    def setter():
        while True:
            with lock:
                k = nxt[0]; nxt[0] += 1
            if k >= n:
                return
            run.acquire(free[k % PLAYERS])          # the player's previous batch has been synthesised and read
            a = time.perf_counter()
            cp.set_batch(bps[k % PLAYERS], batches[k])
            set_span[k] = (a, time.perf_counter())
            ready[k].set()

    def launcher():
        reads, in_flight = {}, []

        def retire(j):
            bp, kind = bps[j % PLAYERS], batches[j]["kind"]
            bp.wait()
            read = None
            if kind != "P":
                bp.readWait()
                view, starts = reads.pop(j)
                read = (np.array(view), starts)
            got[j] = cp.fingerprint(bp, kind, read)
            peak[0] = max(peak[0], device_memory_in_use())
            free[j % PLAYERS].release()
        for k in range(n):
            run.wait(ready[k])
            bp = bps[k % PLAYERS]
            bp.synthesize(wait=False)
            submitted[k] = time.perf_counter()
            if batches[k]["kind"] != "P":
                reads[k] = bp.readAllAsync(outs[k % PLAYERS])
            in_flight.append(k)
            while len(in_flight) > 1:
                retire(in_flight.pop(0))
        retire(in_flight.pop(0))
    return bps, run, [("setter %d" % i, setter) for i in range(SETTERS)] + [("launcher", launcher)], got, set_span, submitted, peak


def side_by_side(batches, mode):
    """One thread per batch, each with a fresh player: the set calls begin together (a rendezvous), then launch and fingerprint.
    -> (run, targets, set spans by thread name)."""
    import nvspeechplayer_amd as eng
    run, spans = cp.Run(), {}

    def one(name, b):
        def go():
            bp = eng.BatchPlayer(cp.SR, mode=mode)
            run.meet("the players are made", len(batches))
            a = time.perf_counter()
            cp.set_batch(bp, b)
            spans[name] = (a, time.perf_counter())
            bp.synthesize()
            out = cp.fingerprint(bp, b["kind"])
            bp.close()
            return out
        return go
    return run, [("%s %d" % (b["kind"], b["k"]), one("%s %d" % (b["kind"], b["k"]), b)) for b in batches], spans


@pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fast"])
def test_the_pipeline_as_bench_runs_it(mode):
    """Twelve batches in the order S I W P P V L S I W V L through four players, three setter threads and a launcher, as bench.py's
    `pipeline` extra runs them: every batch's fingerprint -- the bytes readAllAsync delivered into the player's page-locked buffer, the
    starts, the index marks, the totals and the routing; for the two P the per-utterance digests -- equals that of the same batch on a
    fresh player used alone, in MODE_EXACT and in MODE_FAST (a launch is deterministic in either).  By the recorded times at least one
    pair of set calls overlapped and at least one launch was submitted while a set call on another player was running -- the moment
    synthesize(wait=False) returned lies strictly inside that set call's span, so the launch was in flight beside it: when the launch
    ended is not observed, and nothing is made of it --: otherwise nothing was proved.
    The two P are neighbours in the run, yet their set calls do not meet there: the second waits for player 0, which retires -- its PCM
    read and compared -- only after the first P is set (profiles/concurrent_players.txt: in no run on an MI355X did they overlap).  So the two P are then set once more
    on two fresh players by two threads that begin together: two set calls above the threshold planning in parts on the one pool, by
    the recorded times side by side, with the lone fingerprints."""
    batches = [cp.batch(kind, k) for kind, k in cp.PIPELINE]
    peak = device_memory_in_use()
    t0 = time.perf_counter()
    want = []
    for b in batches:
        want.append(lone_fingerprint(b, mode))
        peak = max(peak, device_memory_in_use())
    sequential = time.perf_counter() - t0
    batches = [dict(b, _samples=w["totals"][0]) for b, w in zip(batches, want)]
    bps, run, targets, got, set_span, submitted, peak_c = pipeline(batches, mode)
    t0 = time.perf_counter()
    cp.run_threads(targets, cp.limit_for(sequential), run)
    concurrent = time.perf_counter() - t0
    for bp in bps:
        bp.close()
    both = [j for j, b in enumerate(batches) if b["kind"] == "P"]
    run2, targets2, spans2 = side_by_side([batches[j] for j in both], mode)
    t0 = time.perf_counter()
    beside_each_other = cp.run_threads(targets2, cp.limit_for(sequential), run2)
    concurrent += time.perf_counter() - t0
    for j in both:
        name = "P %d" % batches[j]["k"]
        assert cp.differing(beside_each_other[name], want[j]) == [], name
    assert len(both) == 2 and cp.overlaps(*spans2.values()), spans2
    n = len(batches)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if cp.overlaps(set_span[i], set_span[j])]
    beside = [(s, l) for s in range(n) for l in range(n) if s != l and set_span[s][0] < submitted[l] < set_span[s][1]]
    p = [j for j, b in enumerate(batches) if b["kind"] == "P"]
    report("pipeline, mode %d" % mode, sequential, concurrent, max(peak, peak_c[0]),
           "; %d pairs of set calls overlapped (%s), the two P set calls %s; %d launches were submitted inside another player's set call, (set call, launch): %s; set calls of P %s ms; "
           "side by side afterwards %s ms, overlapping" % (
               len(pairs), pairs[:6], "overlapped" if tuple(p) in pairs else "did not overlap", len(beside), beside,
               ["%.1f" % (1e3 * (set_span[j][1] - set_span[j][0])) for j in p], ["%.1f" % (1e3 * (s[1] - s[0])) for s in spans2.values()]))
    for j, b in enumerate(batches):
        assert cp.differing(got[j], want[j]) == [], (j, b["kind"], b["k"])
    assert pairs and beside, (pairs, beside)
    assert all(w["totals"][1] >= cp.PART_FRAMES for w, b in zip(want, batches) if b["kind"] == "P")
    assert want[0]["routing"] != want[2]["routing"] and dict(want[5]["routing"])["lane_pipelined_utterances"] == 70, (want[0]["routing"], want[5]["routing"])


# ---- 2. a thread per player, no coordination ----------------------------------------------------------------------------------------------

def six_exports(bp):
    """Six exports of the resident batch on torch's current stream: an ordered dict of what each returns."""
    import nvspeechplayer_amd as eng
    out = collections.OrderedDict()
    out["pcm, float32, packed"] = bp.pcmTensor(padded=False)
    out["tracks, 3 columns, hop 7 phase 3"] = bp.trackTensor([0, 9, 44], hop=7, phase=3)
    out["spectrogram, nFft 256, 8 mel bands"] = bp.spectrogramTensor(nFft=256, hop=64, bank=eng.melFilterbank(cp.SR, 256, 8))
    out["resampled to 16000 Hz"] = bp.resampledTensor(16000)
    out["filtered, one biquad"] = bp.filteredTensor(eng.biquad("lowpass", cp.SR, 3000.0))
    out["coded, ulaw"] = bp.codedTensor("ulaw")
    return out


def walk(t, want=None, spans=None):
    """Thread t's life: a player and a non-default torch stream of its own, the four batches of cp.WALKS[t], after every launch the
    fingerprint and six exports.  want None: -> what it saw, per batch (fingerprint, exports: device tensors); else every one is
    compared with `want` on the spot and the number of outputs compared comes back."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(cp.SR)
    stream = torch.cuda.Stream(bp.device)
    seen, compared = [], 0
    with torch.cuda.stream(stream):
        assert torch.cuda.current_stream(bp.device).cuda_stream == stream.cuda_stream != 0
        for i, (kind, k, count) in enumerate(cp.WALKS[t]):
            b = cp.batch(kind, k, count)
            a = time.perf_counter()
            cp.set_batch(bp, b)
            bp.synthesize()
            if spans is not None:
                spans.append((a, time.perf_counter()))
            fp, ex = cp.fingerprint(bp, kind), six_exports(bp)
            stream.synchronize()
            if want is None:
                seen.append((fp, ex))
                continue
            assert cp.differing(fp, want[i][0]) == [], (t, kind, k)
            assert list(ex) == list(want[i][1]) and [name for name in ex if not same_bits(ex[name], want[i][1][name])] == [], (t, kind, k)
            compared += len(fp) + len(ex)
    stream.synchronize()
    bp.close()
    return seen if want is None else compared


def test_a_thread_per_player_without_coordination():
    """Six threads, each with a player and a non-default torch stream of its own, walk four batches of different kinds each and read,
    after every launch, the fingerprint and six exports -- pcmTensor (float32, packed), trackTensor (3 columns, hop 7, phase 3),
    spectrogramTensor (nFft 256, 8 mel bands), resampledTensor(16000), filteredTensor (one biquad) and codedTensor("ulaw"): all bytes
    equal the same calls of the same walk on a lone player."""
    import torch
    peak = device_memory_in_use()
    t0 = time.perf_counter()
    want = [walk(t) for t in range(len(cp.WALKS))]
    torch.cuda.synchronize()
    sequential = time.perf_counter() - t0
    peak = max(peak, device_memory_in_use())
    spans = [[] for _ in cp.WALKS]
    t0 = time.perf_counter()
    got = cp.run_threads([("walker %d" % t, lambda t=t: walk(t, want[t], spans[t])) for t in range(len(cp.WALKS))], cp.limit_for(sequential))
    concurrent = time.perf_counter() - t0
    peak = max(peak, device_memory_in_use())
    together = sum(1 for s in range(len(spans)) for t in range(s + 1, len(spans)) for x in spans[s] for y in spans[t] if cp.overlaps(x, y))
    report("a thread per player", sequential, concurrent, peak, "; %d outputs compared; %d pairs of set-and-launch steps of different threads overlapped" % (sum(got.values()), together))
    assert all(v == 4 * (5 + 6) for v in got.values()), got
    assert together > 0
    del want
    torch.cuda.empty_cache()      # (the lone walks' exports: nothing of them stays cached under the tests that follow)


# ---- 3. stages and live handles beside batches ---------------------------------------------------------------------------------------------

CHUNKS = (0, 1, 137, 3000, 777)


def to_bytes(result):
    """A stage's (tensors ..., lengths) as bytes."""
    return tuple(t.cpu().numpy().tobytes() for t in result)


def stage_rounds(seed, run=None, shared=None, rounds=4):
    """Four times over: on a player of its own (never set), a resample -> filter -> code chain and a spectrogram stage of five rows are
    made, planned, pushed three chunks of unequal lengths -- the last ends the rows -- and freed.  Then one more filter stage, `keep`,
    is made and pushed.  -> every output's bytes.  With `run` and `shared` (the concurrent pass; party 0 or 1 by `seed`): once both
    threads have made their last stage -- nobody makes another from then on, so a freed handle names no newer stage -- party 0 makes
    and frees a stage of its own through the C entry, and party 1 is refused, with the documented error, when it presents that handle;
    both then push `keep`, unharmed."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    bp = eng.BatchPlayer(cp.SR)
    dev = "cuda:%d" % bp.device
    stream = torch.cuda.Stream(bp.device)
    n, out = len(CHUNKS), []
    lowpass, mel = eng.biquad("lowpass", 16000, 3000.0), eng.melFilterbank(cp.SR, 256, 8)

    def chunk(rng, shift):
        lens = np.roll(np.array(CHUNKS, np.int64), shift)
        x = torch.from_numpy(rng.uniform(-1.0, 1.0, (n, int(lens.max()))).astype(np.float32)).to(dev)
        return x, lens
    with torch.cuda.stream(stream):
        for r in range(rounds):
            rng = np.random.default_rng(1000 * seed + r)
            chain = eng.SignalChain([bp.resampleStage(n, cp.SR, 16000), bp.filterStage(n, lowpass, tail=3), bp.codeStage(n, "ulaw")])
            spectrogram = bp.spectrogramStage(n, nFft=256, hop=64, bank=mel)
            for push in range(3):
                x, lens = chunk(rng, push + r)
                end = push == 2
                planned = spectrogram.plan(lens, end)
                steps = spectrogram.push((x, lens), end)
                assert steps[-1].numpy().tolist() == planned.tolist(), (seed, r, push)
                out.append(to_bytes(chain.push((x, lens), end)) + to_bytes(steps))
            assert not spectrogram.consumed.any()      # (the last push ended every row)
            for s in chain.stages + [spectrogram]:
                s.close()
        keep = bp.filterStage(n, lowpass)
        victim = bp.codeStage(n, "alaw") if shared is not None and seed == 0 else None
        if shared is not None:
            run.meet("the last stages are made", 2)
            if seed == 0:
                shared["victim"] = victim
                _native.load().speechPlayer_stage_free(victim._h)      # (the object keeps the handle: what a stale reference looks like)
                shared["freed"].set()
            else:
                run.wait(shared["freed"])
                stale = shared["victim"]
                with pytest.raises(ValueError, match="is not a stage"):
                    stale.plan(np.array(CHUNKS, np.int64))
                assert _native.last_error_code() == ERR_ARGUMENT
                with pytest.raises(RuntimeError, match="is not a stage"):
                    _ = stale.consumed
                shared["refused"].set()
            run.wait(shared["refused"])
        x, lens = chunk(np.random.default_rng(77 + seed), 2)
        out.append(to_bytes(keep.push((x, lens), True)))
        keep.close()
        if victim is not None:
            victim._h = None      # (freed above)
    stream.synchronize()
    bp.close()
    return out


def live_pulls(n_handles=130, pull=4096):
    """130 live handles, each with the frames of one cfg2 utterance queued, pulled together with synthesizeMany until all have
    drained: -> the samples of every handle, pull by pull, as bytes."""
    import nvspeechplayer_amd as eng
    b = cp.batch("S", 50, n_handles)
    players = [eng.SpeechPlayer(cp.SR, noiseSeed=int(b["seeds"][u])) for u in range(n_handles)]
    for u, p in enumerate(players):
        for k in range(int(b["frame_start"][u]), int(b["frame_start"][u + 1])):
            p.queueFrameSamples(None if b["isnull"][k] else eng.Frame.from_array(b["frames"][k]), int(b["min"][k]), int(b["fade"][k]), int(b["index"][k]))
    buf = np.zeros((n_handles, pull), np.int16)
    out, total = [], 0
    for _ in range(64):
        counts = eng.SpeechPlayer.synthesizeMany(players, pull, out=buf)
        if not counts.any():
            break
        out.append(b"".join(buf[i, :c].tobytes() for i, c in enumerate(counts)))
        total += int(counts.sum())
    else:
        raise AssertionError("the handles did not drain")
    marks = [p.getLastIndex() for p in players]
    for p in players:
        p.close()
    return out, total, marks


def test_stages_and_live_handles_beside_batches():
    """Two threads create, plan, push and free signal stages on players of their own -- a resample -> filter -> code chain and a
    spectrogram stage over chunks of unequal lengths, four times over: the registry of stages under creation and freeing --, one
    thread pulls 130 live handles with synthesizeMany, and two threads walk batches as in the test above: every output equals the
    sequential run's.  A stage handle freed in one thread is refused with the documented error in the other, whose own stage goes on."""
    import torch
    peak = device_memory_in_use()
    t0 = time.perf_counter()
    want_stage = [stage_rounds(seed) for seed in (0, 1)]
    want_live = live_pulls()
    want_walk = [walk(t) for t in (4, 5)]
    torch.cuda.synchronize()
    sequential = time.perf_counter() - t0
    assert want_stage[0] != want_stage[1] and want_live[1] > 130 * 20000 and len(want_live[0]) > 4, (want_live[1], len(want_live[0]))
    run = cp.Run()
    shared = dict(freed=threading.Event(), refused=threading.Event())
    t0 = time.perf_counter()
    got = cp.run_threads([("stages 0", lambda: stage_rounds(0, run, shared)), ("stages 1", lambda: stage_rounds(1, run, shared)), ("live", live_pulls),
                          ("walker 4", lambda: walk(4, want_walk[0])), ("walker 5", lambda: walk(5, want_walk[1]))], cp.limit_for(sequential), run)
    concurrent = time.perf_counter() - t0
    peak = max(peak, device_memory_in_use())
    report("stages and live handles beside batches", sequential, concurrent, peak, "; %d stage outputs, %d live samples in %d pulls" % (
        sum(len(w) for w in want_stage), want_live[1], len(want_live[0])))
    for seed in (0, 1):
        assert len(got["stages %d" % seed]) == len(want_stage[seed])
        assert [i for i, (g, w) in enumerate(zip(got["stages %d" % seed], want_stage[seed])) if g != w] == [], seed
    assert got["live"][1:] == want_live[1:] and [i for i, (g, w) in enumerate(zip(got["live"][0], want_live[0])) if g != w] == []
    assert got["walker 4"] == got["walker 5"] == 4 * (5 + 6)
    assert shared["refused"].is_set()
    del want_walk
    torch.cuda.empty_cache()


# ---- 4. refusals do not leak ----------------------------------------------------------------------------------------------------------------

def refused_set_calls(bp, i):
    """Two set calls the validation refuses, in turn: -> (the call, what its message says)."""
    w = cp.batch("W", 0)
    if i % 2 == 0:
        start = w["frame_start"].copy()
        start[3] = start[4] + 1
        return (lambda: bp.setUtterances(start, w["frames"], w["min"], w["fade"], w["index"], w["isnull"], w["seeds"])), "set: frameStart not monotone at 3"
    return (lambda: bp.setIpa(["hælou"], clauseType="x", noiseSeed=[1])), "speechPlayer_batch_setIpa: bad batch, text array, voice or clause type"


def test_refusals_do_not_leak():
    """Thread A alternates good batches with refused set calls on its player -- a frameStart that does not ascend; a clause type the
    producer does not know --, thread B sets and launches good batches on its own.  Every good batch on both players has the lone
    fingerprint; after each refusal A reads its own message and code, and its player keeps the batch before: same digest, same
    fingerprint; B reads an empty lastError and code 0 after every step -- also right after A's refusal, which a rendezvous orders
    before B's look."""
    from nvspeechplayer_amd import _native
    import nvspeechplayer_amd as eng
    walks = (cp.WALKS[2], cp.WALKS[3])
    t0 = time.perf_counter()
    want = [[lone_fingerprint(cp.batch(*b)) for b in w] for w in walks]
    sequential = time.perf_counter() - t0
    run = cp.Run()

    def a():
        bp = eng.BatchPlayer(cp.SR)
        for i, b in enumerate(walks[0]):
            cp.set_batch(bp, cp.batch(*b))
            bp.synthesize()
            fp = cp.fingerprint(bp, b[0])
            assert cp.differing(fp, want[0][i]) == [], ("A", b)
            digest = bp.digest(per_utterance=True)
            call, message = refused_set_calls(bp, i)
            with pytest.raises(RuntimeError, match="frameStart not monotone at 3|bad batch, text array, voice or clause type"):
                call()
            assert _native.last_error() == message and _native.last_error_code() == ERR_ARGUMENT, (i, _native.last_error())
            run.meet(("refused", i), 2)
            again = bp.digest(per_utterance=True)
            assert again[0] == digest[0] and again[1].tobytes() == digest[1].tobytes(), ("A", b)
            assert cp.differing(cp.fingerprint(bp, b[0]), fp) == [], ("A", b)
        bp.close()
        return len(walks[0])

    def b_():
        bp = eng.BatchPlayer(cp.SR)

        def clean(where):
            seen = (_native.last_error(), _native.last_error_code())
            assert seen == ("", 0), "B reads %r, code %d, %s" % (seen + (where,))
        for i, b in enumerate(walks[1]):
            cp.set_batch(bp, cp.batch(*b))
            clean("after its set call %d" % i)
            bp.synthesize()
            clean("after its launch %d" % i)
            fp = cp.fingerprint(bp, b[0])
            clean("after its reads %d" % i)
            assert cp.differing(fp, want[1][i]) == [], ("B", b)
            run.meet(("refused", i), 2)
            assert bp.totalSamples == want[1][i]["totals"][0]
            clean("after A's refusal %d" % i)
        bp.close()
        return len(walks[1])
    t0 = time.perf_counter()
    got = cp.run_threads([("A", a), ("B", b_)], cp.limit_for(sequential), run)
    concurrent = time.perf_counter() - t0
    report("refusals do not leak", sequential, concurrent, device_memory_in_use())
    assert got == dict(A=4, B=4)


# ---- 5. plan_hash_bits turned over beside set calls ---------------------------------------------------------------------------------------

def test_plan_hash_bits_turned_over_beside_set_calls():
    """A thread turns "plan_hash_bits" over among 64, 128 and 6 -- at 6 bits shapes collide and go through klatt_verify_shared -- while
    three threads set and launch batches of kinds L, I and S on players of their own: PCM, starts, index marks and totals equal the
    lone player's under the default width (the routing is compared there alone: which width a set call met is not the caller's to
    know).  By the recorded times at least one flip fell inside a set call.  The option is restored whatever happens."""
    import nvspeechplayer_amd as eng
    jobs = [[("L", 60 + i, None) for i in range(3)], [("I", 64 + i, cp.SMALL["I"]) for i in range(3)], [("S", 68 + i, cp.SMALL["S"]) for i in range(3)]]
    t0 = time.perf_counter()
    want = [[lone_fingerprint(cp.batch(*b)) for b in job] for job in jobs]
    sequential = time.perf_counter() - t0
    assert all(dict(w["routing"])["tracked_utterances"] > 0 for w in want[1] + want[2])
    run, done, left, lock = cp.Run(), threading.Event(), [len(jobs)], threading.Lock()
    flips, spans = [], []

    def flipper():
        widths = (64, 128, 6)
        while not done.is_set() and not run.cancel.is_set():
            eng.setGlobalOption("plan_hash_bits", widths[len(flips) % 3])
            flips.append(time.perf_counter())
            done.wait(0.0002)
        return len(flips)

    def worker(t):
        def go():
            try:
                bp = eng.BatchPlayer(cp.SR)
                for i, b in enumerate(jobs[t]):
                    a = time.perf_counter()
                    cp.set_batch(bp, cp.batch(*b))
                    spans.append((a, time.perf_counter()))
                    bp.synthesize()
                    fp = cp.fingerprint(bp, b[0], routing=False)
                    assert cp.differing(fp, {key: v for key, v in want[t][i].items() if key != "routing"}) == [], (t, b)
                bp.close()
                return len(jobs[t])
            finally:
                with lock:
                    left[0] -= 1
                    if left[0] == 0:
                        done.set()
        return go
    try:
        t0 = time.perf_counter()
        got = cp.run_threads([("flipper", flipper)] + [("worker %s" % jobs[t][0][0], worker(t)) for t in range(len(jobs))], cp.limit_for(sequential), run)
        concurrent = time.perf_counter() - t0
    finally:
        done.set()
        eng.setGlobalOption("plan_hash_bits", 128)
    inside = sum(1 for f in flips for s in spans if s[0] < f < s[1])
    report("plan_hash_bits turned over", sequential, concurrent, device_memory_in_use(), "; %d flips, %d of them inside a set call" % (got["flipper"], inside))
    assert inside > 0 and all(got["worker %s" % jobs[t][0][0]] == 3 for t in range(len(jobs)))
    again = lone_fingerprint(cp.batch(*jobs[1][0]))
    assert cp.differing(again, want[1][0]) == []      # (the default width is back: the routing too)
