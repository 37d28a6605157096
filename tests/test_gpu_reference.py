"""The HIP engine against the compiled reference on fuzzed call sequences.  Needs a GPU.

The comparand is the reference itself -- oracle/_ref/libspeechPlayer_ref.so, compiled from the reference's checkout by build()
(tests/reference.py) -- where that library is in the tree, else the CPU oracle, which tests/test_reference_pin.py holds to the
same recorded answers sample by sample.  Every test prints which one it had.

Inputs: scenarios.fuzz_sequence, the seeds 0 .. N-1 of the plain and of the extreme variant (a subset of what the CPU pin
plays): purges anywhere (test_the_sequences_hold_every_kind shows from the frame state machine's own arithmetic that a purge on
the first sample of a fade, on an event sample, on a drained handle and a pull boundary inside a purge's fade all occur), pulls
on either side of every hand-over size, frames queued onto drained handles, six sample rates; the extreme variant with negative
bandwidths, overflowing coefficients, +-inf, clipping gains, formants beyond Nyquist and zero / denormal N0 frequencies.

Bar: the project's own -- test_gpu_parity.compare: identical call lengths and marks, <= 1 LSB, <= 5 one-LSB differences per
million samples, RMS < 1e-5 of full scale -- in MODE_EXACT and MODE_FAST.

Admission.  The device's exp / cos differ from glibc's in the last place on 4-31 % of arguments, and an unstable or nearly
cancelling filter amplifies that without bound, so the bar cannot hold for EVERY extreme input, through no fault of a kernel.
Which sequences are held to it is decided on the CPU from the comparand alone, never from the engine's output
(scenarios.admitted): the sequence is played a second time with every non-zero frequency and bandwidth moved one place up, and
is admitted iff the PCM stays identical.  Every test asserts that no plain sequence and at most 15 % of the extreme ones are
left out; those are still run for call lengths, marks and "no sample beyond +-32000".  Measured over the CPU pin's 400 + 400
sequences: 0 plain, 32 extreme (8 %) left out; in the tests here: 0 of 48 plain and 2 of 48 extreme single sequences, 0 of 48
and 3 of 48 of the sequences regrouped for common pulls, 0 of 1251 plain and 91 of 1218 extreme (7.5 %) of the batches' pieces.

Measured on an MI355X against the compiled reference, per test and mode: one handle at a time 7.79 M samples compared, pulled
together 6.81 M, batches 12.71 M; 0 samples differ by one LSB in every test that passed.  Found: with "direct" 2, and with
"direct" 1 under a track budget of 1 MB, MODE_FAST missed the bar on ONE piece (fuzz_extreme_0036_piece00, RMS 0.0263 of full
scale: one sample of +32000 for -32000) -- see test_growing_pole_after_silence; MODE_EXACT and every other path held it.
"""
import functools
import os

import numpy as np
import pytest

from tests import oracle, reference, scenarios
from tests.test_gpu_parity import compare, play_engine

pytestmark = pytest.mark.gpu

N_LIVE = 48         # seeds 0 .. N_LIVE-1 of each variant through live handles
N_BATCH = 40        # seeds 0 .. N_BATCH-1 of each variant as batches
MAX_LEFT_OUT = 0.15


def comparand():
    if os.path.exists(reference.LIB_PATH):
        return "the compiled reference", reference.RefPlayer
    return "the oracle", oracle.OraclePlayer


@functools.lru_cache(maxsize=None)
def fuzz(n):
    return [scenarios.fuzz_sequence(s, extreme) for extreme in (False, True) for s in range(n)]


def is_extreme(scn):
    return "extreme" in scn.name


@functools.lru_cache(maxsize=None)
def single_cases():
    """(sequence, admitted, PCM per call, marks) of every live sequence, from the comparand."""
    _, player = comparand()
    return [(scn,) + scenarios.admitted(scn, player) for scn in fuzz(N_LIVE)]


@functools.lru_cache(maxsize=None)
def grouped_cases():
    """synthesizeMany gives every handle of a pull the same sample count, so the sequences of one sample rate are regrouped: the
    k-th queue call of every member (its own frame, durations, user index and purge) at the place of the first member's k-th,
    the first member's pulls for all, and a drain as pulls of 8192 until every member came back short (a drained member is pulled
    on: frame.cpp:42 counts those calls too).  The comparand is played in that lock-step; each member's calls as they came out are
    a sequence of its own, admitted or not like any other.  -> [(sample rate, [(sequence, admitted, PCM per call, marks)])]"""
    _, player = comparand()
    by_sr = {}
    for scn in fuzz(N_LIVE):
        by_sr.setdefault(scn.sr, []).append(scn)
    out = []
    for sr, members in sorted(by_sr.items()):
        qs = [[op for op in s.ops if op[0] == "q"] for s in members]
        n_q = min(len(x) for x in qs)
        players = [player(sr, seed=s.seed) for s in members]
        ops = [[] for _ in members]; pcm = [[] for _ in members]; marks = [[] for _ in members]

        def pull(n):
            longest = 0
            for j, p in enumerate(players):
                x = p.synthesize(n)
                ops[j].append(("s", n)); pcm[j].append(x); marks[j].append(p.last_index())
                longest = max(longest, len(x))
            return longest
        k = 0
        for op in members[0].ops:
            if op[0] == "q":
                if k == n_q:
                    break
                for j, p in enumerate(players):
                    p.queue(*qs[j][k][1:]); ops[j].append(qs[j][k])
                k += 1
            elif op[0] == "s":
                pull(op[1])
            else:
                while pull(8192) == 8192:
                    pass
        while pull(8192) == 8192:
            pass
        cases = []
        for j, s in enumerate(members):
            players[j].close()
            scn = scenarios.Scenario(s.name + "_grouped", ops[j], sr=sr, seed=s.seed)
            again, _ = scenarios.play(scenarios.nudged(scn), player(sr, seed=s.seed))
            cases.append((scn, all(np.array_equal(a, b) for a, b in zip(pcm[j], again)), pcm[j], marks[j]))
        out.append((sr, cases))
    return out


class Tally:
    def __init__(self, what):
        self.what, self.samples, self.flips, self.left_out, self.n = what, 0, 0, {False: 0, True: 0}, {False: 0, True: 0}

    def check(self, scn, admitted, got_pcm, got_marks, exp_pcm, exp_marks):
        assert [len(x) for x in got_pcm] == [len(x) for x in exp_pcm], (self.what, scn.name)
        assert list(got_marks) == list(exp_marks), (self.what, scn.name)
        got = np.concatenate(got_pcm) if got_pcm else np.zeros(0, np.int16)
        exp = np.concatenate(exp_pcm) if exp_pcm else np.zeros(0, np.int16)
        self.n[is_extreme(scn)] += 1
        if admitted:
            self.flips += compare(got, exp, "%s %s" % (self.what, scn.name))
            self.samples += len(exp)
        else:
            self.left_out[is_extreme(scn)] += 1
            assert len(got) == 0 or np.abs(got.astype(np.int32)).max() <= 32000, (self.what, scn.name)

    def finish(self):
        print("%s against %s: %d samples compared, %d differ by one LSB; left out %d of %d plain and %d of %d extreme sequences"
              % (self.what, comparand()[0], self.samples, self.flips, self.left_out[False], self.n[False], self.left_out[True], self.n[True]))
        assert self.left_out[False] == 0
        assert self.left_out[True] <= MAX_LEFT_OUT * self.n[True]
        assert self.samples > 0


def test_the_sequences_hold_every_kind():
    """From the sequences' own arithmetic (scenarios.trace_sequence: the sample counter of frame.cpp:41-115, whose call lengths
    the other tests check against the comparand's): every kind of purge and, among the admitted sequences, every extreme kind."""
    for what, cases in (("single", single_cases()), ("grouped", [c for _, g in grouped_cases() for c in g])):
        total = dict.fromkeys(scenarios.PURGE_KINDS, 0)
        for scn, _, pcm, _ in cases:
            calls, kinds = scenarios.trace_sequence(scn)
            assert calls == [len(x) for x in pcm], scn.name
            for k, v in kinds.items():
                total[k] += v
        print("%s sequences, purges by kind: %s" % (what, total))
        assert all(total.values()), (what, total)
    kinds = set().union(*(scn.kinds for scn, ok, _, _ in single_cases() if ok and is_extreme(scn)))
    assert kinds == set(scenarios.EXTREME_KINDS), kinds
    by_name = {s.name: s for s in fuzz(N_LIVE)}
    kinds = set().union(*(by_name[scn.name[:-len("_grouped")]].kinds for _, g in grouped_cases() for scn, ok, _, _ in g if ok and is_extreme(scn)))
    assert kinds == set(scenarios.EXTREME_KINDS), kinds
    assert {sr for sr, _ in grouped_cases()} == set(scenarios.FUZZ_RATES)


@pytest.mark.parametrize("mode", [0, 1])
def test_fuzzed_sequences_one_handle_at_a_time(mode):
    """Every sequence through the five reference entry points on a handle of its own, default kernel, call by call."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    tally = Tally("one handle at a time, mode %d" % mode)
    try:
        assert L.speechPlayer_setGlobalOption(b"live_mode", mode) == 0
        for scn, ok, exp_pcm, exp_marks in single_cases():
            got_pcm, got_marks = play_engine(scn)
            tally.check(scn, ok, got_pcm, got_marks, exp_pcm, exp_marks)
    finally:
        L.speechPlayer_setGlobalOption(b"live_mode", 0)
    tally.finish()


def queue_runs(group_ops, a, b):
    """Queue calls a .. b-1 (the same places in every member's list) as runs that one bulk call can take: a purge only on a run's first frame."""
    runs, start = [], a
    for i in range(a + 1, b):
        if any(ops[i][5] for ops in group_ops):
            runs.append((start, i)); start = i
    runs.append((start, b))
    return runs


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("alone,layout,bulk", [(1536, 1, False), (1, 1, False), ("alternate", 1, True), (1, 0, False), (1, "alternate", True)])
def test_fuzzed_sequences_pulled_together(alone, layout, bulk, mode):
    """The handles of one sample rate advanced together by synthesizeMany, in a wavefront each ("live_alone" 1536), sharing
    wavefronts (1) or changing between the two from pull to pull; on the stage-parallel stream kernel ("live_layout" 1), the
    lane kernel (0) or changing from pull to pull; frames queued call by call or through LiveGroup.queue (runs of frames per call)."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    tally = Tally("pulled together, live_alone %s live_layout %s %s, mode %d" % (alone, layout, "bulk queue" if bulk else "queue calls", mode))
    try:
        assert L.speechPlayer_setGlobalOption(b"live_mode", mode) == 0
        assert L.speechPlayer_setGlobalOption(b"live_alone", 1536 if alone == "alternate" else alone) == 0
        assert L.speechPlayer_setGlobalOption(b"live_layout", 1 if layout == "alternate" else layout) == 0
        pulls = 0
        for sr, cases in grouped_cases():
            group_ops = [scn.ops for scn, _, _, _ in cases]
            n = len(cases)
            players = [eng.SpeechPlayer(sr, noiseSeed=scn.seed) for scn, _, _, _ in cases]
            grp = eng.LiveGroup(players)
            got = [[] for _ in cases]; marks = [[] for _ in cases]
            i, n_ops = 0, len(group_ops[0])
            while i < n_ops:
                if group_ops[0][i][0] == "q":
                    j = i
                    while j < n_ops and group_ops[0][j][0] == "q":
                        j += 1
                    if bulk:
                        for a, b in queue_runs(group_ops, i, j):
                            rows = [ops[k] for ops in group_ops for k in range(a, b)]
                            grp.queue(np.arange(n + 1) * (b - a), np.array([np.zeros(47) if r[1] is None else r[1] for r in rows]),
                                      [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows], [r[1] is None for r in rows],
                                      [ops[a][5] for ops in group_ops])
                    else:
                        for k in range(i, j):
                            for p, ops in zip(players, group_ops):
                                op = ops[k]
                                p.queueFrameSamples(None if op[1] is None else eng.Frame.from_array(op[1]), op[2], op[3], op[4], op[5])
                    i = j
                    continue
                if alone == "alternate":
                    assert L.speechPlayer_setGlobalOption(b"live_alone", (1536, 1)[pulls % 2]) == 0
                if layout == "alternate":
                    assert L.speechPlayer_setGlobalOption(b"live_layout", pulls % 2) == 0
                pulls += 1
                want = group_ops[0][i][1]
                bufs = eng.SpeechPlayer.synthesizeMany(players, want)
                for k, b in enumerate(bufs):
                    got[k].append(np.zeros(0, np.int16) if b is None else np.frombuffer(b, dtype=np.int16)[:b.length].copy())
                    marks[k].append(players[k].getLastIndex())
                i += 1
            for p in players:
                p.close()
            for k, (scn, ok, exp_pcm, exp_marks) in enumerate(cases):
                tally.check(scn, ok, got[k], marks[k], exp_pcm, exp_marks)
    finally:
        L.speechPlayer_setGlobalOption(b"live_mode", 0)
        L.speechPlayer_setGlobalOption(b"live_layout", 1)
        L.speechPlayer_setGlobalOption(b"live_alone", 1536)
    tally.finish()


PIECE = 6           # queue calls per utterance of a batch


@functools.lru_cache(maxsize=None)
def batch_cases():
    """The frame lists of the sequences with the purges dropped, one batch per sample rate.  An utterance is PIECE consecutive
    queue calls of a sequence (random_batch's own utterances have 1 to 8), not the whole list: one NaN or infinite parameter keeps
    an utterance off the tracks, the direct stages and the quiet kernels (the planner's classification), and every whole list holds
    some.  Each piece is admitted or not on its own.  -> [(sample rate, batch dict, [(sequence, admitted, [PCM], [mark])])]"""
    _, player = comparand()
    by_sr = {}
    for scn in fuzz(N_BATCH):
        by_sr.setdefault(scn.sr, []).append(scn)
    out = []
    for sr, members in sorted(by_sr.items()):
        pieces = []
        for s in members:
            qs = [op[:5] + (False,) for op in s.ops if op[0] == "q"]
            for i in range(0, len(qs), PIECE):
                pieces.append(scenarios.Scenario("%s_piece%02d" % (s.name, i // PIECE), qs[i:i + PIECE] + [("drain",)], sr=sr,
                                                 seed=(s.seed + i) & 0xFFFFFFFF, batchable=True))
        parts = [p.frames() for p in pieces]
        batch = dict(frames=np.concatenate([p[0] for p in parts]), min=np.concatenate([p[1] for p in parts]),
                     fade=np.concatenate([p[2] for p in parts]), index=np.concatenate([p[3] for p in parts]),
                     isnull=np.concatenate([p[4] for p in parts]),
                     frame_start=np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(np.int64),
                     seeds=np.array([p.seed for p in pieces], np.uint32))
        out.append((sr, batch, [(scn,) + scenarios.admitted(scn, player) for scn in pieces]))
    return out


BATCH_OPTIONS = [dict(layout=-1), dict(layout=2), dict(layout=1), dict(layout=0), dict(tracks=0, direct=2), dict(tracks=0, direct=0),
                 dict(tracks=1, direct=1, track_budget_mb=1)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("options", BATCH_OPTIONS, ids=lambda o: "-".join("%s%s" % kv for kv in o.items()))
def test_fuzzed_frame_lists_as_batches(options, mode):
    """The same frame lists as ragged batches at their sample rates: chosen layout, lane-pipelined, stage-parallel and lane kernels;
    the noisy utterances on the direct stages, on the stages with the frame state machine, and with a track budget that runs out.
    Sequences without any noise source (one in four) and without a nasal branch (one in eight) are among them."""
    import nvspeechplayer_amd as eng
    tally = Tally("batches %s, mode %d" % (options, mode))
    info = {}
    for sr, batch, cases in batch_cases():
        bp = eng.BatchPlayer(sr, mode=mode)
        for name, value in options.items():
            bp.setOption(name, value)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], batch["seeds"])
        bp.synthesize()
        for k, v in bp.kernelInfo().items():
            if k.endswith("_utterances"):
                info[k] = info.get(k, 0) + v
        for u, (scn, ok, exp_pcm, exp_marks) in enumerate(cases):
            tally.check(scn, ok, [bp.read(u)], [bp.getLastIndex(u)], exp_pcm, exp_marks)
        bp.close()
    print("planner: %s" % info)
    tally.finish()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("options", [dict(tracks=0, direct=2), dict(tracks=1, direct=1, track_budget_mb=1), dict()], ids=lambda o: "-".join("%s%s" % kv for kv in o.items()) or "defaults")
def test_growing_pole_after_silence(options, mode):
    """The reduced case of what this file found (scenarios.py, "growing_pole_after_silence"): with "direct" 2 the parent put it on the
    direct stages, whose MODE_FAST gains advance by increments and end a silence's fade 1e-17 beside 0; the pole pair that grows
    after the silence turned that into a sample of +32000 for -32000 (RMS 0.026 of full scale on the piece it came from).  The
    planner now keeps a list with a negative bandwidth off the direct stages (klatt_plan.h)."""
    import nvspeechplayer_amd as eng
    scn = next(s for s in scenarios.build_scenarios(scenarios.Ref()) if s.name == "growing_pole_after_silence")
    _, player = comparand()
    fr, m, f, ix, nu = scn.frames()
    n = 70                                                  # more than a wavefront of copies, noise seeds of their own
    bp = eng.BatchPlayer(scn.sr, mode=mode)
    for k, v in options.items():
        bp.setOption(k, v)
    bp.setUtterances(np.arange(n + 1) * len(m), np.tile(fr, (n, 1)), np.tile(m, n), np.tile(f, n), np.tile(ix, n), np.tile(nu, n),
                     [scn.seed + 1000 * u for u in range(n)])
    assert bp.kernelInfo()["direct_utterances"] == 0
    bp.synthesize()
    tally = Tally("growing pole after silence, %s, mode %d" % (options, mode))
    for u in range(n):
        copy = scenarios.Scenario("extreme copy %d" % u, scn.ops, sr=scn.sr, seed=scn.seed + 1000 * u)
        ok, exp_pcm, exp_marks = scenarios.admitted(copy, player)
        assert ok or u > 0                                  # (copy 0 is the scenario itself)
        tally.check(copy, ok, [bp.read(u)], [bp.getLastIndex(u)], exp_pcm, exp_marks)
    bp.close()
    tally.finish()
