"""Parity of the HIP engine (through its C-ABI) against the CPU oracle.  Needs a GPU.

Bar (BASELINE.json north_star): per-sample RMS error < 1e-5 of full scale (int16/32768).
MODE_EXACT computes in IEEE double with the reference's operation order, so these tests
ask for more: identical int16 PCM, identical call lengths and index marks.  The only
tolerated difference is a last-place difference between the device's exp/cos/sin and
glibc's, which can move a sample by one LSB when a value sits on a truncation boundary;
the tests therefore allow at most MAX_FLIPS one-LSB differences per million samples
and print what they saw.
"""
import os
import numpy as np
import pytest

from tests import oracle, scenarios
from tests.scenarios import random_batch

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5          # north_star tolerance, full-scale units
MAX_FLIPS_PER_M = 5     # one-LSB differences tolerated per million samples in MODE_EXACT


def compare(got, exp, name):
    assert len(got) == len(exp), "%s: length %d != %d" % (name, len(got), len(exp))
    if len(exp) == 0:
        return 0
    d = got.astype(np.int32) - exp.astype(np.int32)
    nbad = int(np.count_nonzero(d))
    rms = float(np.sqrt(np.mean((d / 32768.0) ** 2)))
    mx = int(np.abs(d).max())
    assert rms < RMS_TOL, "%s: rms %.3g" % (name, rms)
    assert mx <= 1, "%s: max |diff| %d LSB (%d samples differ)" % (name, mx, nbad)
    assert nbad <= max(1, MAX_FLIPS_PER_M * len(exp) // 1000000 + 1), "%s: %d samples differ" % (name, nbad)
    return nbad


@pytest.fixture(scope="module")
def ref():
    return scenarios.Ref()


@pytest.fixture(scope="module")
def all_scenarios(ref):
    return scenarios.build_scenarios(ref)


def play_engine(scn):
    import nvspeechplayer_amd as eng
    p = eng.SpeechPlayer(scn.sr, noiseSeed=scn.seed)
    pcm, marks = [], []

    def synth(n):
        buf = p.synthesize(n)
        if buf is None:
            return np.zeros(0, np.int16)
        return np.frombuffer(buf, dtype=np.int16)[:buf.length].copy()

    for op in scn.ops:
        if op[0] == "q":
            fr = None if op[1] is None else eng.Frame.from_array(op[1])
            p.queueFrameSamples(fr, op[2], op[3], op[4], op[5])
        elif op[0] == "s":
            pcm.append(synth(op[1])); marks.append(p.getLastIndex())
        else:
            parts = []
            while True:
                x = synth(8192)
                parts.append(x)
                if len(x) < 8192:
                    break
            pcm.append(np.concatenate(parts)); marks.append(p.getLastIndex())
    p.close()
    return pcm, marks


def test_streaming_abi_scenarios(all_scenarios):
    """The five reference entry points, call by call: chunked pulls, purge, marks, drain/resume."""
    names = ("cfg0_a_1s", "stream_chunks", "purge_resume", "vowelchart_pairs", "hannah_vibrato", "nan_hold",
             "duration_edges", "ipa_l0_16k")
    flips = 0
    for scn in all_scenarios:
        if scn.name not in names and not scn.name.endswith("_s10_c0_p100_i05"):
            continue
        exp_pcm, exp_marks = scenarios.play_oracle(scn)
        got_pcm, got_marks = play_engine(scn)
        assert [len(x) for x in got_pcm] == [len(x) for x in exp_pcm], scn.name
        assert got_marks == exp_marks, scn.name
        flips += compare(np.concatenate(got_pcm), np.concatenate(exp_pcm), scn.name)
    print("streaming scenarios: %d one-LSB differences in total" % flips)


def test_live_handles_in_mode_fast(all_scenarios, ref):
    """speechPlayer_setGlobalOption("live_mode", 1): handles created afterwards run the stream kernels' MODE_FAST instantiations (fused
    multiply-adds in the filters).  Every scenario through the five reference entry points, and 100 unrelated handles pulled together
    under both wavefront policies: call lengths and index marks exactly, PCM to MODE_FAST's bar (<= 1 LSB, <= 5 one-LSB differences per
    million samples, RMS < 1e-5 of full scale); a handle created after the option went back is bit-exact again."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    try:
        assert L.speechPlayer_setGlobalOption(b"live_mode", 2) != 0 and L.speechPlayer_setGlobalOption(b"live_mode", 1) == 0
        flips = 0
        for scn in all_scenarios:
            exp_pcm, exp_marks = scenarios.play_oracle(scn)
            got_pcm, got_marks = play_engine(scn)
            assert [len(x) for x in got_pcm] == [len(x) for x in exp_pcm], scn.name
            assert got_marks == exp_marks, scn.name
            flips += compare(np.concatenate(got_pcm), np.concatenate(exp_pcm), scn.name)
        rng = np.random.default_rng(41)
        cases = [ref.ipa_case(int(i)) for i in rng.integers(0, len(ref.ipa_meta), size=100)]
        for alone in (1536, 1):
            assert L.speechPlayer_setGlobalOption(b"live_alone", alone) == 0
            players = [eng.SpeechPlayer(22050, noiseSeed=70 + k) for k in range(len(cases))]
            oracles = [oracle.OraclePlayer(22050, seed=70 + k) for k in range(len(cases))]
            for k, case in enumerate(cases):
                for j, (fr, m, f) in enumerate(case):
                    players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, j)
                    oracles[k].queue(fr, m, f, j)
            got = [[] for _ in cases]; exp = [[] for _ in cases]
            for n in (5000, 33, 8192, 8192, 8192, 8192):
                bufs = eng.SpeechPlayer.synthesizeMany(players, n)
                for k, b in enumerate(bufs):
                    e = oracles[k].synthesize(n)
                    g = np.zeros(0, np.int16) if b is None else np.frombuffer(b, dtype=np.int16)[:b.length].copy()
                    assert len(g) == len(e) and players[k].getLastIndex() == oracles[k].last_index(), (alone, k)
                    got[k].append(g); exp[k].append(e)
            for k in range(len(cases)):
                flips += compare(np.concatenate(got[k]), np.concatenate(exp[k]), "fast live handle %d" % k)
                players[k].close()
        print("MODE_FAST live handles: %d one-LSB differences in total" % flips)
        assert L.speechPlayer_setGlobalOption(b"live_mode", 0) == 0
        scn = next(s for s in all_scenarios if s.name == "stream_chunks")
        exp_pcm, _ = scenarios.play_oracle(scn)
        got_pcm, _ = play_engine(scn)
        assert np.array_equal(np.concatenate(got_pcm), np.concatenate(exp_pcm))
    finally:
        L.speechPlayer_setGlobalOption(b"live_mode", 0)
        L.speechPlayer_setGlobalOption(b"live_alone", 1536)


def make_batch(sel):
    frames, mins, fades, idx, nul, start, seeds = [], [], [], [], [], [0], []
    for s in sel:
        fr, m, f, ix, nu = s.frames()
        frames.append(fr); mins.append(m); fades.append(f); idx.append(ix); nul.append(nu)
        start.append(start[-1] + len(m)); seeds.append(s.seed)
    return dict(frames=np.concatenate(frames), min=np.concatenate(mins), fade=np.concatenate(fades),
                index=np.concatenate(idx), isnull=np.concatenate(nul), frame_start=np.array(start, np.int64),
                seeds=np.array(seeds, np.uint32))


@pytest.mark.parametrize("layout", [-1, 2, 1, 0])
@pytest.mark.parametrize("mode", [0, 1])
def test_batch_all_scenarios(all_scenarios, mode, layout):
    """Every batchable scenario (vowels, all sampleIpa cases, vibrato, NaN hold, duration edges)
    as ONE ragged batch through speechPlayer_batch_*; each utterance must equal a fresh oracle player.
    mode 0 = MODE_EXACT, mode 1 = MODE_FAST (fused multiply-adds, straight-line exp/cos): same bar.
    layout 1 = stage-parallel workgroups (klatt_systolic.h), 0 = one wavefront per 64 utterances,
    2 = lane-pipelined workgroups (klatt_lanepipe.h) for the quiet, nasal-free utterances."""
    import nvspeechplayer_amd as eng
    sel = [s for s in all_scenarios if s.batchable and s.sr == 22050]
    batch = make_batch(sel)
    k = np.arange(len(batch["index"]))
    batch["index"] = np.where((batch["index"] == -1) & (k % 5 == 2), (k % 997).astype(np.int32), batch["index"]).astype(np.int32)   # marks on frames that had none
    bp = eng.BatchPlayer(22050, mode=mode, layout=layout)
    bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                     batch["isnull"], batch["seeds"])
    exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=4)
    assert bp.totalSamples == total
    bp.synthesize()
    got, got_start = bp.readAll()
    assert np.array_equal(got_start, exp_start)
    flips = 0
    for i, s in enumerate(sel):
        flips += compare(got[got_start[i]:got_start[i + 1]], exp[exp_start[i]:exp_start[i + 1]], s.name)
        assert np.array_equal(bp.read(i), got[got_start[i]:got_start[i + 1]])
    print("mode %d layout %d: batch of %d utterances, %d samples: %d one-LSB differences" % (mode, layout, len(sel), total, flips))
    # index marks (reference src/frame.cpp:69, :117-119) against the oracle's frame state machine (the scenarios carry real marks)
    assert (batch["index"] != -1).any()
    assert [bp.getLastIndex(i) for i in range(len(sel))] == oracle.batch_last_index(22050, batch, threads=4).tolist()
    # unsorted lane packing gives the same PCM
    bp.setOption("sort", 0)
    bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                     batch["isnull"], batch["seeds"])
    bp.synthesize()
    got2, _ = bp.readAll()
    assert np.array_equal(got, got2)
    bp.close()


@pytest.mark.parametrize("layout", [2, 1, 0])
def test_batch_edge_shapes(ref, layout):
    """Empty batch, empty utterances, a single utterance, 65 utterances (one lane in the 2nd wavefront)."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050, layout=layout)
    bp.setUtterances(np.array([0]), np.zeros((0, 47)), [], [])
    bp.synthesize()
    assert bp.totalSamples == 0
    fa = scenarios.vowel_frame(ref, "a", 120.0)
    # utterances 0 and 2 are empty
    bp.setUtterances(np.array([0, 0, 2, 2]), np.stack([fa, fa]), [300, 10], [40, 10], None, [0, 1], [5, 6, 7])
    bp.synthesize()
    assert bp.utteranceSamples(0) == 0 and bp.utteranceSamples(2) == 0
    assert len(bp.read(0)) == 0 and len(bp.read(2)) == 0
    p = oracle.OraclePlayer(22050, seed=6)
    p.queue(fa, 300, 40); p.queue(None, 10, 10)
    compare(bp.read(1), p.drain(), "middle")
    # 65 identical-shape utterances with different pitches
    n = 65
    frames = np.stack([scenarios.vowel_frame(ref, "i", 80.0 + 3 * k, 100.0 + k) for k in range(n)])
    bp.setUtterances(np.arange(n + 1), frames, [1500] * n, [200] * n)
    bp.synthesize()
    for k in (0, 1, 63, 64):
        p = oracle.OraclePlayer(22050, seed=k)
        p.queue(frames[k], 1500, 200)
        compare(bp.read(k), p.drain(), "u%d" % k)
    bp.close()


def test_prototypeless_ctypes_binding(ref):
    """The reference wrapper declares no prototypes (speechPlayer.py:48-57): the handle comes back
    through a C int and every argument is a plain Python int / byref.  Small-integer handles make
    that work on LP64; this test calls the library exactly that way."""
    import ctypes
    from nvspeechplayer_amd import _native, Frame
    dll = ctypes.cdll.LoadLibrary(_native.LIB_PATH)          # fresh handle, no argtypes / restype
    h = dll.speechPlayer_initialize(22050)
    assert isinstance(h, int) and 0 < h < 1 << 20
    fa = Frame.from_array(scenarios.vowel_frame(ref, "a", 120.0))
    dll.speechPlayer_queueFrame(h, ctypes.byref(fa), int(1000 * (22050 / 1000.0)), int(50 * (22050 / 1000.0)), -1, False)
    buf = (ctypes.c_short * 22050)()
    res = dll.speechPlayer_synthesize(h, 22050, buf)
    assert res == 22050
    import hashlib
    assert hashlib.sha1(bytes(buf)).hexdigest() == "3372ce96a8e60706afbfd092c3b79e7e7c43355e"
    assert dll.speechPlayer_getLastIndex(h) == -1
    dll.speechPlayer_queueFrame(h, None, 10, 10, 7, True)
    assert dll.speechPlayer_synthesize(h, 4096, buf) > 0
    assert dll.speechPlayer_getLastIndex(h) == 7
    dll.speechPlayer_terminate(h)


def test_many_live_streams_interleaved(ref):
    """Handles are independent streams: interleaving calls on several handles changes nothing."""
    import nvspeechplayer_amd as eng
    cases = [ref.ipa_case(ref.find_ipa(k)) for k in (0, 4, 6)]
    players = [eng.SpeechPlayer(22050, noiseSeed=50 + k) for k in range(3)]
    outs = [[] for _ in players]
    for k, (p, case) in enumerate(zip(players, cases)):
        for fr, m, f in case:
            p.queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f)
    alive = [True] * 3
    while any(alive):
        for k, p in enumerate(players):
            if not alive[k]:
                continue
            buf = p.synthesize(3000 + 500 * k)
            if buf is None:
                alive[k] = False
                continue
            outs[k].append(np.frombuffer(buf, dtype=np.int16)[:buf.length].copy())
            if buf.length < 3000 + 500 * k:
                alive[k] = False
    for k, case in enumerate(cases):
        o = oracle.OraclePlayer(22050, seed=50 + k)
        for fr, m, f in case:
            o.queue(fr, m, f)
        compare(np.concatenate(outs[k]), o.drain(), "stream %d" % k)
    for p in players:
        p.close()


def test_full_size_cfg1_properties():
    """BASELINE configs[1] at full size (4096 x 1 s): lengths, determinism across launches, equality
    of instanced utterances, and oracle equality on a strided sample of utterances."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    batch = workloads.make("cfg1", 4096)
    bp = eng.BatchPlayer(22050)
    bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                     batch["isnull"], batch["seeds"])
    assert bp.totalSamples == 4096 * 23155
    bp.synthesize()
    a, starts = bp.readAll()
    bp.synthesize()
    b, _ = bp.readAll()
    assert np.array_equal(a, b)                                   # idempotent relaunch
    assert np.all(np.diff(starts) == 23155)
    # utterance u and u + 4100 (= 20 * 205) would repeat; inside 4096 every (vowel, pitch) is unique, so
    # check structure instead: silence tail, non-silence body
    body = a.reshape(4096, 23155)
    assert np.all(np.abs(body[:, 5000:20000]).max(axis=1) > 500)
    assert np.all(np.abs(body[:, -50:]).max(axis=1) < np.abs(body[:, 5000:20000]).max(axis=1))   # faded out
    from tests import whole_batch
    n, differ = whole_batch.check_against_oracle(bp, batch, bp.digest(per_utterance=True)[1], compare, "cfg1")      # every utterance
    print("cfg1: %d utterances against the oracle, %d with one-LSB differences" % (n, differ))
    assert n == 4096
    bp.close()


@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("seed,wild", [(1, False), (2, True)])
def test_random_ragged_batches(seed, wild, layout):
    """1500 random utterances with unrelated timing in every wavefront (the general path of both kernels),
    quiet and noisy utterances mixed, against the oracle utterance by utterance."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(seed)
    batch = random_batch(rng, 1500, wild=wild)
    exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=8)
    for mode in (0, 1):
        bp = eng.BatchPlayer(22050, mode=mode, layout=layout)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                         batch["isnull"], batch["seeds"])
        assert bp.totalSamples == total
        bp.synthesize()
        got, got_start = bp.readAll()
        assert np.array_equal(got_start, exp_start)
        d = got.astype(np.int32) - exp.astype(np.int32)
        nbad = int(np.count_nonzero(d))
        print("seed %d wild %s layout %d mode %d: %d samples, %d differ, max |d| %d" % (seed, wild, layout, mode, total, nbad,
                                                                                     int(np.abs(d).max()) if total else 0))
        assert np.abs(d).max() <= 1
        assert nbad <= max(2, MAX_FLIPS_PER_M * total // 1000000 + 1)
        assert float(np.sqrt(np.mean((d / 32768.0) ** 2))) < RMS_TOL
        bp.close()


def test_lane_pipelined_kernel():
    """klatt_lanepipe.h (cascade resonators across lanes) on what it is for -- quiet, nasal-free utterances:
    ragged random ones (events, fades, NULL frames, vibrato in every wavefront) and a slice of BASELINE
    configs[1]; every utterance must take that kernel and equal the oracle, in both arithmetic modes,
    for one workgroup per CU (32-sample hand-overs) and beyond (16-sample hand-overs, two per CU)."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    rng = np.random.default_rng(7)
    ragged = random_batch(rng, 700, quiet_fraction=1.0, nasal_fraction=0.0)
    vowels = workloads.make("cfg1", 230)
    for name, batch in (("ragged", ragged), ("cfg1 slice", vowels)):
        n = len(batch["frame_start"]) - 1
        exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=8)
        for mode in (0, 1):
            bp = eng.BatchPlayer(22050, mode=mode, layout=2)
            bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                             batch["isnull"], batch["seeds"])
            info = bp.kernelInfo()
            assert info["lane_pipelined"] and info["lane_pipelined_utterances"] == n, info
            bp.synthesize()
            got, got_start = bp.readAll()
            assert np.array_equal(got_start, exp_start)
            nbad = int(np.count_nonzero(got != exp))
            print("%s mode %d: %d utterances, %d samples, %d differ; %s" % (name, mode, n, total, nbad, info))
            if mode == 0:
                assert nbad == 0
            else:
                compare(got, exp, name)
            bp.close()
    # 6000 vowels: more workgroups than CUs (the two-per-CU instantiation), against the stage-parallel kernel and the oracle
    big = workloads.make("cfg1", 6000)
    bp = eng.BatchPlayer(22050, layout=2)
    bp.setUtterances(big["frame_start"], big["frames"], big["min"], big["fade"], big["index"], big["isnull"], big["seeds"])
    assert bp.kernelInfo()["stage_parallel_chunk"] == 16
    bp.synthesize()
    got, got_start = bp.readAll()
    bp1 = eng.BatchPlayer(22050, layout=1)
    bp1.setUtterances(big["frame_start"], big["frames"], big["min"], big["fade"], big["index"], big["isnull"], big["seeds"])
    bp1.synthesize()
    ref1, _ = bp1.readAll()
    assert np.array_equal(got, ref1)
    for u in range(0, 6000, 997):
        sub = big.slice(u, 1)
        e, _, _ = oracle.batch_synthesize(22050, sub)
        assert np.array_equal(got[got_start[u]:got_start[u + 1]], e), u
    bp.close(); bp1.close()


def test_nasal_free_classification_boundaries():
    """Which utterances may skip the nasal pair (UTT_NO_NASAL, klatt_engine.hip): a slice of BASELINE configs[1] with,
    per utterance, one property pushed over a boundary of the classification -- caNP != 0 in one frame, a degenerate
    N0 bandwidth, a negative NP bandwidth, an enormous gain, a noise gain.  The engine must count exactly the untouched
    utterances as nasal-free, and every utterance (skipped pair or not) must equal the oracle."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    batch = workloads.make("cfg1", 60)
    fr = batch["frames"].copy()
    real = np.arange(0, 120, 2)                       # frame 0 of each utterance (frame 1 is the NULL frame)
    def touch(u, idx, value):
        fr[real[u], idx] = value
    touched = set()
    for u, (idx, value) in enumerate([(23, 0.25), (23, -0.0), (21, 0.5), (21, 0.0), (22, -1.0), (22, 0.0), (44, 1e31),
                                      (5, -3.0), (24, 0.1), (6, 0.05), (3, 0.2), (13, 2.0e6), (14, 300.0), (13, 0.0)]):
        touch(u, idx, value)
        if not ((idx == 23 and value == 0.0) or (idx == 22 and value == 0.0) or (idx == 5) or (idx == 14) or (idx == 13 and value == 0.0)):
            touched.add(u)                            # -0.0 caNP, NP bandwidth 0, a negative amplitude, another NP/N0 frequency stay eligible
    batch["frames"] = fr
    exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=4)
    for layout in (-1, 2, 1):
        bp = eng.BatchPlayer(22050, layout=layout)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                         batch["isnull"], batch["seeds"])
        info = bp.kernelInfo()
        assert info["lane_pipelined_utterances"] + info["nasal_free_utterances"] == 60 - len(touched), (layout, info, sorted(touched))
        bp.synthesize()
        got, got_start = bp.readAll()
        assert np.array_equal(got_start, exp_start)
        for u in range(60):
            a, b = got[got_start[u]:got_start[u + 1]], exp[exp_start[u]:exp_start[u + 1]]
            if u == 6:
                compare(a, b, "utterance 6 (gain 1e31: every sample clips)")
            else:
                assert np.array_equal(a, b), (layout, u, int(np.count_nonzero(a != b)))
        bp.close()


def test_zero_length_real_frame_division_by_zero(ref):
    """minFrameDuration = 0 on a real frame makes voicePitchInc = (end - start) / 0 (reference src/frame.cpp:98):
    +-inf or NaN pitch, NaN phase, and the reference's min/max macros turn the NaN sample into 32000.
    The engine follows IEEE arithmetic through the same steps."""
    import nvspeechplayer_amd as eng
    fa = scenarios.vowel_frame(ref, "a", 120.0)            # 0/0 -> NaN increment
    fb = scenarios.vowel_frame(ref, "i", 100.0, 180.0)     # 80/0 -> +inf increment
    fc = scenarios.vowel_frame(ref, "o", 150.0, 90.0)
    streams = [[(fa, 0, 30), (fc, 400, 100), (None, 50, 50)],
               [(fc, 300, 50), (fb, 0, 20), (fa, 300, 100), (None, 50, 50)]]
    frames = np.stack([np.zeros(47) if f is None else f for st in streams for f, _, _ in st])
    m = [x[1] for st in streams for x in st]; fd = [x[2] for st in streams for x in st]
    nul = [x[0] is None for st in streams for x in st]
    for layout in (-1, 2, 1, 0):     # vowels: the lane-pipelined and the nasal-free stage-parallel kernel see the NaN pitch too
        bp = eng.BatchPlayer(22050, layout=layout)
        bp.setUtterances([0, 3, 7], frames, m, fd, None, nul, [3, 4])
        bp.synthesize()
        for u, st in enumerate(streams):
            o = oracle.OraclePlayer(22050, seed=3 + u)
            for f, mm, ff in st:
                o.queue(f, mm, ff)
            exp = o.drain()
            got = bp.read(u)
            assert np.array_equal(got, exp), (layout, u, int(np.count_nonzero(got != exp)))
            assert (exp == 32000).any()
        bp.close()


def test_zero_length_real_frame_in_noisy_tracked_utterances(ref):
    """The same division by zero (reference src/frame.cpp:98, then :71 and :76-79) in utterances that take the FLAT stages: fricatives
    and an aspirated vowel with finite parameters are eligible for tracks, and the flat source stage walks (g46 - g0) / 0 -- +-inf or
    NaN -- through its pitch fade and glide.  M = 0 on a first frame, on a mid-utterance frame and right after a NULL frame;
    tracks on and off; the stage-parallel layouts and the lane kernel; other sample rates too."""
    import nvspeechplayer_amd as eng
    fs = scenarios.vowel_frame(ref, "s", 110.0)                  # 0/0 -> NaN increment
    fz = scenarios.vowel_frame(ref, "z", 130.0, 90.0)            # -40/0 -> -inf
    fh = scenarios.vowel_frame(ref, "a", 120.0, 180.0); fh[scenarios.ASPAMP] = 0.3      # aspirated: noisy; +60/0 -> +inf
    fv = scenarios.vowel_frame(ref, "o", 150.0, 95.0); fv[scenarios.FRICAMP] = 0.05
    streams = [[(fs, 0, 40), (fv, 500, 120), (None, 60, 60)],                                   # first frame
               [(fv, 400, 80), (fz, 0, 25), (fh, 350, 90), (None, 50, 50)],                     # mid-utterance
               [(fh, 300, 60), (None, 120, 40), (fh, 0, 30), (fs, 260, 70), (None, 40, 40)],    # right after a NULL frame
               [(fz, 0, 1), (fs, 0, 0), (fv, 200, 50), (None, 30, 30)]]                         # twice in a row, fades of one sample
    frames = np.stack([np.zeros(47) if f is None else f for st in streams for f, _, _ in st])
    m = [x[1] for st in streams for x in st]; fd = [x[2] for st in streams for x in st]
    nul = [x[0] is None for st in streams for x in st]
    start = np.concatenate([[0], np.cumsum([len(st) for st in streams])])
    for sr in (22050, 44100, 8000):
        exp = []
        for u, st in enumerate(streams):
            o = oracle.OraclePlayer(sr, seed=30 + u)
            for f, mm, ff in st:
                o.queue(f, mm, ff)
            exp.append(o.drain())
        assert any((e == 32000).any() for e in exp)
        for layout, tracks in ((-1, 1), (-1, 0), (1, 1), (1, 0), (0, 1)):
            bp = eng.BatchPlayer(sr, layout=layout)
            bp.setOption("tracks", tracks)
            bp.setUtterances(start, frames, m, fd, None, nul, [30 + u for u in range(len(streams))])
            info = bp.kernelInfo()
            if tracks and layout != 0:
                assert info["tracked_utterances"] == len(streams), info
            else:
                assert info["tracked_utterances"] == 0, info
            bp.synthesize()
            for u in range(len(streams)):
                got = bp.read(u)
                assert np.array_equal(got, exp[u]), (sr, layout, tracks, u, int(np.count_nonzero(got != exp[u])))
            bp.close()


def test_text_to_pcm_through_the_producer():
    """IPA text -> nvspeechplayer_amd.ipa -> BatchPlayer equals the oracle fed with the same frames."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import ipa
    texts = ["hælou", "ˈt͡ʃɑːt͡ʃ d͡ʒʌd͡ʒɪz", "ðɪs ɪz veɹj fɑn", "ʃiː sɛlz siːʃɛlz"]
    bp = eng.BatchPlayer(22050)
    bp.setIpa(texts, speed=1.0, basePitch=[100, 130, 85, 110], inflection=0.5, clauseType="?", noiseSeed=[9, 8, 7, 6])
    bp.synthesize()
    pk = ipa.frames_for_batch(texts, basePitch=[100, 130, 85, 110], clauseType="?")
    for u in range(len(texts)):
        o = oracle.OraclePlayer(22050, seed=9 - u)
        for k in range(pk["frame_start"][u], pk["frame_start"][u + 1]):
            o.queue(None if pk["isnull"][k] else pk["frames"][k], int(pk["min"][k]), int(pk["fade"][k]))
        compare(bp.read(u), o.drain(), texts[u])
    bp.close()


def test_full_size_cfg2_properties():
    """BASELINE configs[2] at full size (65 536 speech utterances, 1.5e9 samples): closed-form lengths,
    idempotent relaunch, noise-free utterances are independent of their seed (line 8 is all vowels, so
    u and u + 512 -- same line, same pitch variant, different noise stream -- must be bit-identical),
    noisy ones differ, and EVERY utterance equals the oracle (digest and index mark)."""
    import hashlib
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    batch = workloads.make("cfg2", 65536)
    k = np.arange(len(batch["index"]))
    batch["index"] = np.where(k % 11 == 4, (k % 30011).astype(np.int32), -1).astype(np.int32)      # index marks on every eleventh frame
    bp = eng.BatchPlayer(22050)
    bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                     batch["isnull"], batch["seeds"])
    counts = batch.sample_counts()
    assert bp.totalSamples == int(counts.sum())
    assert list(counts[:8]) == [8273, 29374, 29218, 20745, 12907, 41238, 13459, 29788]
    bp.synthesize()
    a, starts = bp.readAll()
    assert np.array_equal(np.diff(starts), counts)
    h1 = hashlib.sha1(a.tobytes()).hexdigest()
    bp.synthesize()
    b, _ = bp.readAll()
    assert hashlib.sha1(b.tobytes()).hexdigest() == h1            # idempotent
    del b
    for u in (7, 15, 7 + 8 * 63):                                  # quiet line, three pitch variants
        assert np.array_equal(a[starts[u]:starts[u + 1]], a[starts[u + 512]:starts[u + 513]])
    for u in (2, 13):                                              # noisy lines: another seed, another PCM
        assert not np.array_equal(a[starts[u]:starts[u + 1]], a[starts[u + 512]:starts[u + 513]])
    # EVERY utterance against the oracle: per-utterance digests computed where the PCM lives against the same digest of the oracle's
    # PCM (tests/whole_batch.py), index marks too; the digest kernel itself against the host's formula on what was read back
    from tests import whole_batch
    per = bp.digest(per_utterance=True)[1]
    assert np.array_equal(per[:2048], whole_batch.host_digests(a[:starts[2048]], starts[:2049]))
    del a
    n, differ = whole_batch.check_against_oracle(bp, batch, per, compare, "cfg2")
    print("cfg2: %d utterances against the oracle, %d with one-LSB differences" % (n, differ))
    assert n == 65536
    bp.close()


def test_output_formats(ref, tmp_path):
    """float samples scaled by 1/32767 (reference lavPlayer.py:17) and a WAV file,
    at the NVDA driver's 16 kHz rate (reference nvdaAddon/synthDrivers/nvSpeechPlayer/__init__.py:137)."""
    import wave
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(16000)
    bp.setIpa(["hælou", "ɑɑɑ"], clauseType=".")
    bp.synthesize()
    for u in range(2):
        pcm = bp.read(u)
        fl = bp.readFloat(u)
        assert fl.dtype == np.float32 and len(fl) == len(pcm)
        assert np.array_equal(fl, pcm.astype(np.float32) / np.float32(32767.0))
    path = str(tmp_path / "u0.wav")
    bp.writeWav(0, path)
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        assert np.array_equal(np.frombuffer(w.readframes(w.getnframes()), dtype="<i2"), bp.read(0))
    bp.close()


def test_cfg3_and_cfg4_recipes_small():
    """BASELINE configs[3] (utterances cut to <= 0.5 s) and configs[4] (voice variants with pitch / formant
    glides) at small size, utterance by utterance against the oracle."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    for batch in (workloads.make("cfg3", 200), workloads.cfg4_voice_variants(5, 40), workloads.make("cfg4", 300, first=900)):
        exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=8)
        bp = eng.BatchPlayer(22050)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                         batch["isnull"], batch["seeds"])
        bp.synthesize()
        got, got_start = bp.readAll()
        assert np.array_equal(got_start, exp_start)
        compare(got, exp, batch["name"])
        bp.close()


def test_engine_against_committed_golden_fixtures(all_scenarios):
    """The engine against tests/golden/expected.json + expected_pcm.npz directly (no oracle in the loop):
    SHA-1 and length of every batchable scenario, full PCM where it is stored."""
    import hashlib
    import json
    import os
    import nvspeechplayer_amd as eng
    table = json.load(open(os.path.join(scenarios.GOLDEN, "expected.json")))
    stored = np.load(os.path.join(scenarios.GOLDEN, "expected_pcm.npz"))
    rates = sorted({s.sr for s in all_scenarios if s.batchable})
    assert rates == [8000, 16000, 22050, 44100]
    for sr in rates:
        sel = [s for s in all_scenarios if s.batchable and s.sr == sr]
        batch = make_batch(sel)
        bp = eng.BatchPlayer(sr)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                         batch["isnull"], batch["seeds"])
        bp.synthesize()
        for i, s in enumerate(sel):
            pcm = bp.read(i)
            assert len(pcm) == table[s.name]["samples"], s.name
            assert hashlib.sha1(pcm.tobytes()).hexdigest() == table[s.name]["sha1"], s.name
            if s.name in stored.files:
                assert np.array_equal(pcm, stored[s.name]), s.name
        bp.close()


def test_limits_are_reported_not_wrapped(ref):
    """An utterance longer than 2^32 - 1 samples is refused with an error (lengths are 32-bit on the device)."""
    import nvspeechplayer_amd as eng
    fa = scenarios.vowel_frame(ref, "a", 120.0)
    bp = eng.BatchPlayer(22050)
    with pytest.raises(RuntimeError, match="too long"):
        bp.setUtterances([0, 2], np.stack([fa, fa]), [4294967295, 4294967295], [1, 1])
    bp.setUtterances([0, 1], fa[None, :], [100], [10])          # the object stays usable
    bp.synthesize()
    assert len(bp.read(0)) == 101
    bp.close()


@pytest.mark.parametrize("policy", ["alone", "shared", "alternate"])
def test_many_live_streams_one_launch(ref, all_scenarios, policy):
    """speechPlayer_synthesizeMany: 130 (300) live handles at unrelated points of unrelated streams, pulled together in uneven chunks, one
    of them purged on the way, frames queued between pulls -- each handle's PCM, call lengths and index marks equal its own oracle
    player's.  "alone": every handle in a wavefront of its own (the default up to 1536 handles, option "live_alone"); "shared": 64
    handles per wavefront (3 wavefronts; "live_alone" 1); "alternate": the policy changes from pull to pull of the same handles."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    rng = np.random.default_rng(5)
    # (300 handles alone: more workgroups than the chip has CUs, so some wait for a CU; the first 130 cases are the same in every policy)
    cases = [ref.ipa_case(int(i)) for i in rng.integers(0, len(ref.ipa_meta), size=300)][:300 if policy == "alone" else 130]
    players = [eng.SpeechPlayer(22050, noiseSeed=300 + k) for k in range(len(cases))]
    oracles = [oracle.OraclePlayer(22050, seed=300 + k) for k in range(len(cases))]
    fz = scenarios.vowel_frame(ref, "z", 130.0, 90.0)
    for k, case in enumerate(cases):
        half = len(case) // 2 if k % 3 == 0 else len(case)        # every third stream gets the rest later
        for j, (fr, m, f) in enumerate(case[:half]):
            players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, j)
            oracles[k].queue(fr, m, f, j)
    got = [[] for _ in cases]
    exp = [[] for _ in cases]
    for step, n in enumerate((3000, 1, 777, 8192, 4096, 8192, 8192, 8192, 8192, 8192, 8192)):
        if step == 2:
            players[7].queueFrameSamples(eng.Frame.from_array(fz), 900, 300, 99, True)     # purge one live stream
            oracles[7].queue(fz, 900, 300, 99, True)
        if step == 3:
            for k, case in enumerate(cases):
                if k % 3 == 0:
                    for j, (fr, m, f) in enumerate(case[len(case) // 2:]):
                        players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, 1000 + j)
                        oracles[k].queue(fr, m, f, 1000 + j)
        assert L.speechPlayer_setGlobalOption(b"live_alone", {"alone": 1536, "shared": 1, "alternate": 1536 if step % 2 else 1}[policy]) == 0
        try:
            bufs = eng.SpeechPlayer.synthesizeMany(players, n)
        finally:
            L.speechPlayer_setGlobalOption(b"live_alone", 1536)
        for k, b in enumerate(bufs):
            e = oracles[k].synthesize(n)
            g = np.zeros(0, np.int16) if b is None else np.frombuffer(b, dtype=np.int16)[:b.length].copy()
            assert len(g) == len(e), (step, k, len(g), len(e))
            assert players[k].getLastIndex() == oracles[k].last_index(), (step, k)
            got[k].append(g); exp[k].append(e)
    total = 0
    for k in range(len(cases)):
        total += compare(np.concatenate(got[k]), np.concatenate(exp[k]), "live stream %d" % k)
        players[k].close()
    assert total == 0


def test_live_handles_with_more_frames_than_their_rings(ref):
    """A handle keeps 256 frames on the device (klatt_engine.hip kRing); what is queued beyond waits on the host.  70 handles,
    each with 700-1500 short frames (4-40 samples, a few null, a few of length 0) queued at once, so that an 8192-sample pull
    runs past the ring's last frame and proceeds in pieces; a purge while frames wait on both sides; a handle closed with frames
    waiting and its arena slot taken over by a new handle.  PCM, call lengths and index marks against one oracle player each."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    rng = np.random.default_rng(77)
    names = ["a", "i", "u", "s", "z", "m", "n", "f", "v", "h"]
    shapes = [scenarios.vowel_frame(ref, nm, 110.0 + 7 * k, 100.0 + 5 * k) for k, nm in enumerate(names)]
    n = 70
    players = [eng.SpeechPlayer(22050, noiseSeed=900 + k) for k in range(n)]
    oracles = [oracle.OraclePlayer(22050, seed=900 + k) for k in range(n)]

    def queue_some(k, count, base):
        for j in range(count):
            r = rng.random()
            fr = None if r < 0.03 else shapes[int(rng.integers(0, len(shapes)))]
            m = 0 if r > 0.97 else int(rng.integers(4, 41))
            f = int(rng.integers(1, 30))
            players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, base + j)
            oracles[k].queue(fr, m, f, base + j)

    for k in range(n):
        queue_some(k, int(rng.integers(700, 1500)), 0)
    got = [[] for _ in range(n)]
    exp = [[] for _ in range(n)]
    L = _native.load()
    launches = []
    for step, cnt in enumerate((8192, 5000, 8192, 333, 8192, 8192, 8192)):
        if step == 1:       # purge: ring and host queue both hold frames of handle 3
            players[3].queueFrameSamples(eng.Frame.from_array(shapes[1]), 700, 200, 5000, True)
            oracles[3].queue(shapes[1], 700, 200, 5000, True)
            queue_some(3, 400, 6000)
        if step == 2:       # handle 5 closes with frames waiting; a new handle takes its slot over
            players[5].close()
            players[5] = eng.SpeechPlayer(22050, noiseSeed=4242)
            oracles[5] = oracle.OraclePlayer(22050, seed=4242)
            got[5], exp[5] = [], []
            queue_some(5, 300, 0)
        bufs = eng.SpeechPlayer.synthesizeMany(players, cnt)
        launches.append(L.speechPlayer_lastLiveLaunches(0))
        for k, b in enumerate(bufs):
            e = oracles[k].synthesize(cnt)
            g = np.zeros(0, np.int16) if b is None else np.frombuffer(b, dtype=np.int16)[:b.length].copy()
            assert len(g) == len(e), (step, k, len(g), len(e))
            assert players[k].getLastIndex() == oracles[k].last_index(), (step, k)
            got[k].append(g); exp[k].append(e)
    assert max(launches) > 1, launches          # some pull did go in pieces
    total = 0
    for k in range(n):
        total += compare(np.concatenate(got[k]), np.concatenate(exp[k]), "overflowing live stream %d" % k)
        players[k].close()
    assert total == 0


def test_live_queueing_thread_beside_pulling_thread(ref):
    """speechPlayer_queueFrame from one thread while another pulls OTHER handles (the NVDA driver queues from the speech thread while
    its audio thread pulls): the queueing thread fills the pinned log (and sends it on its way when no pull is running), the pulls
    upload what is left of it.  Two groups of 40 handles; while group A is pulled four times, a second thread queues group B's
    frames; then B is pulled.  Every handle against its own oracle player."""
    import threading
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(99)
    cases = [ref.ipa_case(int(i)) for i in rng.integers(0, len(ref.ipa_meta), size=80)]
    players = [eng.SpeechPlayer(22050, noiseSeed=700 + k) for k in range(80)]
    oracles = [oracle.OraclePlayer(22050, seed=700 + k) for k in range(80)]
    for k in range(40):
        for j, (fr, m, f) in enumerate(cases[k]):
            players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, j)
            oracles[k].queue(fr, m, f, j)

    def queue_b():
        for rep in range(6):                      # 6 x the case: ~1.7 MB of log per handle group and repetition
            for k in range(40, 80):
                for j, (fr, m, f) in enumerate(cases[k]):
                    players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, 100 * rep + j)
    t = threading.Thread(target=queue_b)
    t.start()
    got = [[] for _ in range(80)]
    exp = [[] for _ in range(80)]
    ga = eng.LiveGroup(players[:40])
    out = np.zeros((40, 8192), dtype=np.int16)
    for _ in range(4):
        prod = ga.pull(8192, out).copy()
        for k in range(40):
            got[k].append(out[k, :prod[k]].copy())
    t.join()
    for rep in range(6):
        for k in range(40, 80):
            for j, (fr, m, f) in enumerate(cases[k]):
                oracles[k].queue(fr, m, f, 100 * rep + j)
    gb = eng.LiveGroup(players[40:])
    for _ in range(5):
        prod = gb.pull(8192, out).copy()
        for k in range(40):
            got[40 + k].append(out[k, :prod[k]].copy())
    total = 0
    for k in range(80):
        for _ in range(4 if k < 40 else 5):
            exp[k].append(oracles[k].synthesize(8192))
        total += compare(np.concatenate(got[k]), np.concatenate(exp[k]), "threaded live stream %d" % k)
        assert players[k].getLastIndex() == oracles[k].last_index(), k
        players[k].close()
    assert total == 0


def test_random_ragged_batch_large():
    """One big random batch (20 000 utterances, ~8e7 samples, both launch groups, two workgroups per CU):
    bit-for-bit against the oracle.  Bounds the rate of differing samples well below 1e-7."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(11)
    batch = random_batch(rng, 20000, wild=True)
    exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=16)
    for layout in (-1, 2):     # 2: the quiet, nasal-free utterances (about 1000 of them, ragged) through the lane-pipelined kernel
        bp = eng.BatchPlayer(22050, layout=layout)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                         batch["isnull"], batch["seeds"])
        info = bp.kernelInfo()
        bp.synthesize()
        got, got_start = bp.readAll()
        assert np.array_equal(got_start, exp_start)
        nbad = int(np.count_nonzero(got != exp))
        print("large random batch, layout %d: %d samples, %d differ (lane-pipelined %d, nasal-free stage-parallel %d utterances)" % (
            layout, total, nbad, info["lane_pipelined_utterances"], info["nasal_free_utterances"]))
        assert nbad == 0
        # (layout -1 sends quiet utterances whose timing nobody shares to the flat stages -- same PCM; an explicit layout is taken at its word)
        if layout == 2:
            assert info["lane_pipelined_utterances"] + info["nasal_free_utterances"] > 300
        bp.close()


def test_threads_and_lifetime(ref):
    """Producer/consumer threading as in the NVDA driver (queueFrame from one thread, synthesize from another,
    reference nvdaAddon/synthDrivers/nvSpeechPlayer/__init__.py:62-81,231-235), several handles at once from
    several threads, and repeated create/destroy of handles and batches."""
    import threading
    import nvspeechplayer_amd as eng
    cases = [ref.ipa_case(ref.find_ipa(k)) for k in (1, 2, 3, 5)]
    results = [None] * len(cases)

    def worker(k):
        p = eng.SpeechPlayer(22050, noiseSeed=70 + k)
        done_queueing = threading.Event()

        def producer():
            for fr, m, f in cases[k]:
                p.queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f)
            done_queueing.set()
        t = threading.Thread(target=producer)
        t.start()
        done_queueing.wait()          # the PCM depends on when frames arrive relative to pulls; keep it deterministic
        parts = []
        while True:
            buf = p.synthesize(2048)
            if buf is None:
                break
            parts.append(np.frombuffer(buf, dtype=np.int16)[:buf.length].copy())
            if buf.length < 2048:
                break
        t.join()
        results[k] = np.concatenate(parts)
        p.close()

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(len(cases))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k, case in enumerate(cases):
        o = oracle.OraclePlayer(22050, seed=70 + k)
        for fr, m, f in case:
            o.queue(fr, m, f)
        compare(results[k], o.drain(), "thread %d" % k)
    fa = scenarios.vowel_frame(ref, "a", 120.0)
    first = None
    for rep in range(30):                                   # handles and batches come and go
        p = eng.SpeechPlayer(22050)
        p.queueFrameSamples(eng.Frame.from_array(fa), 200, 20)
        b = p.synthesize(512)
        bp = eng.BatchPlayer(22050)
        bp.setUtterances([0, 1], fa[None, :], [200], [20])
        bp.synthesize()
        x = bp.read(0)
        if first is None:
            first = x.copy()
        assert np.array_equal(x, first) and np.array_equal(np.frombuffer(b, dtype=np.int16)[:b.length], first)
        bp.close(); p.close()


@pytest.mark.parametrize("workload,n_utt", [("cfg3", 125000), ("cfg4", 524288)])
def test_full_size_cfg3_cfg4_properties(workload, n_utt):
    """BASELINE configs[3] and configs[4] at their per-GPU size (10^6 / 8 = 125 000 cut utterances; 256 / 8 = 32 voice
    variants x 16 384 utterances = 524 288 utterances, 1.2e10 samples, 24 GB of PCM): closed-form lengths, the two
    independent kernel layouts (stage-parallel workgroups and one wavefront per 64 utterances) produce the same bytes,
    both arithmetic modes stay within the tolerance, and a strided sample of utterances equals the oracle.  The PCM never
    leaves the device whole: layouts are compared by the device-side digest (speechPlayer_batch_digest, itself checked
    against numpy on the utterances that are read back)."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    from nvspeechplayer_amd.speechPlayer import pcm_digest
    batch = workloads.make(workload, n_utt)
    assert batch.n_utt == n_utt
    k = np.arange(len(batch["index"]))
    batch["index"] = np.where(k % 11 == 4, (k % 30011).astype(np.int32), -1).astype(np.int32)      # index marks on every eleventh frame
    counts = batch.sample_counts()
    assert np.array_equal(counts, workloads.sample_counts(workload, n_utt))
    if workload == "cfg4":
        assert batch["name"].endswith("x 16384 utterances") and int(counts.sum()) > 1.2e10
    digests = {}
    per = {}
    strided = list(range(3, n_utt, max(1, n_utt // 40)))
    for layout, mode in ((1, 0), (0, 0), (1, 1)):
        bp = eng.BatchPlayer(22050, mode=mode, layout=layout)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"],
                         batch["isnull"], batch["seeds"])
        assert bp.totalSamples == int(counts.sum())
        bp.synthesize()
        digests[(layout, mode)], per[(layout, mode)] = bp.digest(per_utterance=True)
        if (layout, mode) == (1, 0):
            for u in strided:
                got = bp.read(u)
                assert len(got) == counts[u]
                assert pcm_digest(got) == int(per[(1, 0)][u]), u                 # the digest kernel agrees with numpy
                exp, _, _ = oracle.batch_synthesize(22050, batch.slice(u, 1))
                compare(got, exp, "%s utt %d" % (workload, u))
                assert bp.getLastIndex(u) == int(oracle.batch_last_index(22050, batch.slice(u, 1))[0])      # reference src/frame.cpp:69, :117-119
            for u in (0, n_utt - 1):
                assert bp.utteranceSamples(u) == counts[u] and len(bp.read(u)) == counts[u]
            # configs[3]'s share: every utterance against the oracle; configs[4]'s (1.2e10 samples): every eighth
            from tests import whole_batch
            n, differ = whole_batch.check_against_oracle(bp, batch, per[(1, 0)], compare, workload, stride=1 if workload == "cfg3" else 8)
            print("%s: %d utterances against the oracle, %d with one-LSB differences" % (workload, n, differ))
            keep = bp
            continue
        if mode == 1:
            differ = np.flatnonzero(per[(layout, mode)] != per[(1, 0)])
            print("%s: MODE_FAST differs from MODE_EXACT in %d of %d utterances" % (workload, len(differ), n_utt))
            for u in differ[:50]:
                compare(bp.read(int(u)), keep.read(int(u)), "%s MODE_FAST against MODE_EXACT, utt %d" % (workload, u))   # tolerance, not identity
        bp.close()
    keep.close()
    assert digests[(1, 0)] == digests[(0, 0)], "the two kernel layouts disagree on %s" % workload
    assert np.array_equal(per[(1, 0)], per[(0, 0)])


def test_native_c_client(ref, tmp_path):
    """A C program built with gcc against include/speechPlayer.h and the engine library (no Python, no
    prototypes beyond the header) gets the oracle's PCM, in one pull and in ragged pulls."""
    import subprocess
    from nvspeechplayer_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.environ.get("SPEECHPLAYER_LIB") or _native.LIB_PATH
    exe = str(tmp_path / "c_client")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "native", "c_client.c"), lib, "-Wl,-rpath," + os.path.dirname(lib)])
    for name, pitch, pull in (("a", 120.0, 22050), ("s", 0.0, 777), ("m", 95.0, 4096)):
        fr = scenarios.vowel_frame(ref, name, pitch)
        fbin = tmp_path / ("frame_%s.bin" % name)
        fbin.write_bytes(np.asarray(fr, dtype=np.float64).tobytes())
        out = tmp_path / ("out_%s.pcm" % name)
        line = subprocess.check_output([exe, str(fbin), str(out), "22050", "3000", "400", str(pull)]).decode().split()
        pcm = np.frombuffer(out.read_bytes(), dtype=np.int16)
        o = oracle.OraclePlayer(22050, seed=0)
        o.queue(fr, 3000, 400, 7)
        o.queue(None, 400, 400, -1)
        exp = o.drain()
        assert int(line[0]) == len(exp) == len(pcm) and int(line[1]) == 7
        compare(pcm, exp, "c client %s" % name)


def test_nan_targets_out_of_silence(ref):
    """A NaN parameter ("hold", reference src/utils.h:21) on the FIRST frame of an utterance and on the frame right
    after a NULL frame: both fade out of silence (reference src/frame.cpp:64-67: old = new with gain 0), so old and
    new are the same NaN except for the gain, and a NaN gain must hold 0 (silence) -- the branch ADVICE r1 found
    dropping the "NaN target" flag.  Every parameter 1..45, a vowel and a fricative shape, all four layouts."""
    import nvspeechplayer_amd as eng
    shapes = [scenarios.vowel_frame(ref, "a", 120.0, 90.0), scenarios.vowel_frame(ref, "s", 0.0), scenarios.vowel_frame(ref, "m", 100.0, 140.0)]
    follow = scenarios.vowel_frame(ref, "i", 200.0, 150.0)
    streams = []
    for idx in range(1, 46):
        for si, shape in enumerate(shapes):
            if (idx + si) % 3 and idx != scenarios.PREGAIN:
                continue                                   # a third of the (parameter, shape) pairs; the gain with all shapes
            f = shape.copy(); f[idx] = np.nan
            streams.append([(f, 700, 300), (follow, 600, 250), (None, 200, 200)])                      # first frame
            streams.append([(follow, 500, 120), (None, 300, 150), (f, 700, 300), (shape, 400, 100), (None, 100, 100)])   # after a NULL frame
    frames = np.stack([np.zeros(47) if f is None else f for st in streams for f, _, _ in st])
    m = [x[1] for st in streams for x in st]; fd = [x[2] for st in streams for x in st]
    nul = [x[0] is None for st in streams for x in st]
    start = np.concatenate([[0], np.cumsum([len(st) for st in streams])])
    seeds = np.arange(len(streams)) + 77
    exp = []
    for u, st in enumerate(streams):
        o = oracle.OraclePlayer(22050, seed=int(seeds[u]))
        for f, mm, ff in st:
            o.queue(f, mm, ff)
        exp.append(o.drain())
    silent = 0
    for layout in (-1, 1, 0, 2):
        bp = eng.BatchPlayer(22050, layout=layout)
        bp.setUtterances(start, frames, m, fd, None, nul, seeds)
        bp.synthesize()
        for u in range(len(streams)):
            got = bp.read(u)
            assert np.array_equal(got, exp[u]), (layout, u, int(np.count_nonzero(got != exp[u])))
        bp.close()
    # the NaN gain on a first frame holds 0: silence for the whole first request
    for u, st in enumerate(streams):
        if st[0][0] is not None and np.isnan(st[0][0][scenarios.PREGAIN]):
            assert not exp[u][:700].any() and (exp[u][705:900] == 32000).all()   # then the NaN itself is the fade's origin
            silent += 1
    assert silent == len(shapes)


def test_bench_two_ranks_on_one_gpu(tmp_path):
    """`python bench.py --gpus 2` for real: the parent starts two ranks itself; with one GPU on the box they share device 0
    and rendezvous over gloo (RCCL needs one device per rank).  World size 2, node batch = 2 x the per-GPU size, shards
    balanced by samples, whole-job throughput reported once."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--workload", "cfg3", "--utterances", "4000",
                                   "--steps", "4", "--warmup", "1"], env=env, cwd=str(tmp_path), timeout=600)
    lines = [l for l in out.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["world_size"] == 2 and d["config"]["node_utterances"] == 8000
    assert d["value"] > 1e9 and d["steps"] == 4 and "roofline" in d and "cpu_baseline" not in d
    b = d["config"]["shard_bounds"]
    assert b[0] == 0 and b[2] == 8000 and abs(b[1] - 4000) < 200


def test_bench_rccl_branch_at_world_size_one(tmp_path):
    """The process group of the N > 1 run -- backend "nccl" (RCCL) initialised with device_id, the barrier around the timed region
    and both all_reduces on device tensors -- on the one GPU of this box: BENCH_FORCE_PG=1 takes that branch at world size 1."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["BENCH_FORCE_PG"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py"), "--workload", "cfg3", "--utterances", "4000", "--steps", "4",
                                   "--warmup", "1", "--no-extras", "--no-cpu-baseline"], env=env, cwd=str(tmp_path), timeout=600)
    lines = [l for l in out.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    c = d["config"]
    assert c["process_group"] == "nccl" and c["rccl_ranks"] == 1 and c["world_size"] == 1 and d["n_gpus"] == 1
    assert d["value"] > 1e9 and d["steps"] == 4 and "roofline" in d
    assert c["host"]["set_utterances_s"] > 0 and c["host"]["first_launch_end_to_end_samples_per_s"] > 0


def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """A plain `bench.py` line is the headline alone (the extras come with --full), and --dump-outputs writes what the last timed
    step computed for a seeded sample of the utterances: float32 / float64 .npy files, the same on a second run, the PCM and the
    index marks the oracle gives for those utterances."""
    import json
    import subprocess
    import sys
    from nvspeechplayer_amd import workloads
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    names = ("pcm", "pcm_offsets", "utterances", "last_index")
    dumps = []
    for k in range(2):
        outdir = tmp_path / ("dump%d" % k)
        out = subprocess.check_output([sys.executable, os.path.join(root, "bench.py"), "--workload", "cfg3", "--utterances", "4000", "--steps", "3",
                                       "--warmup", "1", "--dump-outputs", str(outdir)], env=env, cwd=str(tmp_path), timeout=600)
        lines = [l for l in out.decode().splitlines() if l.startswith("{")]
        assert len(lines) == 1, out
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 1e9 and d["dtype"] == "f64"
        assert not set(d) & {"mode_fast", "tracks_off", "cfg1", "pipeline", "single_stream", "live_handles", "cfg0_cpu", "cpu_baseline"}
        dumps.append({n: np.load(str(outdir / (n + ".npy"))) for n in names})
    a, b = dumps
    for n in names:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    utt, off = a["utterances"].astype(np.int64), a["pcm_offsets"].astype(np.int64)
    assert len(utt) == 256 and (np.diff(utt) > 0).all() and len(off) == 257 and off[-1] == len(a["pcm"])
    batch = workloads.make("cfg3", 4000)
    for j, u in enumerate(utt):
        one = batch.slice(int(u), 1)
        exp, _, _ = oracle.batch_synthesize(batch["sr"], one)
        compare(a["pcm"][off[j]:off[j + 1]].astype(np.int16), exp, "utterance %d" % u)
        assert a["last_index"][j] == int(oracle.batch_last_index(batch["sr"], one)[0])


def test_error_codes_and_digest(ref):
    """speechPlayer_lastErrorCode: non-zero after a failed call, back to 0 after the next successful one; and the device-side
    digest against the same formula in numpy, per utterance, on a ragged batch (lengths 0, 1, 7, 8, 9, ... samples)."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    from nvspeechplayer_amd.speechPlayer import pcm_digest
    fa = scenarios.vowel_frame(ref, "a", 120.0)
    bp = eng.BatchPlayer(22050)
    with pytest.raises(RuntimeError, match="too long"):
        bp.setUtterances([0, 2], np.stack([fa, fa]), [4294967295, 4294967295], [1, 1])
    assert _native.last_error_code() == 1
    with pytest.raises(RuntimeError, match="not monotone"):
        bp.setUtterances([0, 100, 5], np.stack([fa] * 5), [10] * 5, [1] * 5)          # validated before anything is indexed
    lens = [0, 1, 5, 6, 7, 8, 30, 31, 32, 33, 500, 4097]
    m = [max(0, n - 2) for n in lens]                                               # a frame of M spans max(M, F + 1) + 1 = M + 1 (F = 0 -> 1) ... plus one
    frames = np.stack([fa] * len(lens))
    bp.setUtterances(np.arange(len(lens) + 1), frames, m, [0] * len(lens))
    assert _native.last_error_code() == 0
    bp.synthesize()
    whole, per = bp.digest(per_utterance=True)
    for u in range(len(lens)):
        pcm = bp.read(u)
        assert len(pcm) == max(m[u], 2) + 1
        assert pcm_digest(pcm) == int(per[u]), u
    bp2 = eng.BatchPlayer(22050, layout=0)
    bp2.setUtterances(np.arange(len(lens) + 1), frames, m, [0] * len(lens))
    bp2.synthesize()
    assert bp2.digest() == whole
    frames[3, 7] += 1.0                                                              # another F1: another PCM, another digest
    bp2.setUtterances(np.arange(len(lens) + 1), frames, m, [0] * len(lens))
    bp2.synthesize()
    w2, per2 = bp2.digest(per_utterance=True)
    assert w2 != whole and np.flatnonzero(per2 != per).tolist() == [3]
    # a live handle: a drained queue and a failure both return 0 samples; the code tells them apart
    p = eng.SpeechPlayer(22050)
    assert p.synthesize(64) is None and _native.last_error_code() == 0
    p.close(); bp.close(); bp2.close()


def test_one_batch_over_several_devices(ref, all_scenarios):
    """speechPlayer_node_*: one ragged batch cut into sample-balanced contiguous shards, one per device entry (this box has
    one GPU, so the three shards share device 0 -- three Batch objects, three streams, three upload threads): every
    utterance's PCM and index mark equal the single-device batch's, default seeds are the utterance's number in the WHOLE
    batch, and the shards' sample counts are balanced."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd.sharding import shard_bounds
    sel = [s for s in all_scenarios if s.batchable and s.sr == 22050]
    batch = make_batch(sel)
    n = len(sel)
    one = eng.BatchPlayer(22050)
    one.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], None)
    one.synthesize()
    node = eng.NodePlayer(22050, [0, 0, 0])
    node.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], None)
    assert node.totalSamples == one.totalSamples
    sh = node.shards()
    lens = np.array([one.utteranceSamples(u) for u in range(n)])
    assert [a for a, _, _, _ in sh] + [n] == list(shard_bounds(lens, 3))                 # the same deal as the Python helper
    assert sum(c for _, c, _, _ in sh) == n and [s for _, _, s, _ in sh] == [int(lens[a:a + c].sum()) for a, c, _, _ in sh]
    assert max(s for _, _, s, _ in sh) - min(s for _, _, s, _ in sh) <= 2 * lens.max()
    node.synthesize()
    for u in range(n):
        assert np.array_equal(node.read(u), one.read(u)), u
        assert node.getLastIndex(u) == one.getLastIndex(u)
    ms = node.time(2)
    assert len(ms) == 2 and (ms > 0).all()
    with pytest.raises(RuntimeError, match="out of range|failed"):
        node.read(n)
    # the SORTED deal (option "deal"): blocks of 64 length-sorted utterances dealt round-robin -- the same partition as
    # nvspeechplayer_amd.sharding.shard_deal, every utterance's PCM and mark still found under its number in the whole batch
    from nvspeechplayer_amd.sharding import shard_deal
    big = make_batch(sel * 5)                                   # 5 x the corpus: several blocks of 64 per shard
    nb = len(sel) * 5
    one.setUtterances(big["frame_start"], big["frames"], big["min"], big["fade"], big["index"], big["isnull"], None)
    one.synthesize()
    node.setOption("deal", 1)
    node.setUtterances(big["frame_start"], big["frames"], big["min"], big["fade"], big["index"], big["isnull"], None)
    lens = np.array([one.utteranceSamples(u) for u in range(nb)])
    want = shard_deal(lens, 3, "sorted")
    for d in range(3):
        assert np.array_equal(node.shardUtterances(d), want[d])
    assert [a for a, _, _, _ in node.shards()] == [-1, -1, -1] and sum(c for _, c, _, _ in node.shards()) == nb
    assert node.totalSamples == one.totalSamples
    node.synthesize()
    assert np.array_equal(node.digests(), one.digest(per_utterance=True)[1])
    for u in range(0, nb, 7):
        assert np.array_equal(node.read(u), one.read(u)), u
        assert node.getLastIndex(u) == one.getLastIndex(u)
    node.setOption("deal", 0)
    node.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], None)
    assert [a for a, _, _, _ in node.shards()] + [n] == list(shard_bounds(np.array([lens[u] for u in range(n)]), 3))
    node.close(); one.close()


def test_live_handles_on_both_kernels(all_scenarios, ref):
    """Live handles advance on the stage-parallel kernel's STREAM instantiation by default (every stage restores and saves its slice
    of the handle's 240-double state) and on the lane kernel when asked (speechPlayer_setGlobalOption("live_layout", 0)).  The
    saved state is one format: the streaming scenarios (chunked pulls of 1..8192 samples, purge in steady state and inside a
    fade, drain and resume, vibrato, NaN holds) must equal the oracle call by call on either kernel AND when the kernel
    changes between pulls of the same handle; 200 handles pulled together (more than three workgroups) likewise."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    names = ("cfg0_a_1s", "stream_chunks", "purge_resume", "vowelchart_pairs", "hannah_vibrato", "nan_hold", "duration_edges")
    try:
        assert L.speechPlayer_setGlobalOption(b"live_alone", 1) == 0      # (the 200 handles share wavefronts: the kernels this test is about)
        for policy in ("stage", "lane", "alternate"):
            pulls = [0]

            def before_pull():
                if policy == "alternate":
                    assert L.speechPlayer_setGlobalOption(b"live_layout", pulls[0] % 2) == 0
                pulls[0] += 1
            assert L.speechPlayer_setGlobalOption(b"live_layout", 0 if policy == "lane" else 1) == 0
            for scn in all_scenarios:
                if scn.name not in names:
                    continue
                exp_pcm, exp_marks = scenarios.play_oracle(scn)
                p = eng.SpeechPlayer(scn.sr, noiseSeed=scn.seed)
                got_pcm, got_marks = [], []

                def synth(n):
                    before_pull()
                    buf = p.synthesize(n)
                    return np.zeros(0, np.int16) if buf is None else np.frombuffer(buf, dtype=np.int16)[:buf.length].copy()
                for op in scn.ops:
                    if op[0] == "q":
                        p.queueFrameSamples(None if op[1] is None else eng.Frame.from_array(op[1]), op[2], op[3], op[4], op[5])
                    elif op[0] == "s":
                        got_pcm.append(synth(op[1])); got_marks.append(p.getLastIndex())
                    else:
                        parts = []
                        while True:
                            x = synth(1000 + 37 * len(parts))            # ragged pulls, not multiples of the hand-over size
                            parts.append(x)
                            if len(x) < 1000 + 37 * (len(parts) - 1):
                                break
                        got_pcm.append(np.concatenate(parts)); got_marks.append(p.getLastIndex())
                p.close()
                assert [len(x) for x in got_pcm] == [len(x) for x in exp_pcm], (policy, scn.name)
                assert got_marks == exp_marks, (policy, scn.name)
                assert np.array_equal(np.concatenate(got_pcm), np.concatenate(exp_pcm)), (policy, scn.name)
        # many handles together, the kernel changing between pulls
        rng = np.random.default_rng(17)
        cases = [ref.ipa_case(int(i)) for i in rng.integers(0, len(ref.ipa_meta), size=200)]
        players = [eng.SpeechPlayer(22050, noiseSeed=900 + k) for k in range(len(cases))]
        oracles = [oracle.OraclePlayer(22050, seed=900 + k) for k in range(len(cases))]
        for k, case in enumerate(cases):
            for j, (fr, m, f) in enumerate(case):
                players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, j)
                oracles[k].queue(fr, m, f, j)
        for step, n in enumerate((4097, 13, 8192, 8192, 5000, 8192, 8192, 8192)):
            assert L.speechPlayer_setGlobalOption(b"live_layout", (step + 1) % 2) == 0
            bufs = eng.SpeechPlayer.synthesizeMany(players, n)
            for k, b in enumerate(bufs):
                e = oracles[k].synthesize(n)
                g = np.zeros(0, np.int16) if b is None else np.frombuffer(b, dtype=np.int16)[:b.length].copy()
                assert np.array_equal(g, e), (step, k, len(g), len(e))
                assert players[k].getLastIndex() == oracles[k].last_index(), (step, k)
        for p in players:
            p.close()
    finally:
        L.speechPlayer_setGlobalOption(b"live_layout", 1)
        L.speechPlayer_setGlobalOption(b"live_alone", 1536)


def test_large_live_pulls_take_the_two_per_cu_stream_kernel(all_scenarios, ref):
    """pulls of more live handles than CUs x 64 (16 384 on MI355X) launch klatt_systolic<MODE, true, 8, 2, true, true>
    -- 8-sample hand-overs, two workgroups per CU -- which no test had ever run.  speechPlayer_setGlobalOption("live_cus", 1) makes
    every pull of more than 64 handles take it: 330 handles (six workgroups, the last one ragged) with index marks, purge and late
    queueing on the way, the kernel alternating with the lane kernel and with the one-per-CU instantiation between pulls of the
    same handles, pulls that are not multiples of the hand-over size; then the 8 kHz / 16 kHz / 44.1 kHz golden scenarios through
    70 live handles each on the same kernel -- against one oracle player per handle, sample for sample and mark for mark."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    try:
        assert L.speechPlayer_setGlobalOption(b"live_alone", 1) == 0      # (64 handles per wavefront: the kernels this test is about)
        rng = np.random.default_rng(23)
        cases = [ref.ipa_case(int(i)) for i in rng.integers(0, len(ref.ipa_meta), size=330)]
        players = [eng.SpeechPlayer(22050, noiseSeed=5000 + k) for k in range(len(cases))]
        oracles = [oracle.OraclePlayer(22050, seed=5000 + k) for k in range(len(cases))]
        for k, case in enumerate(cases):
            for j, (fr, m, f) in enumerate(case):
                players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, j)
                oracles[k].queue(fr, m, f, j)
        late = cases[7]
        # (live_cus, live_layout) per pull: the two-per-CU stream kernel, the one-per-CU one, the lane kernel
        plan = ((1, 1, 4097), (1, 1, 13), (0, 1, 2500), (1, 1, 8192), (1, 0, 3001), (1, 1, 8192), (1, 1, 7), (1, 1, 8192), (1, 1, 8192), (1, 1, 8192))
        for step, (cus, layout, n) in enumerate(plan):
            assert L.speechPlayer_setGlobalOption(b"live_cus", cus) == 0 and L.speechPlayer_setGlobalOption(b"live_layout", layout) == 0
            if step == 3:      # a purge inside whatever every fifth handle is doing, and new frames behind it (reference src/frame.cpp:103-112)
                for k in range(0, len(players), 5):
                    fr, m, f = late[2]
                    players[k].queueFrameSamples(eng.Frame.from_array(fr), m, f, 777, True)
                    oracles[k].queue(fr, m, f, 777, True)
            if step == 5:      # late queueing: handles that have run dry speak again
                for k in range(3, len(players), 4):
                    for j, (fr, m, f) in enumerate(late):
                        players[k].queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f, 100 + j)
                        oracles[k].queue(fr, m, f, 100 + j)
            bufs = eng.SpeechPlayer.synthesizeMany(players, n)
            for k, b in enumerate(bufs):
                e = oracles[k].synthesize(n)
                g = np.zeros(0, np.int16) if b is None else np.frombuffer(b, dtype=np.int16)[:b.length].copy()
                assert np.array_equal(g, e), (step, k, len(g), len(e))
                assert players[k].getLastIndex() == oracles[k].last_index(), (step, k)
        for p in players:
            p.close()
        # the sample rates of the golden scenarios through live handles on the same kernel: 70 handles per scenario, pulled together
        for name in ("ipa_l3_8k", "ipa_l0_16k", "ipa_l1_44k", "vowel_fric_nasal_44k", "vowel_fric_nasal_8k"):
            scn = next(s for s in all_scenarios if s.name == name)
            assert L.speechPlayer_setGlobalOption(b"live_cus", 1) == 0 and L.speechPlayer_setGlobalOption(b"live_layout", 1) == 0
            ps = [eng.SpeechPlayer(scn.sr, noiseSeed=scn.seed + k) for k in range(70)]
            os_ = [oracle.OraclePlayer(scn.sr, seed=scn.seed + k) for k in range(70)]
            for op in scn.ops:
                if op[0] == "q":
                    for p, o in zip(ps, os_):
                        p.queueFrameSamples(None if op[1] is None else eng.Frame.from_array(op[1]), op[2], op[3], op[4], op[5])
                        o.queue(op[1], op[2], op[3], op[4], op[5])
            while True:
                bufs = eng.SpeechPlayer.synthesizeMany(ps, 3000)
                done = True
                for p, o, b in zip(ps, os_, bufs):
                    e = o.synthesize(3000)
                    g = np.zeros(0, np.int16) if b is None else np.frombuffer(b, dtype=np.int16)[:b.length].copy()
                    assert np.array_equal(g, e), (name, len(g), len(e))
                    assert p.getLastIndex() == o.last_index()
                    done = done and len(e) < 3000
                if done:
                    break
            for p in ps:
                p.close()
    finally:
        L.speechPlayer_setGlobalOption(b"live_cus", 0)
        L.speechPlayer_setGlobalOption(b"live_layout", 1)
        L.speechPlayer_setGlobalOption(b"live_alone", 1536)


def test_quiet_classification_needs_finite_parallel_coefficients(ref):
    """an utterance with zero noise gains skips the parallel bank only while the bank's coefficients stay finite. A large
    negative parallel bandwidth makes exp(-pi bw / sr) overflow: a = inf, a * 0 = NaN, and the reference's clip turns NaN into
    32000.  Such utterances must run the full (noisy) kernel -- in every layout -- and equal the oracle."""
    import nvspeechplayer_amd as eng
    base = scenarios.vowel_frame(ref, "a", 120.0)
    assert base[3] == 0 and base[6] == 0 and base[24] == 0                    # a quiet frame
    cases = []
    for idx, value in ((31, -8.0e6), (34, -6.0e6), (36, -2.0e7), (33, 2.0e6), (25, 3.0e6), (31, -100.0), (31, 0.0), (25, -5000.0)):
        f = base.copy(); f[idx] = value
        cases.append(f)
    streams = [[(f, 600, 100), (base, 500, 200), (None, 100, 100)] for f in cases] + [[(base, 400, 100), (f, 500, 200), (None, 100, 100)] for f in cases]
    frames = np.stack([np.zeros(47) if f is None else f for st in streams for f, _, _ in st])
    m = [x[1] for st in streams for x in st]; fd = [x[2] for st in streams for x in st]
    nul = [x[0] is None for st in streams for x in st]
    start = np.arange(len(streams) + 1) * 3
    exp = []
    for u, st in enumerate(streams):
        o = oracle.OraclePlayer(22050, seed=u)
        for f, mm, ff in st:
            o.queue(f, mm, ff)
        exp.append(o.drain())
    assert sum(bool((e == 32000).any()) for e in exp) >= 6                     # the overflowing ones clip
    for layout in (-1, 2, 1, 0):
        bp = eng.BatchPlayer(22050, layout=layout)
        bp.setUtterances(start, frames, m, fd, None, nul, np.arange(len(streams)))
        info = bp.kernelInfo()
        bp.synthesize()
        for u in range(len(streams)):
            got = bp.read(u)
            assert np.array_equal(got, exp[u]), (layout, u, int(np.count_nonzero(got != exp[u])))
        bp.close()


def test_wild_batch_repeated_in_fresh_batches():
    """The same wild batch (NaN parameters: the coefficient code takes its device-library path, an out-of-line call) through fresh
    batch objects again and again, every layout and arithmetic mode: each run must equal the oracle.  Catches results that depend on
    what earlier launches left behind in scratch memory or registers -- round 2 had one (MODE_FAST, lane kernel: a nested out-of-line
    call from a divergent branch, ~70 % of the runs wrong in one or more utterances after a few launches)."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(2)
    batch = random_batch(rng, 1500, wild=True)
    exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=8)
    for rep in range(12):
        for layout in (0, 1):
            for mode in (0, 1):
                bp = eng.BatchPlayer(22050, mode=mode, layout=layout)
                bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], batch["seeds"])
                bp.synthesize()
                got, _ = bp.readAll()
                bad = np.flatnonzero(got != exp)
                assert len(bad) == 0, (rep, layout, mode, len(bad), sorted(set(int(x) for x in np.searchsorted(exp_start, bad, side="right") - 1))[:5])
                bp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,wild", [(11, False), (12, True)])
def test_coefficient_tracks_change_nothing(seed, wild):
    """Tracks and flat stages (klatt_tracks.h: the resonator coefficients and interpolated gains of every fade sample evaluated
    densely, one track per distinct fade, picked up by stages without a frame state machine) against the same batch without them: the PCM must be the same bytes, in
    both arithmetic modes, sorted and unsorted, with a track budget too small for the batch (then nothing is tracked), and with utterances
    repeated (shared tracks).  Random ragged timing: NULL frames anywhere (also first, also in a row), fades longer than
    their frame, 1-sample fades; wild: NaN "hold" parameters, whose utterances must stay untracked."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(seed)
    one = random_batch(rng, 700, quiet_fraction=0.15, wild=wild)
    # the same utterances again with other seeds: every fade of the second half has its track already
    batch = dict(frames=np.concatenate([one["frames"], one["frames"]]), min=np.concatenate([one["min"], one["min"]]),
                 fade=np.concatenate([one["fade"], one["fade"]]), index=np.concatenate([one["index"], one["index"]]),
                 isnull=np.concatenate([one["isnull"], one["isnull"]]),
                 frame_start=np.concatenate([one["frame_start"], one["frame_start"][1:] + one["frame_start"][-1]]),
                 seeds=np.concatenate([one["seeds"], one["seeds"] ^ np.uint32(0x5bd1e995)]))
    # and five of them forty more times each: runs of equally timed utterances that do not fill whole wavefronts, so the
    # lane packing ends wavefronts early (empty lanes) -- the PCM must not care (sort = 0 packs densely in the given order)
    extra = [u for u in range(5) for _ in range(40)]
    fs, parts = [int(batch["frame_start"][-1])], {k: [batch[k]] for k in ("frames", "min", "fade", "index", "isnull")}
    for u in extra:
        a0, a1 = int(one["frame_start"][u]), int(one["frame_start"][u + 1])
        for k in parts:
            parts[k].append(one[k][a0:a1])
        fs.append(fs[-1] + a1 - a0)
    batch = dict({k: np.concatenate(v) for k, v in parts.items()},
                 frame_start=np.concatenate([batch["frame_start"], np.array(fs[1:], np.int64)]),
                 seeds=np.concatenate([batch["seeds"], rng.integers(0, 2 ** 32, len(extra)).astype(np.uint32)]))
    n_utt = len(batch["seeds"])

    def run(mode, tracks, sort=1, budget=None):
        bp = eng.BatchPlayer(22050, mode=mode)
        bp.setOption("tracks", tracks)
        bp.setOption("direct", 0)      # (the direct stages have their own test: test_direct_stages_change_nothing)
        bp.setOption("sort", sort)
        if budget is not None:
            bp.setOption("track_budget_mb", budget)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], batch["seeds"])
        bp.synthesize()
        pcm, start = bp.readAll()
        info = bp.kernelInfo()
        bp.close()
        return pcm, start, info

    for mode in (0, 1):
        waves = {}
        ref_pcm, ref_start, info0 = run(mode, 0)
        assert info0["tracked_utterances"] == 0
        for sort, budget in ((1, None), (0, None), (1, 1)):
            pcm, start, info = run(mode, 1, sort, budget)
            assert np.array_equal(start, ref_start)
            assert np.array_equal(pcm, ref_pcm), "mode %d sort %d budget %s: %d samples differ" % (
                mode, sort, budget, int(np.count_nonzero(pcm != ref_pcm)))
            print("mode %d sort %d budget %s: %d of %d utterances tracked, %d tracks, %d MB" % (
                mode, sort, budget, info["tracked_utterances"], n_utt, info["tracks"], info["track_mbytes"]))
            if budget is None:
                assert info["tracked_utterances"] > n_utt // (4 if wild else 2)   # the noisy utterances with finite parameters
                # the second copy of every utterance shares the first one's tracks: at most one track per frame of the first
                assert info["tracks"] <= len(one["min"])
                waves[sort] = info["wavefronts"]
            else:
                assert info["tracked_utterances"] == 0                   # 1 MB holds the tracks of a few utterances only: all or nothing
            if budget is None and len(waves) == 2:
                assert waves[1] > waves[0]       # runs of equal timing end their wavefronts early: more wavefronts than the dense packing
            if wild:
                nan_utts = sum(1 for u in range(n_utt) if np.isnan(batch["frames"][batch["frame_start"][u]:batch["frame_start"][u + 1]]).any())
                assert nan_utts > 0 and info["tracked_utterances"] <= n_utt - nan_utts
    # and against the oracle, utterance by utterance
    exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=8)
    pcm, start, _ = run(0, 1)
    d = pcm.astype(np.int32) - exp.astype(np.int32)
    assert np.array_equal(start, exp_start) and np.abs(d).max() <= 1
    assert int(np.count_nonzero(d)) <= max(2, MAX_FLIPS_PER_M * total // 1000000 + 1)


@pytest.mark.gpu
def test_planning_threads_change_nothing(monkeypatch):
    """A large batch's tracks are planned in parts by several host threads (plan_tracks): the engine must make the same tracks and
    the same PCM as with one pass (SPEECHPLAYER_PLAN_THREADS=1).  16 384 sampleIpa utterances: 395 000 frames, above the threshold."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    b = workloads.make("cfg2", 16384)
    assert len(b["fade"]) > 200000
    got = {}
    for threads in ("1", "8"):
        monkeypatch.setenv("SPEECHPLAYER_PLAN_THREADS", threads)
        bp = eng.BatchPlayer(b["sr"])
        bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
        bp.synthesize()
        info = bp.kernelInfo()
        got[threads] = (bp.digest(), info["tracked_utterances"], info["tracks"], info["track_mbytes"])
        bp.close()
    assert got["1"] == got["8"] and got["1"][1] > 0


def test_text_input_without_espeak_fails_loudly():
    """speechPlayer_batch_setText needs eSpeak NG at run time; where it is absent the call fails with code 4 and a message that
    names the library, and the batch stays usable through the IPA path."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, ipa
    if ipa.textAvailable():
        pytest.skip("eSpeak NG is installed here")
    bp = eng.BatchPlayer(22050)
    with pytest.raises(RuntimeError) as e:
        bp.setText(["Hello, world."])
    assert "libespeak-ng" in str(e.value) and _native.last_error_code() == 4
    bp.setIpa(["həlˈoʊ"], clauseType=".")
    bp.synthesize()
    assert bp.totalSamples > 0
    bp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,wild", [(21, False), (22, True)])
def test_direct_stages_change_nothing(seed, wild):
    """The direct stages (klatt_direct.h: flat control, every fade sample's coefficients computed in place from per-frame records
    that klatt_seeds evaluates before the launch) against the stages with the frame state machine and against the tracked flat
    stages, on random ragged batches (NULL frames anywhere, fades longer than their frame, 1-sample fades and frames, vibrato,
    M = 0 frames; wild: NaN "hold" utterances, which must stay with the frame state machine).
    MODE_EXACT: the same bytes from all three.  MODE_FAST: the direct stages advance the coefficients by recurrences
    (re-seeded at every fade's first sample): held to the usual bar against the oracle, like every kernel."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(seed)
    batch = random_batch(rng, 900, quiet_fraction=0.15, wild=wild)
    n_utt = len(batch["seeds"])
    exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=8)

    def run(mode, tracks, direct, sort=1, lean=-1):
        bp = eng.BatchPlayer(22050, mode=mode)
        bp.setOption("tracks", tracks); bp.setOption("direct", direct); bp.setOption("sort", sort); bp.setOption("direct_lean", lean)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], batch["seeds"])
        bp.synthesize()
        pcm, start = bp.readAll()
        info = bp.kernelInfo()
        marks = [bp.getLastIndex(u) for u in range(0, n_utt, 37)]
        bp.close()
        assert np.array_equal(start, exp_start)
        return pcm.copy(), info, marks

    nan_utts = sum(1 for u in range(n_utt) if np.isnan(batch["frames"][batch["frame_start"][u]:batch["frame_start"][u + 1]]).any())
    for mode in (0, 1):
        legacy, info0, marks0 = run(mode, 0, 0)
        assert info0["direct_utterances"] == 0 and info0["tracked_utterances"] == 0
        # (lean: the direct stages two workgroups to a CU -- 8-sample hand-overs, 128 registers, no steady path; 0: one, 16-sample hand-overs)
        for tracks, direct, sort, lean in ((0, 2, 1, 0), (0, 2, 1, 1), (0, 2, 0, 0), (0, 2, 0, 1), (0, 1, 1, -1), (1, 2, 1, -1)):
            pcm, info, marks = run(mode, tracks, direct, sort, lean)
            assert marks == marks0
            if tracks == 0:
                assert info["tracked_utterances"] == 0 and info["direct_utterances"] > n_utt // (4 if wild else 2)
                assert info["direct_utterances"] <= n_utt - nan_utts
                assert info["scratch_bytes"] == 0 and info["direct"]
                lean_runs = lean == 1 or (lean == -1 and mode == 1)      # (the engine's choice: MODE_FAST takes the lean stages at every size, MODE_EXACT beyond two workgroups per CU)
                assert info["stage_parallel_chunk"] == (8 if lean_runs else 16) and info["vgprs"] <= (128 if lean_runs else 256)
            else:
                assert info["direct_utterances"] == 0 and info["tracked_utterances"] > 0      # every candidate got its tracks
            d = pcm.astype(np.int32) - exp.astype(np.int32)
            nbad = int(np.count_nonzero(d))
            print("seed %d wild %s mode %d tracks %d direct %d sort %d lean %d: %d direct, %d tracked of %d utterances; %d of %d samples differ from the oracle" % (
                seed, wild, mode, tracks, direct, sort, lean, info["direct_utterances"], info["tracked_utterances"], n_utt, nbad, total))
            if mode == 0 or tracks == 1:
                assert np.array_equal(pcm, legacy), "%d samples differ from the stages with the frame state machine" % int(np.count_nonzero(pcm != legacy))
            assert np.abs(d).max() <= 1 and nbad <= max(2, MAX_FLIPS_PER_M * total // 1000000 + 1)
            assert float(np.sqrt(np.mean((d / 32768.0) ** 2))) < RMS_TOL


@pytest.mark.gpu
def test_batch_in_which_nothing_is_shared_and_nothing_is_aligned():
    """BASELINE configs[2]'s utterances with every frame's duration and fade scaled by its own random factor AND every frame's
    formants by another (workloads.all_different: what 2048 different sentences in different voices look like to the kernels):
    with a track budget that such a batch exceeds at its real size (65 536 utterances: 57 GB of tracks; here 8 MB stand in for the
    4 GB) the engine sends them to the direct stages by itself; against the oracle utterance by utterance, both modes; index marks
    on every seventh frame against the oracle's."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    base = workloads.make("cfg2", 2048)
    b = workloads.all_different(base)
    b["index"] = np.where(np.arange(len(b["min"])) % 7 == 3, np.arange(len(b["min"]), dtype=np.int32) % 1000, -1).astype(np.int32)
    exp, exp_start, total = oracle.batch_synthesize(b["sr"], b, threads=8)
    ref_marks = oracle.batch_last_index(b["sr"], b, threads=8)
    for mode, lean in ((0, -1), (1, -1), (0, 1), (1, 1)):
        bp = eng.BatchPlayer(b["sr"], mode=mode)
        bp.setOption("track_budget_mb", 8)
        bp.setOption("direct_lean", lean)
        bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
        info = bp.kernelInfo()
        assert info["direct"] and info["direct_utterances"] == 2048 and info["tracked_utterances"] == 0 and info["scratch_bytes"] == 0, info
        # 32 workgroups: by itself the engine keeps MODE_EXACT at one workgroup per CU (the lean stages -- two per CU -- are what a launch of
        # more than two workgroups per CU takes); MODE_FAST takes the lean stages at every size
        assert info["stage_parallel_chunk"] == (8 if (lean == 1 or mode == 1) else 16), info
        bp.synthesize()
        pcm, start = bp.readAll()
        assert np.array_equal(start, exp_start)
        d = pcm.astype(np.int32) - exp.astype(np.int32)
        nbad = int(np.count_nonzero(d))
        print("all_different x 2048, mode %d lean %d: %d samples, %d differ from the oracle (max %d)" % (mode, lean, total, nbad, int(np.abs(d).max())))
        assert np.abs(d).max() <= 1 and nbad <= max(2, MAX_FLIPS_PER_M * total // 1000000 + 1)
        assert float(np.sqrt(np.mean((d / 32768.0) ** 2))) < RMS_TOL
        # index marks (reference src/frame.cpp:69, :117-119) against the oracle's own frame state machine
        assert [bp.getLastIndex(u) for u in range(2048)] == ref_marks.tolist()
        # the aligned parent batch without tracks: in MODE_EXACT it stays with the stages that run whole chunks on uniform paths
        # ("direct" = 1: by timing), in MODE_FAST the direct stages take it as well (their recurrences win there too)
        bp.setOption("tracks", 0)
        bp.setUtterances(base["frame_start"], base["frames"], base["min"], base["fade"], base["index"], base["isnull"], base["seeds"])
        if mode == 0:
            assert bp.kernelInfo()["direct_utterances"] == 0
        else:
            assert bp.kernelInfo()["direct_utterances"] > 0
        bp.close()
    # the residency the engine picks by itself (direct_lean(), klatt_engine.hip): MODE_EXACT keeps one workgroup per CU up to two
    # workgroups' worth per CU (a launch that short lasts as long as its longest utterance takes through ONE workgroup's pipeline) and
    # takes the lean stages beyond; planning alone is looked at here (nothing is launched)
    big = workloads.all_different(workloads.make("cfg2", 36864))
    for n_utt, want in ((32768, 16), (36864, 8)):
        part = big.slice(0, n_utt)
        bp = eng.BatchPlayer(big["sr"], mode=0)
        bp.setUtterances(part["frame_start"], part["frames"], part["min"], part["fade"], part["index"], part["isnull"], part["seeds"])
        info = bp.kernelInfo()
        assert info["direct"] and info["direct_utterances"] == n_utt and info["stage_parallel_chunk"] == want, (n_utt, info)
        bp.close()


@pytest.mark.gpu
def test_direct_stages_long_fades_hold_the_recurrence_bound(ref):
    """MODE_FAST on the direct stages advances a moving resonator's pole by a constant complex factor per fade sample, re-seeded at
    every fade's first sample: the relative error of a coefficient is bounded by ~4 F 2^-53 after F samples (klatt_direct.h).  The
    longest fades of speech are ~1500 samples; here fades of 350 000 samples (16 s; every formant, bandwidth and gain moving, the
    nasal pair included) -- bound 1.6e-10 -- against the oracle at the usual bar, in both modes, with a short fade in front and a
    one-sample fade behind (the recurrences must stop on the fade's last sample and start again exactly)."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(41)
    frames, mins, fades, nul, start, seeds = [], [], [], [], [0], []
    for u in range(24):
        def vowel():
            f = np.zeros(47)
            f[0] = rng.uniform(80, 300); f[46] = f[0] * rng.uniform(0.8, 1.3)
            f[5] = rng.uniform(0.3, 1); f[3] = rng.uniform(0, 0.3); f[4] = rng.uniform(0, 1); f[6] = rng.uniform(0, 0.5); f[24] = rng.uniform(0, 1)
            f[7:13] = np.sort(rng.uniform(200, 5200, 6)); f[13] = rng.uniform(200, 600); f[14] = rng.uniform(200, 500)
            f[15:23] = rng.uniform(40, 900, 8); f[23] = rng.uniform(0, 1)
            f[25:31] = np.sort(rng.uniform(200, 5200, 6)); f[31:37] = rng.uniform(40, 900, 6); f[37:43] = rng.uniform(0, 1, 6)
            f[43] = rng.uniform(0, 1); f[44] = rng.uniform(0.2, 1.2); f[45] = rng.uniform(0.3, 2)
            return f
        seq = [(vowel(), 800, 120, 0), (vowel(), int(rng.integers(1, 400000)), 350000 + int(rng.integers(0, 999)), 0), (vowel(), 3, 1, 0), (np.zeros(47), 500, 300, 1)]
        for f, m, fd, n in seq:
            frames.append(f); mins.append(m); fades.append(fd); nul.append(n)
        start.append(start[-1] + len(seq)); seeds.append(1000 + u)
    batch = dict(frames=np.array(frames), min=np.array(mins, np.uint32), fade=np.array(fades, np.uint32), index=np.full(len(mins), -1, np.int32),
                 isnull=np.array(nul, np.uint8), frame_start=np.array(start, np.int64), seeds=np.array(seeds, np.uint32))
    exp, exp_start, total = oracle.batch_synthesize(22050, batch, threads=8)
    for mode, lean in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bp = eng.BatchPlayer(22050, mode=mode)
        bp.setOption("tracks", 0); bp.setOption("direct", 2); bp.setOption("direct_lean", lean)
        bp.setUtterances(batch["frame_start"], batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], batch["seeds"])
        assert bp.kernelInfo()["direct_utterances"] == 24
        bp.synthesize()
        pcm, st = bp.readAll()
        bp.close()
        assert np.array_equal(st, exp_start)
        d = pcm.astype(np.int32) - exp.astype(np.int32)
        nbad = int(np.count_nonzero(d))
        print("long fades, mode %d lean %d: %d samples, %d differ from the oracle (max %d)" % (mode, lean, total, nbad, int(np.abs(d).max())))
        assert np.abs(d).max() <= 1 and nbad <= max(2, MAX_FLIPS_PER_M * total // 1000000 + 1)
        assert float(np.sqrt(np.mean((d / 32768.0) ** 2))) < RMS_TOL


@pytest.mark.gpu
def test_pcm_delivery_paths_agree():
    """The ways PCM leaves a batch give the same bytes: per utterance (speechPlayer_batch_read, straight out of the padded pool), readAll
    into pageable memory (dense order made on the device by pcm_compact, bounce buffers), readAll into page-locked memory
    (speechPlayer_hostAlloc: one DMA), readAllAsync + readWait with another launch queued behind it -- on a ragged batch with utterances
    of zero frames, of one sample, of odd lengths (dense starts at every alignment), with the frames themselves handed over in
    page-locked memory; and a batch that was never launched still reads as nothing."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(77)
    batch = random_batch(rng, 500, quiet_fraction=0.2)
    # utterances without frames in between (length 0), and a tail of very short ones
    fs = batch["frame_start"].tolist()
    fs = fs[:100] + [fs[100]] * 3 + fs[100:]            # three empty utterances after the 100th
    seeds = np.concatenate([batch["seeds"][:100], np.array([1, 2, 3], np.uint32), batch["seeds"][100:]])
    n_utt = len(fs) - 1
    frames_pinned = eng.host_array(batch["frames"].shape, np.float64)
    frames_pinned[...] = batch["frames"]
    bp = eng.BatchPlayer(22050)
    bp.setUtterances(fs, frames_pinned, batch["min"], batch["fade"], batch["index"], batch["isnull"], seeds)
    total = bp.totalSamples
    lens = np.array([bp.utteranceSamples(u) for u in range(n_utt)])
    assert (lens == 0).sum() >= 3 and (lens % 2 == 1).any() and (lens % 8 != 0).any()
    never, st0 = bp.readAll()
    assert len(never) == 0                                # nothing synthesised yet
    bp.synthesize()
    pageable, starts = bp.readAll()
    assert len(pageable) == total and np.array_equal(np.diff(starts), lens)
    for u in list(range(0, n_utt, 7)) + [100, 101, 102, n_utt - 1]:
        assert np.array_equal(bp.read(u), pageable[starts[u]:starts[u + 1]]), u
    pinned = eng.host_array(total + 5, np.int16)
    pinned[...] = 0x5555
    got, starts2 = bp.readAll(out=pinned)
    assert np.array_equal(starts2, starts) and np.array_equal(got, pageable) and (pinned[total:] == 0x5555).all()
    # asynchronously, with the next launch of the same batch queued right behind the read (the pool is rewritten with the same bytes)
    pinned[...] = 0
    got, starts3 = bp.readAllAsync(pinned)
    bp.synthesize(wait=False)
    bp.readWait()
    bp.wait()
    assert np.array_equal(starts3, starts) and np.array_equal(got, pageable)
    # the same frames from pageable memory: the same batch
    bq = eng.BatchPlayer(22050)
    bq.setUtterances(fs, batch["frames"], batch["min"], batch["fade"], batch["index"], batch["isnull"], seeds)
    bq.synthesize()
    assert bq.digest() == bp.digest()
    # ... and the same PLAN: page-locked frames are classified and hashed on the device (klatt_frame_facts), pageable ones by the host's
    # threads (klatt_plan.h, the same function): groups, tracks and direct utterances must come out alike
    assert bq.kernelInfo() == bp.kernelInfo()
    with pytest.raises(RuntimeError):
        bq.readAllAsync(np.zeros(total, np.int16))        # not page-locked
    bq.close(); bp.close()


@pytest.mark.gpu
def test_eight_shards_of_a_node_sized_share():
    """What the driver's 8-GPU run does to BASELINE configs[3], rehearsed on one device: the per-GPU share (125 000 short utterances)
    as ONE batch and as a NodePlayer of EIGHT shards (eight Batch objects, eight streams, eight planning threads on device 0): the
    deal is the Python helper's, balanced within 0.1 % of the samples, and every utterance's PCM digest and a strided sample of the
    index marks equal the single batch's.  (Nothing above three shards had ever run before round 5.)"""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    from nvspeechplayer_amd.sharding import shard_bounds
    b = workloads.make("cfg3", 125000)
    n = b.n_utt
    b["index"] = np.where(np.arange(len(b["min"])) % 5 == 2, np.arange(len(b["min"]), dtype=np.int32) % 997, -1).astype(np.int32)
    one = eng.BatchPlayer(b["sr"])
    one.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
    one.synthesize()
    _, ref = one.digest(per_utterance=True)
    node = eng.NodePlayer(b["sr"], [0] * 8)
    node.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
    assert node.totalSamples == one.totalSamples
    sh = node.shards()
    lens = b.sample_counts()
    assert len(sh) == 8 and [a for a, _, _, _ in sh] + [n] == list(shard_bounds(lens, 8))
    shares = np.array([s for _, _, s, _ in sh], dtype=np.float64)
    assert shares.sum() == lens.sum() and (shares.max() - shares.min()) / shares.mean() < 1e-3
    node.synthesize()
    got = node.digests()
    assert np.array_equal(got, ref), "%d utterances differ" % int(np.count_nonzero(got != ref))
    for u in range(0, n, 1237):
        assert node.getLastIndex(u) == one.getLastIndex(u), u
    for u in (0, sh[3][0], sh[3][0] - 1, n - 1):          # across a shard boundary: the PCM itself
        assert np.array_equal(node.read(u), one.read(u)), u
    node.close(); one.close()


@pytest.mark.gpu
def test_frame_facts_device_equals_host():
    """klatt_frame_facts (what frames that arrive by DMA from page-locked memory are classified and hashed by) against the host's
    evaluation of the same function (csrc/klatt_plan.h) on frames with every kind of trouble: the same 24 bytes per frame."""
    from tests.test_track_planning import facts_frames, frame_facts
    f = facts_frames(np.random.default_rng(10), 50000)
    for sr in (22050, 8000):
        host, dev = frame_facts(f, sr, 0), frame_facts(f, sr, 1)
        assert np.array_equal(host["flags"], dev["flags"]) and np.array_equal(host["h0"], dev["h0"]) and np.array_equal(host["h1"], dev["h1"])
