"""Shared parity scenarios: frame streams + the call sequence that plays them.

A scenario is a list of operations against the speechPlayer C-ABI, in SAMPLES:
    ("q", frame[47] | None, minSamples, fadeSamples, userIndex, purge)
    ("s", n)         one synthesize(n) call
    ("drain",)       synthesize(8192) until a short count
It can be played on the oracle (play_oracle) or on the HIP engine (tests do that
through the product C-ABI) and the PCM / index marks compared call by call.

Inputs come from tests/golden/ref_frames.npz, i.e. from the reference's own frame
producer (see tests/golden/make_golden.py); the call recipes follow the
reference's demo scripts, cited per scenario.
"""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SR = 22050

# parameter indices (frame.h:24-42)
VOICEPITCH, VIBOFFSET, VIBSPEED, TURB, OPENQ, VOICEAMP, ASPAMP = range(7)
CANP, FRICAMP, BYPASS, PREGAIN, OUTGAIN, ENDPITCH = 23, 24, 43, 44, 45, 46


def ms(x, sr=SR):
    """speechPlayer.py:53 ms -> samples (truncation)."""
    return int(x * (sr / 1000.0))


class Ref:
    def __init__(self, path=None):
        z = np.load(path or os.path.join(GOLDEN, "ref_frames.npz"))
        self.names = [b.decode("utf8") for b in z["phoneme_names"]]
        self.frames = z["phoneme_frames"]
        self.mask = z["phoneme_mask"].astype(bool)
        self.field_names = [b.decode() for b in z["field_names"]]
        self.is_vowel = z["phoneme_isVowel"].astype(bool)
        self.is_voiced = z["phoneme_isVoiced"].astype(bool)
        self.voiced_order = z["voiced_order"]
        self.ipa_meta = z["ipa_case_meta"]
        self.ipa_frames = z["ipa_frames"]
        self.ipa_isnull = z["ipa_isnull"]
        self.ipa_dur_ms = z["ipa_dur_ms"]
        self.ipa_fade_ms = z["ipa_fade_ms"]
        self.ipa_start = z["ipa_start"]

    def phoneme(self, name):
        return self.frames[self.names.index(name)].copy()

    def set_frame(self, frame, name):
        """ipa.setFrame (ipa.py:29-32): overwrite the fields the phoneme entry defines."""
        i = self.names.index(name)
        frame[self.mask[i]] = self.frames[i][self.mask[i]]
        return frame

    def vowels(self):
        return [n for n, v in zip(self.names, self.is_vowel) if v]

    def ipa_case(self, i, sr=SR):
        """-> list of (frame|None, M, F) incl. the trailing NULL(150 ms, 0) of test_speakIpa.py:27."""
        a, b = self.ipa_start[i], self.ipa_start[i + 1]
        out = []
        for k in range(a, b):
            fr = None if self.ipa_isnull[k] else self.ipa_frames[k].copy()
            out.append((fr, ms(self.ipa_dur_ms[k], sr), ms(self.ipa_fade_ms[k], sr)))
        out.append((None, ms(150, sr), 0))
        return out

    def find_ipa(self, line, speed=1.0, clause=0, pitch=100.0, infl=0.5):
        for i, m in enumerate(self.ipa_meta):
            if int(m[0]) == line and m[1] == speed and int(m[2]) == clause and m[3] == pitch and m[4] == infl:
                return i
        raise KeyError((line, speed, clause, pitch, infl))


def vowel_frame(ref, name, pitch, end_pitch=None, out_gain=1.0):
    """test_playVowelchart.py:27-30 + ipa.setFrame."""
    f = np.zeros(47)
    f[PREGAIN] = 1.0
    f[VOICEAMP] = 1.0
    f[OUTGAIN] = out_gain
    ref.set_frame(f, name)
    f[VOICEPITCH] = pitch
    f[ENDPITCH] = pitch if end_pitch is None else end_pitch
    return f


def q(frame, m, f, index=-1, purge=False):
    return ("q", None if frame is None else np.asarray(frame, dtype=np.float64), int(m), int(f), int(index), bool(purge))


class Scenario:
    def __init__(self, name, ops, sr=SR, seed=0, batchable=False):
        self.name, self.ops, self.sr, self.seed, self.batchable = name, ops, sr, seed, batchable

    def frames(self):
        """(frames[n,47], min, fade, index, isnull) of the queue ops (batchable scenarios)."""
        fr, m, f, ix, nu = [], [], [], [], []
        for op in self.ops:
            if op[0] == "q":
                assert not op[5]
                fr.append(np.zeros(47) if op[1] is None else op[1])
                m.append(op[2]); f.append(op[3]); ix.append(op[4]); nu.append(op[1] is None)
        return (np.array(fr).reshape(-1, 47), np.array(m, np.uint32), np.array(f, np.uint32),
                np.array(ix, np.int32), np.array(nu, np.uint8))


def build_scenarios(ref):
    sc = []
    # cfg0: SURVEY 8(c) recipe == test_playVowelchart.py frame set-up, /a/ at 120 Hz, 1 s
    fa = vowel_frame(ref, "a", 120.0)
    sc.append(Scenario("cfg0_a_1s", [q(fa, ms(1000), ms(50)), ("s", 22050), ("s", 22050)], batchable=False))
    sc.append(Scenario("cfg0_a_1s_batch", [q(fa, ms(1000), ms(50)), ("drain",)], batchable=True))

    # steady vowels (BASELINE cfg1 recipe at 0.25 s): every vowel at three pitches
    for vi, v in enumerate(ref.vowels()):
        for pi, pitch in enumerate((80.0, 163.5, 320.0)):
            f = vowel_frame(ref, v, pitch)
            sc.append(Scenario("vowel_%02d_p%d" % (vi, pi),
                               [q(f, ms(250), ms(50)), q(None, ms(50), ms(50)), ("drain",)], batchable=True))

    # sampleIpa.txt through the reference frame producer (test_speakIpa.py:25-27)
    for i in range(len(ref.ipa_meta)):
        ops = [q(fr, m, f) for (fr, m, f) in ref.ipa_case(i)]
        ops.append(("drain",))
        li, speed, clause, pitch, infl = ref.ipa_meta[i]
        sc.append(Scenario("ipa_l%d_s%02d_c%d_p%d_i%02d" % (li, speed * 10, clause, pitch, infl * 10), ops,
                           seed=1000 + i, batchable=True))

    # the same line pulled in uneven chunks (streaming contract, __init__.py:67)
    i0 = ref.find_ipa(2)
    ops = [q(fr, m, f, index=k) for k, (fr, m, f) in enumerate(ref.ipa_case(i0))]
    for n in (8192, 1, 77, 1000, 64, 63, 65, 4096):
        ops.append(("s", n))
    ops.append(("drain",))
    sc.append(Scenario("stream_chunks", ops, seed=7))

    # purge during steady state and during a fade, drain, then resume (frame.cpp:103-112;
    # test_midiSing.py:105-132 usage pattern)
    fs = vowel_frame(ref, "s", 110.0); fz = vowel_frame(ref, "z", 130.0, 90.0)
    fm = vowel_frame(ref, "m", 100.0, 140.0); fi = vowel_frame(ref, "i", 200.0, 100.0)
    ops = [q(fa, 4000, 500, index=1), q(fs, 3000, 800, index=2), q(fz, 3000, 800, index=3), ("s", 3000),
           q(fm, 2500, 600, index=4, purge=True), ("s", 300),       # purge in steady state of fa
           q(fi, 2000, 700, index=5, purge=True), ("s", 2500),      # purge inside the fade into fm
           q(None, 500, 300, index=6), ("drain",),
           q(fz, 1500, 200, index=7), q(None, 0, 441, index=-1, purge=True), ("s", 100), ("drain",),
           q(fs, 1200, 100, index=8), q(None, 300, 300), ("drain",)]
    sc.append(Scenario("purge_resume", ops, seed=11))

    # vowel-chart demo call pattern (test_playVowelchart.py:32-44)
    voiced = [ref.names[i] for i in ref.voiced_order]
    ops = []
    for a, b in ((voiced[0], voiced[5]), (voiced[9], voiced[20]), (voiced[30], voiced[3])):
        ops.append(q(None, 0, ms(20), purge=True))
        ops.append(q(vowel_frame(ref, a, 40.0, 300.0), ms(300), ms(50)))
        ops.append(q(vowel_frame(ref, b, 300.0, 40.0), ms(500), ms(400)))
        ops.append(q(None, ms(50), ms(50)))
        ops.append(("s", 9000))
    ops.append(("drain",))
    sc.append(Scenario("vowelchart_pairs", ops, seed=3))

    # vibrato + breathiness + open quotient (test_sayHannah.py:14-30, test_midiSing.py:60-61)
    def hannah(name, pitch, amp=1.0):
        f = vowel_frame(ref, name, pitch)
        f[VIBOFFSET] = 0.1; f[VIBSPEED] = 5.5; f[VOICEAMP] = amp
        f[TURB] = 0.3; f[OPENQ] = 0.4
        return f
    ops = [q(hannah("æ", 150.0, 0.0), ms(120), ms(100)), q(hannah("æ", 150.0), ms(120), ms(40)),
           q(hannah("n", 100.0), ms(120), ms(40)), q(hannah("ɑ", 90.0), ms(80), ms(40)),
           q(None, ms(40), ms(40)), ("drain",)]
    sc.append(Scenario("hannah_vibrato", ops, seed=5, batchable=True))

    # NaN means "hold the previous value" (utils.h:21)
    fn = vowel_frame(ref, "u", 140.0, 100.0)
    for k in (8, 16, 26, 38, BYPASS, OUTGAIN, VIBSPEED):
        fn[k] = np.nan
    ops = [q(vowel_frame(ref, "e", 120.0), 2000, 400), q(fn, 3000, 1500), q(vowel_frame(ref, "o", 90.0), 1500, 300),
           q(None, 400, 400), ("drain",)]
    sc.append(Scenario("nan_hold", ops, seed=9, batchable=True))

    # duration edge cases: fade longer than the frame, zero fade (clamped to 1), zero-length silences
    ops = [q(None, 0, 0), q(fa, 10, 2000), q(fs, 1, 1), q(fz, 2, 0), q(None, 0, 50), q(fm, 700, 699),
           q(fi, 700, 700), q(fa, 700, 701), q(None, 1, 1), ("drain",)]
    sc.append(Scenario("duration_edges", ops, seed=13, batchable=True))

    # 16 kHz, the NVDA driver's rate (__init__.py:137,144)
    i1 = ref.find_ipa(0)
    ops = [q(fr, m, f) for (fr, m, f) in ref.ipa_case(i1, sr=16000)] + [("drain",)]
    sc.append(Scenario("ipa_l0_16k", ops, sr=16000, seed=21, batchable=True))

    # other sample rates the C-ABI accepts (reference src/speechPlayer.cpp:25-32 takes any): everything that depends on the rate --
    # the resonator coefficients, the phase increments, ms -> samples, the tracks' evaluation -- at 44.1 kHz and at 8 kHz
    # (at 8 kHz the upper formants lie beyond the Nyquist frequency: the coefficients simply follow the formulas)
    for sr, line, seed in ((44100, 1, 23), (8000, 3, 25)):
        ops = [q(fr, m, f) for (fr, m, f) in ref.ipa_case(ref.find_ipa(line), sr=sr)] + [("drain",)]
        sc.append(Scenario("ipa_l%d_%dk" % (line, sr // 1000), ops, sr=sr, seed=seed, batchable=True))
        fv = vowel_frame(ref, "ɑ", 110.0, 170.0); fv[VIBOFFSET] = 0.1; fv[VIBSPEED] = 5.5
        ops = [q(fv, ms(180, sr), ms(40, sr)), q(vowel_frame(ref, "s", 120.0), ms(90, sr), ms(30, sr)),
               q(vowel_frame(ref, "m", 100.0, 90.0), ms(120, sr), ms(50, sr)), q(None, ms(40, sr), ms(40, sr)), ("drain",)]
        sc.append(Scenario("vowel_fric_nasal_%dk" % (sr // 1000), ops, sr=sr, seed=seed + 1, batchable=True))

    # a pole pair that GROWS right after a silence (found by tests/test_gpu_reference.py; queue calls 1 .. 4 of fuzz_sequence(36, extreme)
    # at 8 kHz): a frame, a silence of 1842 samples, a 2-sample frame with a parallel bandwidth of -3.2e5 Hz (r = e^127 per sample),
    # a frame that fades back.  The silence's fade takes preFormantGain to exactly 0 (frame.cpp:61, utils.h:22), so what the growing
    # pair amplifies to full scale is the filters' own ring-down; a gain that ends 1e-17 beside 0 shows as samples of the other sign
    fz36 = fuzz_sequence(36, True)
    ops = [op[:5] + (False,) for op in fz36.ops if op[0] == "q"][1:5] + [("drain",)]
    sc.append(Scenario("growing_pole_after_silence", ops, sr=fz36.sr, seed=fz36.seed, batchable=True))
    return sc


def play(scn, p):
    """Play a scenario on a player with the oracle's call surface (tests/oracle.py, tests/reference.py) and close it.
    -> (list of int16 arrays, one per synth/drain op; list of lastIndex after each such op)"""
    pcm, marks = [], []
    for op in scn.ops:
        if op[0] == "q":
            p.queue(op[1], op[2], op[3], op[4], op[5])
        elif op[0] == "s":
            pcm.append(p.synthesize(op[1])); marks.append(p.last_index())
        else:
            pcm.append(p.drain()); marks.append(p.last_index())
    p.close()
    return pcm, marks


def play_oracle(scn):
    from tests import oracle
    return play(scn, oracle.OraclePlayer(scn.sr, noise=oracle.NOISE_COUNTER, seed=scn.seed))


def random_batch(rng, n_utt, quiet_fraction=0.3, wild=False, nasal_fraction=0.4):
    """Ragged random utterances: random formants / bandwidths / gains / pitches, random durations
    (including fade > frame, fade 0, 1-sample frames), NULL frames anywhere, optional NaN holds."""
    frames, mins, fades, nul, start, seeds = [], [], [], [], [0], []
    for u in range(n_utt):
        n = int(rng.integers(1, 9))
        quiet = rng.random() < quiet_fraction
        prev_real = False
        for k in range(n):
            f = np.zeros(47)
            f[0] = rng.uniform(40, 400); f[46] = f[0] * rng.uniform(0.6, 1.6)
            if rng.random() < 0.3:
                f[1] = rng.uniform(0, 0.2); f[2] = rng.uniform(0, 8)
            f[5] = rng.uniform(0, 1)
            if not quiet:
                f[3] = rng.uniform(0, 0.5) * (rng.random() < 0.5); f[4] = rng.uniform(0, 1)
                f[6] = rng.uniform(0, 1) * (rng.random() < 0.5); f[24] = rng.uniform(0, 1) * (rng.random() < 0.6)
            f[7:13] = np.sort(rng.uniform(150, 5500, 6)); f[13] = rng.uniform(0, 600) * (rng.random() < 0.5); f[14] = rng.uniform(200, 500)
            f[15:23] = rng.uniform(30, 1000, 8); f[23] = rng.uniform(0, 1) * (rng.random() < nasal_fraction)
            f[25:31] = np.sort(rng.uniform(150, 5500, 6)); f[31:37] = rng.uniform(30, 1000, 6); f[37:43] = rng.uniform(0, 1, 6)
            f[43] = rng.uniform(0, 1); f[44] = rng.uniform(0, 1.5); f[45] = rng.uniform(0.2, 2.5)
            is_null = rng.random() < 0.2
            if wild and prev_real and not is_null and rng.random() < 0.3:
                f[rng.integers(1, 46, size=3)] = np.nan          # "hold" semantics (utils.h:21); only where a value exists to hold
            prev_real = not is_null
            frames.append(f); nul.append(is_null)
            mode = rng.integers(0, 5)
            if mode == 0: m, fd = int(rng.integers(0, 4)), int(rng.integers(0, 4))
            elif mode == 1: m, fd = int(rng.integers(1, 300)), int(rng.integers(300, 900))       # fade longer than the frame
            else: m, fd = int(rng.integers(50, 2500)), int(rng.integers(0, 700))
            if not is_null and m == 0 and not (wild and rng.random() < 0.25):
                m = 1                                           # M = 0 on a real frame divides by zero (frame.cpp:98: an infinite or NaN pitch,
                                                                # samples of 32000): in the wild batches only, and there on one such frame in four
            mins.append(m); fades.append(fd)
        start.append(start[-1] + n); seeds.append(int(rng.integers(0, 2 ** 32)))
    return dict(frames=np.array(frames), min=np.array(mins, np.uint32), fade=np.array(fades, np.uint32),
                index=np.full(len(mins), -1, np.int32), isnull=np.array(nul, np.uint8), frame_start=np.array(start, np.int64),
                seeds=np.array(seeds, np.uint32))


STORED_PCM = ("cfg0_a_1s", "stream_chunks", "purge_resume", "vowelchart_pairs", "hannah_vibrato", "nan_hold",
              "duration_edges", "ipa_l0_16k", "ipa_l1_44k", "ipa_l3_8k", "vowel_fric_nasal_44k", "vowel_fric_nasal_8k", "growing_pole_after_silence")


def write_expected_pcm(ref_path, outdir):
    """Called by make_golden.py: expected PCM (oracle, counter noise) for every scenario as SHA-1 +
    length, and the full PCM for a small subset."""
    ref = Ref(ref_path)
    table, store = {}, {}
    for scn in build_scenarios(ref):
        pcm, marks = play_oracle(scn)
        flat = np.concatenate(pcm) if pcm else np.zeros(0, np.int16)
        table[scn.name] = {"sha1": hashlib.sha1(flat.tobytes()).hexdigest(), "samples": int(len(flat)),
                           "calls": [int(len(x)) for x in pcm], "marks": [int(m) for m in marks]}
        if scn.name in STORED_PCM or (scn.name.startswith("ipa_") and "_s10_c0_p100_i05" in scn.name):
            store[scn.name] = flat
    with open(os.path.join(outdir, "expected.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(outdir, "expected_pcm.npz"), **store)
    print("expected.json: %d scenarios; expected_pcm.npz: %d stored" % (len(table), len(store)))


# ---- fuzzed call sequences (tests/test_reference_pin.py, tests/test_gpu_reference.py) --------------------------------------------
# either side of every hand-over size the kernels use
FUZZ_PULLS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 500, 1000, 4096, 8192)
FUZZ_RATES = (8000, 11025, 16000, 22050, 44100, 48000)
N0_EDGE = (0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308)     # the anti-resonator's `f != 0` (speechWaveGenerator.cpp:120)
EXTREME_KINDS = ("neg_cascade_bw", "neg_parallel_bw", "inf", "n0_zero", "gain", "beyond_nyquist", "n0_edge")
PURGE_KINDS = ("fade_first", "fade_last", "frame_end", "drained", "boundary_in_fade")
N_FUZZ = 400        # sequences of each variant the CPU pin plays (seeds 0 .. N_FUZZ-1)


def fuzz_sequence(seed, extreme=False, n_utt=40):
    """One seeded call sequence against the five entry points, as a Scenario (its .kinds: the extreme kinds it holds).
    Frames as random_batch(wild=True) draws them, each queued with a random user index and, one time in five, with purge; after it,
    one time in two, ONE synthesize(n) with n from FUZZ_PULLS, and one time in ten a drain -- so frames pile up in the queue, are
    purged out of it, and are queued onto drained handles.  One sample rate per sequence.  extreme: a real frame additionally gets,
    one time in ten each, a negative cascade bandwidth, a negative parallel bandwidth down to -3e6 (exp overflows: infinite
    coefficients), +-inf in any parameter, N0 frequency 0 with caNP 1, an output gain up to 1e6 (clipping), a formant beyond the
    Nyquist frequency up to 1e5 Hz, an N0 frequency from N0_EDGE with caNP > 0."""
    rng = np.random.default_rng([int(bool(extreme)), int(seed)])
    sr = int(rng.choice(FUZZ_RATES))
    # (one sequence in four has no noise source at all and every second of those no nasal branch either: what the batch planner
    # calls quiet and nasal-free, each with kernels of its own)
    b = random_batch(rng, n_utt, wild=True, quiet_fraction=1.0 if seed % 4 == 3 else 0.3, nasal_fraction=0.0 if seed % 8 == 7 else 0.4)
    ops, kinds = [], set()
    for k in range(len(b["min"])):
        fr = None if b["isnull"][k] else b["frames"][k].copy()
        if extreme and fr is not None:
            hit = rng.random(len(EXTREME_KINDS)) < 0.1
            u = rng.random(len(EXTREME_KINDS))
            j = rng.integers(0, 1 << 30, len(EXTREME_KINDS))
            if hit[0]: fr[15 + j[0] % 8] = -300.0 * u[0]
            if hit[1]: fr[31 + j[1] % 6] = -(10.0 ** (2.0 + u[1] * (np.log10(3e6) - 2.0)))
            if hit[2]: fr[j[2] % 47] = np.inf if u[2] < 0.5 else -np.inf
            if hit[3]: fr[13] = 0.0; fr[CANP] = 1.0
            if hit[4]: fr[OUTGAIN] = 10.0 ** (1.0 + 5.0 * u[4])
            if hit[5]: fr[(7, 25)[j[5] % 2] + (j[5] >> 1) % 6] = sr / 2.0 + u[5] * (1e5 - sr / 2.0)
            if hit[6]: fr[13] = N0_EDGE[j[6] % len(N0_EDGE)]; fr[CANP] = 0.1 + 0.9 * u[6]
            kinds.update(name for name, h in zip(EXTREME_KINDS, hit) if h)
        ops.append(q(fr, b["min"][k], b["fade"][k], index=int(rng.integers(-1, 1000)), purge=rng.random() < 0.2))
        if rng.random() < 0.5:
            ops.append(("s", int(rng.choice(FUZZ_PULLS))))
        if rng.random() < 0.1:
            ops.append(("drain",))
    ops.append(("drain",))
    scn = Scenario("fuzz_%s_%04d" % ("extreme" if extreme else "plain", seed), ops, sr=sr, seed=int(rng.integers(0, 2 ** 32)))
    scn.kinds = kinds
    return scn


def without_purges(scn):
    """(frames, min, fade, index, isnull) of a sequence's queue calls, the purges dropped: one utterance of a batch."""
    return Scenario(scn.name, [op[:5] + (False,) for op in scn.ops if op[0] == "q"], sr=scn.sr, seed=scn.seed, batchable=True).frames()


def trace_sequence(scn):
    """The frame state machine of frame.cpp:41-115 alone -- its sample counter, no parameters -- over a sequence's calls.
    -> (calls, kinds): the length of every synthesize / drain op, and how many purges arrived
      fade_first        right after the sample that took a request out of the queue, before the first interpolated sample of its fade
      fade_last         right after the last interpolated sample of a fade (counter == fade): the next sample would have ended it
      frame_end         in steady state on an event sample: right after the sample that ended a fade, or with the frame's time just
                        up (counter == min: the next sample takes a request), samples having been pulled since the last purge
      drained           on a handle whose last pull came back short and that has nothing queued
      boundary_in_fade  (counted per pull, not per purge) a pull that ends inside the fade of a frame that was queued with purge
    The calls are checked against the oracle's and the reference's (tests/test_reference_pin.py), so the counts stand on the same
    arithmetic as the PCM."""
    has_new = False; counter = 0; old_min = 0; new_min = new_fade = 0
    queue = []; drained = True; produced = 0; just_ended = False
    new_is_purge = False; pulled = False
    kinds = dict.fromkeys(PURGE_KINDS, 0)
    calls = []

    def advance(n):
        nonlocal pulled, has_new, counter, old_min, new_min, new_fade, drained, produced, just_ended, new_is_purge
        done = 0
        while done < n:
            if has_new:
                k = min(n - done, new_fade + 1 - counter)          # the sample with counter == fade + 1 ends the fade
                counter += k; done += k
                just_ended = False
                if counter > new_fade:
                    has_new = False; old_min = new_min; just_ended = True
            elif counter < old_min:
                k = min(n - done, old_min - counter)
                counter += k; done += k; just_ended = False
            else:
                counter += 1
                just_ended = False
                if not queue:
                    drained = True
                    break
                new_min, new_fade, new_is_purge = queue.pop(0)
                has_new = True; drained = False; counter = 0; done += 1
        produced += done
        pulled = pulled or done > 0
        return done

    for op in scn.ops:
        if op[0] == "q":
            m, f, purge = op[2], max(op[3], 1), op[5]
            if purge:
                if has_new and counter == 0:
                    kinds["fade_first"] += 1
                elif has_new and counter == new_fade:
                    kinds["fade_last"] += 1
                elif not has_new and not drained and pulled and (counter == old_min or just_ended):
                    kinds["frame_end"] += 1
                elif drained and not queue and produced:
                    kinds["drained"] += 1
                del queue[:]
                counter = old_min
                has_new = False; just_ended = False; pulled = False
            queue.append((m, f, purge))
        elif op[0] == "s":
            got = advance(op[1])
            calls.append(got)
            if got == op[1] and has_new and new_is_purge and 1 <= counter < new_fade:
                kinds["boundary_in_fade"] += 1
        else:
            total = 0
            while True:
                got = advance(8192)
                total += got
                if got < 8192:
                    break
                if has_new and new_is_purge and 1 <= counter < new_fade:
                    kinds["boundary_in_fade"] += 1
            calls.append(total)
    return calls, kinds


FREQ_BW = tuple(range(7, 23)) + tuple(range(25, 37))


def nudged(scn):
    """The sequence with every non-zero frequency and bandwidth one place up (zeros stay: `f != 0` is a branch)."""
    ops = []
    for op in scn.ops:
        if op[0] == "q" and op[1] is not None:
            fr = op[1].copy()
            v = fr[list(FREQ_BW)]
            fr[list(FREQ_BW)] = np.where(v != 0, np.nextafter(v, np.inf), v)
            op = op[:1] + (fr,) + op[2:]
        ops.append(op)
    return Scenario(scn.name, ops, sr=scn.sr, seed=scn.seed)


def admitted(scn, player):
    """Whether the device's last-place differences in exp / cos can be held to the parity bar on this sequence: decided on the CPU
    alone.  The sequence is played twice on `player` (oracle.OraclePlayer or reference.RefPlayer), the second time nudged();
    a filter that is unstable or cancels nearly completely amplifies that last place into the PCM, a sound one does not.
    -> (admitted, pcm per call, marks) of the sequence as it stands."""
    pcm, marks = play(scn, player(scn.sr, seed=scn.seed))
    pcm2, _ = play(nudged(scn), player(scn.sr, seed=scn.seed))
    return all(np.array_equal(a, b) for a, b in zip(pcm, pcm2)), pcm, marks


def sequence_digest(pcm, marks):
    """ONE SHA-1 over PCM bytes, call lengths and marks in order."""
    h = hashlib.sha1()
    for x, m in zip(pcm, marks):
        h.update(np.ascontiguousarray(x, dtype="<i2").tobytes())
        h.update(np.array([len(x), m], dtype="<i8").tobytes())
    return h.hexdigest()


def input_digest(scns):
    """SHA-1 of the generated frames and calls of a list of sequences: what the recorded outputs belong to."""
    h = hashlib.sha1()
    for scn in scns:
        h.update(np.array([scn.sr, scn.seed, len(scn.ops)], dtype="<i8").tobytes())
        for op in scn.ops:
            if op[0] == "q":
                h.update(b"n" if op[1] is None else np.ascontiguousarray(op[1], dtype="<f8").tobytes())
                h.update(np.array([op[2], op[3], op[4], op[5]], dtype="<i8").tobytes())
            else:
                h.update(np.array([-1 if op[0] == "drain" else op[1]], dtype="<i8").tobytes())
    return h.hexdigest()


REFERENCE_BATCHES = ((1, False), (2, True), (11, False), (12, True), (21, False), (22, True))    # the GPU parity tests' random_batch seeds


def batch_scenarios(seed, wild, n_utt=1500):
    """random_batch(seed) utterance by utterance, as drain-only scenarios."""
    b = random_batch(np.random.default_rng(seed), n_utt, wild=wild)
    out = []
    for u in range(n_utt):
        ops = [q(None if b["isnull"][k] else b["frames"][k], b["min"][k], b["fade"][k], b["index"][k])
               for k in range(b["frame_start"][u], b["frame_start"][u + 1])]
        out.append(Scenario("batch%d_%04d" % (seed, u), ops + [("drain",)], seed=int(b["seeds"][u])))
    return out


def group_digest(results):
    """One SHA-1 over the sequence digests of a group, in order."""
    return hashlib.sha1("".join(results).encode()).hexdigest()


def reference_table(player_of, ref=None, progress=None):
    """What `player_of(sr, seed)` answers on everything tests/golden/reference.json records, in that file's layout."""
    table = {"numpy": np.__version__, "scenarios": {}, "fuzz": {}, "batches": {}}
    for scn in build_scenarios(ref or Ref()):
        pcm, marks = play(scn, player_of(scn.sr, scn.seed))
        flat = np.concatenate(pcm) if pcm else np.zeros(0, np.int16)
        table["scenarios"][scn.name] = {"sha1": hashlib.sha1(flat.tobytes()).hexdigest(), "calls": [int(len(x)) for x in pcm],
                                        "marks": [int(m) for m in marks]}
    samples = sum(sum(v["calls"]) for v in table["scenarios"].values())
    for extreme in (False, True):
        scns = [fuzz_sequence(s, extreme) for s in range(N_FUZZ)]
        out = []
        for scn in scns:
            pcm, marks = play(scn, player_of(scn.sr, scn.seed))
            out.append(sequence_digest(pcm, marks)); samples += sum(len(x) for x in pcm)
        table["fuzz"]["extreme" if extreme else "plain"] = {"input": input_digest(scns), "sha1": out}
        if progress:
            progress("fuzz %s: %d samples so far" % ("extreme" if extreme else "plain", samples))
    for seed, wild in REFERENCE_BATCHES:
        scns = batch_scenarios(seed, wild)
        out = []
        for scn in scns:
            pcm, marks = play(scn, player_of(scn.sr, scn.seed))
            out.append(sequence_digest(pcm, marks)); samples += sum(len(x) for x in pcm)
        table["batches"]["%d" % seed] = {"wild": bool(wild), "input": input_digest(scns), "sha1": group_digest(out)}
    table["samples"] = int(samples)
    return table
