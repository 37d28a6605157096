"""The pitch export on the host (include/speechPlayer_batch.h: speechPlayer_pcmPitch, signalPitch; nvspeechplayer_amd.pcmPitch, signalPitch,
pitchLags, check_pitch_request, PITCH_FIELDS; csrc/klatt_pitch.h): a transcription of the definition written here in numpy and plain
Python, independent of the shared header, held to the statements bit for bit over the shapes at which the kernel's tiling changes; the
cases that can be worked out by hand; the estimate against the truth -- steady vowels of the CPU oracle whose frames state the period
exactly --; every refusal; and a model of the kernel's walk in a program of its own under the sanitizers (tests/native/check_pitch.cpp).
`t_pitch`, `vowel_pcm` and `inside_steps` are what tests/test_gpu_pitch.py shares.  No GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_lpc_host import bits, float_row, golden_pcm, segment, t_steps, t_x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
F32, F64 = np.float32, np.float64
ALL = 63
WINS = (32, 33, 34, 35, 2048)
LAG_MAXES = (3, 63, 64, 65, 1024)


# ---- the transcription of the definition, in numpy and plain Python --------------------------------------------------------------------------
def t_curve(f, W, lagMax):
    """m[0 .. lagMax] (m[0] unused) of one frame f[W + lagMax] of float32.  The product of two float32 values widened to binary64 is
    exact, so `chain + term` is the definition's single rounding without an fma."""
    tau = np.arange(1, lagMax + 1)
    u = f[:W, None] - f[np.arange(W)[:, None] + tau[None, :]]
    assert u.dtype == F32      # one binary32 subtraction
    term = u.astype(F64) * u.astype(F64)
    chain = np.zeros((4, lagMax))
    for i in range(W):      # ascending i; chain i mod 4
        chain[i % 4] = chain[i % 4] + term[i]
    d = (chain[0] + chain[1]) + (chain[2] + chain[3])
    m, s = [0.0] * (lagMax + 1), 0.0
    for t in range(1, lagMax + 1):
        s = s + float(d[t - 1])
        m[t] = (float(d[t - 1]) * float(t)) / s if s > 0 else 1.0
    return m


BRANCHES = {"edge": 0, "den": 0, "far": 0, "parabola": 0}


def t_choice(m, lagMin, lagMax, threshold):
    """(tau*, voiced, delta) of a curve."""
    star, voiced = None, False
    for t in range(lagMin, lagMax + 1):
        if m[t] < threshold and (t == lagMax or not m[t + 1] < m[t]):
            star, voiced = t, True
            break
    if star is None:
        star = lagMin
        for t in range(lagMin + 1, lagMax + 1):
            if m[t] < m[star]:
                star = t
    delta = 0.0
    if star - 1 >= 1 and star + 1 <= lagMax:
        y0, y1, y2 = m[star - 1], m[star], m[star + 1]
        den = (y0 - y1) + (y2 - y1)
        if den > 0:
            dd = (0.5 * (y0 - y2)) / den
            if abs(dd) <= 0.5:
                delta = dd
                BRANCHES["parabola"] += 1
            else:
                BRANCHES["far"] += 1
        else:
            BRANCHES["den"] += 1
    else:
        BRANCHES["edge"] += 1
    return star, voiced, delta


def t_pitch(row, rate, W, lagMin, lagMax, threshold, hop, phase, what):
    """float64 [steps, nCols] of a row of int16 or float32 samples."""
    x, L, N = t_x(row), len(row), W + lagMax
    steps = t_steps(L, hop, phase)
    nCols = sum(1 for b in range(5) if what >> b & 1) + (lagMax - lagMin + 1 if what & 32 else 0)
    out = np.zeros((steps, nCols))
    for j in range(steps):
        c = phase + j * hop
        f = np.zeros(N, F32)
        lo, hi = c - N // 2, c - N // 2 + N
        a, b = max(lo, 0), min(hi, L)
        if b > a:
            f[a - lo:b - lo] = x[a:b]
        m = t_curve(f, W, lagMax)
        star, voiced, delta = t_choice(m, lagMin, lagMax, threshold)
        period = float(star) + delta
        o = []
        if what & 1:
            o.append(float(rate) / period if voiced else 0.0)
        if what & 2:
            o.append(period)
        if what & 4:
            o.append(float(star))
        if what & 8:
            o.append(m[star])
        if what & 16:
            o.append(1.0 if voiced else 0.0)
        if what & 32:
            o.extend(m[lagMin:lagMax + 1])
        out[j] = o
    return out


def statement(row, rate, W, lagMin, lagMax, threshold, hop, phase, what):
    import nvspeechplayer_amd as eng
    fn = eng.pcmPitch if row.dtype == np.int16 else eng.signalPitch
    return fn(row, rate, nWin=W, lagMin=lagMin, lagMax=lagMax, threshold=threshold, hop=hop, phase=phase, fields=what)


def same(got, want, what):
    assert got.dtype == F64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


# ---- 1. the statements are the transcription -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lagMax", LAG_MAXES)
@pytest.mark.parametrize("W", WINS)
def test_the_statements_are_the_transcription(W, lagMax):
    """Golden PCM segments (a silence, an onset, voiced sound) and float rows made of them, both lagMin, rows shorter than a frame and of
    0 and 1 samples, phase > 0, hop 1 and N + 1; every field."""
    N = W + lagMax
    big = W == 2048 or lagMax == 1024
    for k, lagMin in enumerate(sorted({2, lagMax - 1})):
        name = ("ipa_l2_s10_c0_p100_i05", "ipa_l11_s10_c0_p100_i05")[k]
        far = segment(name, 3 * N + 40, lead=N // 3)      # three steps at hop N + 1
        near = segment(name, N // 2 + 9)                   # shorter than a frame
        rows = [(far, N + 1, 3 * k), (float_row(far), N + 1, 0)]
        if not big:
            rows += [(near[:40], 1, 2), (float_row(near), 7, 5 * k), (far[:N + 30], 1, N - 3)]
        else:
            rows += [(near, N + 1, 5)]
        rows += [(far[:0], 1, 0), (far[:1], 1, 0), (float_row(far[:1]), N + 1, 0), (far[:4], 3, 4)]
        for i, (row, hop, phase) in enumerate(rows):
            for threshold in ((0.1, 0.35)[i % 2],):
                want = t_pitch(row, 22050, W, lagMin, lagMax, threshold, hop, phase, ALL)
                same(statement(row, 22050, W, lagMin, lagMax, threshold, hop, phase, ALL), want, (W, lagMin, lagMax, i, hop, phase))


def test_fields_come_in_the_fixed_order():
    import nvspeechplayer_amd as eng
    row = segment("ipa_l15_s10_c0_p100_i05", 900, lead=300)
    kw = dict(nWin=64, lagMin=20, lagMax=65, threshold=0.3, hop=100, phase=3)
    every = eng.pcmPitch(row, 16000, fields=eng.PITCH_FIELDS, **kw)
    at, total = eng.pitchColumns(eng.PITCH_FIELDS, 20, 65)
    assert total == 5 + 46 == every.shape[1] and list(at) == eng.PITCH_FIELDS and at["cmnd"] == (5, 46) and at["voiced"] == (4, 1)
    for fields in (["aperiodicity", "f0"], "cmnd", ("voiced", "lag", "period"), 1 | 32, ["cmnd", "lag"]):
        got = eng.pcmPitch(row, 16000, fields=fields, **kw)
        where, n = eng.pitchColumns(fields, 20, 65)
        assert got.shape == (every.shape[0], n)
        for name, (col, count) in where.items():      # in PITCH_FIELDS' order whatever the order asked for
            assert np.array_equal(bits(got[:, col:col + count]), bits(every[:, at[name][0]:at[name][0] + count])), (fields, name)
    assert np.array_equal(eng.signalPitch(float_row(row), 16000, fields=ALL, **kw)[:, 1:], eng.signalPitch(float_row(row), 8000, fields=ALL, **kw)[:, 1:])      # the rate serves F0 alone


# ---- 2. by hand ----------------------------------------------------------------------------------------------------------------------------
def test_a_silent_row_is_unvoiced_at_lagmin():
    for row in (np.zeros(700, np.int16), np.zeros(700, F32), np.full(700, F32(-0.0))):
        got = statement(row, 22050, 128, 10, 80, 1.0, 100, 0, ALL)
        f0, period, lag, ap, voiced, curve = got[:, 0], got[:, 1], got[:, 2], got[:, 3], got[:, 4], got[:, 5:]
        assert got.shape == (7, 76) and np.all(voiced == 0) and np.all(lag == 10) and np.all(period == 10) and np.all(curve == 1.0) and np.all(ap == 1.0)
        assert np.all(f0 == 0) and not np.signbit(f0).any()


def periodic_row(P, L, seed=5):
    rng = np.random.default_rng(seed)
    return np.tile(rng.integers(-9000, 9000, P).astype(np.int16), L // P + 1)[:L]


def test_an_exactly_periodic_row():
    """d(P) = 0 exactly, so tau* = P with aperiodicity 0 wherever the frame lies inside the row.  With P the range's last lag the
    refinement has no right neighbour: delta = +0 and F0 = rate / P exactly.  Inside the range the parabola's neighbours m(P - 1) and
    m(P + 1) differ (the cumulative mean has grown by one lag), so delta is a small number, not 0: it is the transcription's."""
    P, W, rate = 57, 200, 22050
    row = periodic_row(P, 3000)
    for lagMax in (P, 130):
        N = W + lagMax
        got = statement(row, rate, W, 20, lagMax, 0.1, 64, 0, 31)
        inside = [j for j in range(len(got)) if j * 64 - N // 2 >= 0 and j * 64 - N // 2 + N <= len(row)]
        assert len(inside) > 20
        g = got[inside]
        assert np.all(g[:, 2] == P) and np.all(g[:, 3] == 0.0) and np.all(g[:, 4] == 1)      # P, not 2 P, although m(2 P) is 0 too
        if lagMax == P:
            assert np.all(g[:, 1] == P) and np.all(g[:, 0] == rate / P)
        else:
            assert np.all(np.abs(g[:, 1] - P) <= 0.5) and np.all(g[:, 0] == rate / g[:, 1])
            same(got, t_pitch(row, rate, W, 20, lagMax, 0.1, 64, 0, 31), "periodic")
    # threshold 0 never voices: m < 0 is never true.  The least m is 0 at P and at 2 P: the tie goes to the lower lag.
    got = statement(row, rate, W, 20, 130, 0.0, 64, 0, 31)[inside]
    assert np.all(got[:, 4] == 0) and np.all(got[:, 0] == 0) and np.all(got[:, 2] == P) and np.all(got[:, 3] == 0.0)
    # a threshold of 1 takes the first lag that is not above its right neighbour, whatever its height
    got = statement(row, rate, W, 20, 130, 1.0, 64, 0, ALL)[inside]
    for g in got:
        curve = g[5:]
        first = next(t for t in range(len(curve)) if curve[t] < 1.0 and (t == len(curve) - 1 or not curve[t + 1] < curve[t]))
        assert g[2] == 20 + first and g[4] == 1


def test_a_plateau_is_a_dip_and_ties_go_to_the_lowest_lag():
    """A row that is constant inside the frame: every d is 0, s never becomes positive, every m is 1.0 -- a plateau.  Below a threshold of
    1 nothing is voiced and the least m ties over the whole range: lagMin.  (m < 1.0 fails at threshold 1.0 too.)"""
    row = np.full(2000, 1234, np.int16)
    got = statement(row, 8000, 64, 7, 40, 1.0, 50, 0, 31)
    inside = [j for j in range(len(got)) if j * 50 - 52 >= 0 and j * 50 + 52 <= 2000]
    assert np.all(got[inside][:, 2] == 7) and np.all(got[inside][:, 4] == 0) and np.all(got[inside][:, 3] == 1.0) and np.all(got[inside][:, 1] == 7)


def test_the_refinements_three_fall_backs():
    """A sine of period 80.3 at threshold 1 with lagMin walked up the rising side of its dip: the first lag taken is lagMin itself, where
    the curve is convex and rising (the parabola's vertex lies more than half a lag away), then concave (den <= 0); lagMax == tau* is the
    range's edge.  Every branch is met, and the statement is the transcription on each."""
    for k in BRANCHES:
        BRANCHES[k] = 0
    t = np.arange(1500)
    row = np.round(9000 * np.sin(2 * np.pi * t / 80.3)).astype(np.int16)
    for lagMin in range(60, 150, 6):
        want = t_pitch(row, 22050, 160, lagMin, 170, 1.0, 700, 750, 31)
        same(statement(row, 22050, 160, lagMin, 170, 1.0, 700, 750, 31), want, lagMin)
    before = dict(BRANCHES)
    want = t_pitch(row, 22050, 160, 104, 116, 0.0, 700, 750, 31)      # unvoiced, the least m at lagMin on the concave rise towards 1.5 periods: den < 0
    assert BRANCHES["den"] > before["den"] and want[0, 2] == 104 and want[0, 1] == 104 and want[0, 4] == 0
    same(statement(row, 22050, 160, 104, 116, 0.0, 700, 750, 31), want, "concave")
    want = t_pitch(row, 22050, 160, 60, 80, 0.5, 700, 750, 31)      # the dip is the range's last lag
    assert want[0, 2] == 80 and want[0, 1] == 80
    same(statement(row, 22050, 160, 60, 80, 0.5, 700, 750, 31), want, "edge")
    assert all(v > 0 for v in BRANCHES.values()), BRANCHES


# ---- 3. against the truth --------------------------------------------------------------------------------------------------------------------
VOWELS, PITCHES, TRUTH_RATE, VOWEL_SAMPLES = ("a", "u"), (70.0, 100.0, 155.5, 220.0, 330.0, 470.0), 22050, 12000
_vowels = {}


def vowel_frames(vowel, pitch):
    """One steady vowel at a constant pitch: (frame, samples, fade)."""
    from tests import scenarios
    return scenarios.vowel_frame(scenarios.Ref(), vowel, pitch), VOWEL_SAMPLES, 200


def vowel_pcm(vowel, pitch):
    """The CPU oracle's PCM of it at 22050 Hz, synthesised once."""
    if (vowel, pitch) not in _vowels:
        from tests import oracle
        o = oracle.OraclePlayer(TRUTH_RATE, seed=1)
        o.queue(*vowel_frames(vowel, pitch))
        _vowels[vowel, pitch] = o.drain()[:VOWEL_SAMPLES].copy()
        o.close()
    return _vowels[vowel, pitch]


def inside_steps(L, W, lagMax, hop, margin=2000):
    """The steps whose frame lies `margin` samples inside a row of L samples."""
    N = W + lagMax
    return [j for j in range(t_steps(L, hop, 0)) if j * hop - N // 2 >= margin and j * hop - N // 2 + N <= L - margin]


def test_steady_vowels_against_the_truth(capsys):
    """Steady vowels a and u of the oracle at six constant pitches, 22050 Hz, W 512 and 1024, lags 44 .. 368, hop 256, threshold 0.1: every
    step whose frame lies 2000 samples inside the vowel is voiced and its period lies within half a sample of 22050 / pitch -- no worse than
    the best integer lag could be.  (Vowel i at 220 Hz is not here: its first dip below the threshold is a formant's, docs/KERNELS.md 4.25.)"""
    import nvspeechplayer_amd as eng
    worst = 0.0
    for vowel in VOWELS:
        for pitch in PITCHES:
            pcm = vowel_pcm(vowel, pitch)
            assert len(pcm) == VOWEL_SAMPLES and np.abs(pcm.astype(np.int32)).max() > 1000
            for W in (512, 1024):
                got = eng.pcmPitch(pcm, TRUTH_RATE, nWin=W, lagMin=44, lagMax=368, hop=256, threshold=0.1, fields=("period", "voiced", "f0"))
                steps = inside_steps(len(pcm), W, 368, 256)
                assert len(steps) >= 20
                err = np.abs(got[steps, 1] - TRUTH_RATE / pitch)      # the fields in PITCH_FIELDS' order: f0, period, voiced
                worst = max(worst, float(err.max()))
                print("pitch truth: vowel %s %.1f Hz W %d: worst %.4f sample over %d steps, voiced %d" % (vowel, pitch, W, err.max(), len(steps), int(got[steps, 2].sum())))
                assert np.all(got[steps, 2] == 1), (vowel, pitch, W)
                assert np.all(err <= 0.5), (vowel, pitch, W, float(err.max()))
                assert np.all(got[steps, 0] == TRUTH_RATE / got[steps, 1])      # F0 is rate / period
    with capsys.disabled():
        print("pitch truth: worst of all %.4f sample" % worst)


# ---- 4. the requests ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = (("speechPlayer_pcmPitch", 11), ("speechPlayer_signalPitch", 12), ("speechPlayer_batch_exportPitch", 14), ("speechPlayer_batch_exportPitchOf", 16))


def test_entry_points_are_declared_exported_and_bound():
    import re
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer as sp
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs in ENTRIES:
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and len(fn.argtypes) == nargs, name
        declared = header.split("long long " + name + "(")[1].split(");")[0]
        assert declared.count(",") + 1 == nargs, name
    section = header.split("Pitch ESTIMATED FROM THE SIGNAL")[1].split("speechPlayer_batch_exportPitchOf(")[0]
    for word in ("kPitchMaxWin", "kPitchMaxLag", "N = W + lagMax", "ONE binary32 subtraction", "exact in", "j = i mod 4", "(c_0 + c_1) + (c_2 + c_3)", "never -0.0",
                 "s(tau - 1) + d(tau)", "one product and one division", "!(m(tau + 1) < m(tau))", "ties to the lowest tau", "total order", "(y0 - y1) + (y2 - y1)",
                 "fabs(delta) <= 0.5", "1 F0", "2 PERIOD", "4 LAG", "8 APERIODICITY", "16 VOICED", "32 CMND", "rounded once", "formant", "cross-correlation", "tracking across steps",
                 "octave-error", "FFT or MFMA", "decimation", "live handles", "NodePlayer", "bit above 32"):
        assert word in section, word
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_pitch.h")).read()
    assert "KLATT_PITCH_HD" in shared and "Out of scope" in shared and "Lemma" in shared and '#include "klatt_tiles.h"' in shared and "static_assert(kPitchLdsBudget" in shared
    between = shared.split("namespace klatt {")[1].split("// ---- the device")[0]
    assert "#if" not in between      # nothing between the shared functions changes arithmetic from one side to the other
    for const, value in (("kPitchMaxWin", sp.PITCH_MAX_WIN), ("kPitchMaxLag", sp.PITCH_MAX_LAG), ("kPitchGroup", sp.PITCH_GROUP), ("kPitchMinWin", sp.PITCH_MIN_WIN)):
        assert int(re.search(r"\b%s = (\d+)" % const, shared).group(1)) == value, const
    assert sp.PITCH_FIELDS == ["f0", "period", "lag", "aperiodicity", "voiced", "cmnd"] and callable(sp.BatchPlayer.pitchTensor)
    for name in ("PITCH_FIELDS", "pitchLags", "pitchColumns", "check_pitch_request", "pcmPitch", "signalPitch"):
        assert getattr(nvspeechplayer_amd, name) is getattr(sp, name) and name in nvspeechplayer_amd.__all__, name
    engine = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_engine.hip")).read()
    assert '#include "klatt_pitch.h"' in engine


def test_pitch_lags():
    import nvspeechplayer_amd as eng
    assert eng.pitchLags(22050) == (44, 368) and eng.pitchLags(16000) == (32, 267) and eng.pitchLags(16000, 50.0, 400.0) == (40, 320)
    assert eng.pitchLags(8000, 60.0, 7000.0) == (2, 134) and eng.pitchLags(96000) == (192, 1024) and eng.pitchLags(22050, 1.0, 2.0) == (1023, 1024)
    assert eng.pitchLags(22050.0, 100.0, 441.0) == (50, 221)      # exact divisions stay
    for bad in ((0, 60.0, 500.0), (22050, 0.0, 500.0), (22050, 500.0, 60.0), (22050, 60.0, math.inf), (22050, math.nan, 500.0)):
        with pytest.raises(ValueError, match="pitchLags"):
            eng.pitchLags(*bad)


def test_binding_request_checks():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    ok = dict(sampleRate=22050, fmin=60.0, fmax=500.0, lagMin=None, lagMax=None, nWin=1024, hop=256, phase=0, threshold=0.1, fields=("f0", "aperiodicity"), dtype=None)
    assert sp.check_pitch_request(**ok) == (22050, 1024, 44, 368, 0.1, 256, 0, 9, 2, 1)
    assert sp.check_pitch_request(**{**ok, "lagMin": 2, "lagMax": 1024, "fields": 63, "dtype": torch.float64, "threshold": 1})[2:] == (2, 1024, 1.0, 256, 0, 63, 1028, 0)
    for kw, error, words in ((dict(sampleRate=0), ValueError, "sampleRate"), (dict(sampleRate=22050.0), ValueError, "sampleRate"), (dict(sampleRate=None), ValueError, "sampleRate"),
                             (dict(lagMin=44), ValueError, "come together"), (dict(lagMax=44), ValueError, "come together"), (dict(lagMin=1, lagMax=9), ValueError, "lagMin"),
                             (dict(lagMin=9, lagMax=9), ValueError, "lagMin"), (dict(lagMin=9, lagMax=1025), ValueError, "lagMax"), (dict(lagMin=9.0, lagMax=90), ValueError, "integers"),
                             (dict(fmin=0.0), ValueError, "pitchLags"), (dict(fmax=50.0), ValueError, "pitchLags"),
                             (dict(nWin=31), ValueError, "nWin"), (dict(nWin=2049), ValueError, "nWin"), (dict(nWin=512.0), ValueError, "nWin"), (dict(nWin=True), ValueError, "nWin"),
                             (dict(hop=0), ValueError, "hop"), (dict(hop=2.5), ValueError, "hop must be an integer"), (dict(phase=-1), ValueError, "phase"),
                             (dict(threshold=-0.1), ValueError, "threshold"), (dict(threshold=1.01), ValueError, "threshold"), (dict(threshold=math.nan), ValueError, "threshold"),
                             (dict(threshold="0.1"), ValueError, "threshold"), (dict(fields=()), ValueError, "no fields"), (dict(fields=("f0", "energy")), KeyError, "energy"),
                             (dict(fields=0), ValueError, "fields 0"), (dict(fields=64), ValueError, "fields 64"), (dict(dtype=torch.int16), TypeError, "dtype")):
        with pytest.raises(error, match=words):
            sp.check_pitch_request(**{**ok, **kw})
    row = np.arange(300, dtype=np.int16)
    with pytest.raises(TypeError, match="int16"):
        sp.pcmPitch(row.astype(np.int32), 22050)
    with pytest.raises(TypeError, match="int16 or float32"):
        sp.signalPitch(row.astype(np.float64), 22050)
    assert sp.pcmPitch(row[:0], 22050).shape == (0, 2) and sp.pcmPitch(row, 22050, phase=300).shape == (0, 2) and sp.pcmPitch(row, 22050, fields="cmnd").shape == (2, 325)


def test_every_refusal_of_the_c_entry_points():
    """Every refusal of the two host entry points writes nothing, sets SPEECHPLAYER_ERR_ARGUMENT and names its entry point."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    p = lambda a: None if a is None else a.ctypes.data
    pcm = (np.arange(400) * 37 % 2001 - 1000).astype(np.int16)
    x = np.linspace(-1, 1, 400).astype(F32)
    out = np.full(4000, -7.0)

    def call(x=pcm, of_signal=None, length=400, rate=16000, nWin=64, lagMin=4, lagMax=40, threshold=0.2, hop=50, phase=0, what=63, out=out):
        if of_signal is None:
            return L.speechPlayer_pcmPitch(p(x), length, rate, nWin, lagMin, lagMax, threshold, hop, phase, what, p(out))
        return L.speechPlayer_signalPitch(p(x), of_signal, length, rate, nWin, lagMin, lagMax, threshold, hop, phase, what, p(out))

    def refused(fn, name, table):
        for case, (kw, words) in table.items():
            assert fn(**kw) == -1, (name, case)
            err = L.speechPlayer_lastError()
            assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and name in err and words in err, (name, case, err)
            assert np.all(out == -7.0), (name, case)
    table = dict(length_negative=(dict(length=-1), b"length -1"), length_above=(dict(length=(1 << 44) + 1), b"length"), no_samples=(dict(x=None), b"with its samples"),
                 hop_0=(dict(hop=0), b"hop 0"), phase_negative=(dict(phase=-1), b"phase -1"), rate_0=(dict(rate=0), b"sampleRate 0"), rate_negative=(dict(rate=-8000), b"sampleRate -8000"),
                 nwin_31=(dict(nWin=31), b"nWin 31"), nwin_2049=(dict(nWin=2049), b"nWin 2049"), lagmin_1=(dict(lagMin=1), b"lagMin 1"), lags_equal=(dict(lagMin=40), b"lagMin 40, lagMax 40"),
                 lags_crossed=(dict(lagMin=41), b"lagMin 41"), lagmax_1025=(dict(lagMax=1025), b"lagMax 1025"), threshold_negative=(dict(threshold=-1e-9), b"threshold"),
                 threshold_above=(dict(threshold=1.0000001), b"threshold"), threshold_nan=(dict(threshold=math.nan), b"threshold"), threshold_inf=(dict(threshold=math.inf), b"threshold"),
                 what_0=(dict(what=0), b"what 0"), what_64=(dict(what=64), b"what 64"), what_negative=(dict(what=-1), b"what -1"), no_output=(dict(out=None), b"no output"))
    refused(call, b"pcmPitch", table)
    refused(lambda **kw: call(**{**dict(x=x, of_signal=1), **kw}), b"signalPitch",
            dict(table, in_format_2=(dict(of_signal=2), b"input format 2"), in_format_negative=(dict(of_signal=-1), b"input format -1"),
                 sample_nan=(dict(x=np.where(np.arange(400) == 9, np.nan, x).astype(F32)), b"sample 9 is"),
                 sample_large=(dict(x=np.where(np.arange(400) == 11, -65537.0, x).astype(F32)), b"sample 11 is")))
    assert call() == 8 * 42 and np.all(out[336:] == -7.0) and out[:336].any()
    assert call(x=None, length=0, out=None) == 0 and call(length=3, phase=3, out=None) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert call(threshold=0.0) == 336 and call(threshold=1.0, lagMin=2, lagMax=3, what=1) == 8


# ---- 5. the kernel's walk ------------------------------------------------------------------------------------------------------------------------
def test_the_kernels_walk_under_sanitizers(tmp_path):
    """csrc/klatt_pitch.h and klatt_tiles.h in a program of its own, tests/native/check_pitch.cpp, under AddressSanitizer + UBSan: the
    kernel's walk modelled on the host against brute force -- 16-step groups across row ends, four lags a lane in passes of 256, the scan
    through the lanes, the choice's butterfly, the per-step CMND write through the row writer, padded and packed outputs, misaligned first
    elements, W in {32, 33, 34, 35, 2048}, lagMax in {3, 63, 64, 65, 1024}, lagMin in {2, lagMax - 1}, rows shorter than a frame and of 0
    and 1 samples, phase > 0, hop 1 and N + 1.  The program is run directly: nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_pitch")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_pitch.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and int(out.split()[1]) > 1000000, out
