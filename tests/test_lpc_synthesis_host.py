"""LPC synthesis on the host (include/speechPlayer_batch.h: speechPlayer_pcmLpcSynthesis, signalLpcSynthesis, lpcFromReflection;
nvspeechplayer_amd.pcmLpcSynthesis, signalLpcSynthesis, lpcFromReflection, lpcBandwidthExpand, check_lpc_synthesis_request;
csrc/klatt_lpcsynth.h): a transcription of the definition written here in plain Python with an exact fma, independent of the shared
header, held to the statements bit for bit; the exact cases; the round trip through the residual; every refusal; and a model of the
kernel's walk in a program of its own under the sanitizers (tests/native/check_lpc_synth.cpp).  `t_synthesis` is what
tests/test_gpu_lpc_synthesis.py does not need: the device is held to the statements.  No GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_lpc_host import bits, float_row, fma, fma_int, golden_pcm, segment, t_int16, t_steps, t_x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
F32, F64 = np.float32, np.float64
LENGTHS = (0, 1, 3, 63, 64, 65, 700)


# ---- the transcription: the definition in plain Python ---------------------------------------------------------------------------------------
def t_frame(t, hop, phase, steps):
    return min(steps - 1, (max(t - phase, 0) + hop // 2) // hop)


def t_synthesis(row, coeff, hop, phase, f=fma_int):
    """{type: [L]}: one row through 1 / A(z), float32 and int16 of the same float32 y; the history is the float32 y."""
    e, L = t_x(row), len(row)
    steps, order = t_steps(L, hop, phase), coeff.shape[1]
    out = {F32: np.zeros(L, F32), np.int16: np.zeros(L, np.int16)}
    rows = [[float(v) for v in c] for c in coeff]
    y = []
    for t in range(L):
        a = rows[t_frame(t, hop, phase, steps)] if steps else [0.0] * order
        s = float(e[t])
        for m in range(1, order + 1):
            s = f(-a[m - 1], y[t - m] if t - m >= 0 else 0.0, s)
        with np.errstate(over="ignore"):
            v = F32(s)
        y.append(float(v))
        out[F32][t], out[np.int16][t] = v, (t_int16(v) if math.isfinite(v) else 0)
    return out


def stable(order, steps, rng, scale=0.9):
    """[steps, order] float64: a_1 .. a_order of stable filters that vary slowly from step to step (independent filters switched every
    sample make an unstable time-varying system): one draw of reflection coefficients in (-scale, scale), each step's shrunk by its
    own factors in (0.8, 1), stepped up."""
    import nvspeechplayer_amd as eng
    k0 = rng.uniform(-scale, scale, order)
    return np.array([eng.lpcFromReflection(k0 * rng.uniform(0.8, 1.0, order)) for _ in range(steps)], F64).reshape(steps, order)


def rows_for(L):
    return segment("ipa_l15_s10_c0_p100_i05", L), float_row(segment("ipa_l3_8k", L, lead=25))


def statement_of(row):
    import nvspeechplayer_amd as eng
    return eng.pcmLpcSynthesis if row.dtype == np.int16 else eng.signalLpcSynthesis


# ---- 1. the transcription ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 8, 9, 32])
def test_the_statements_are_the_transcription(order):
    """Golden segments of 0, 1, 3, 63, 64, 65 and 700 samples, int16 and float32 x hop {1, 7, 160, L + 9} x phase {0, 7} x int16 and
    float32 out, stable random coefficients (binary64, not float32 images): pcmLpcSynthesis / signalLpcSynthesis against the
    transcription on integer views; the int16 rows through signalLpcSynthesis (inFormat 0) as well."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(order)
    samples = 0
    for L in LENGTHS:
        for hop in (1, 7, 160, L + 9):
            if L == 700 and hop == 1 and order > 9:
                continue      # (700 frames of order 32 in plain Python: the shorter rows meet hop 1 at this order)
            for phase in (0, 7):
                steps = t_steps(L, hop, phase)
                coeff = stable(order, steps, rng)
                for row in rows_for(L):
                    want = t_synthesis(row, coeff, hop, phase)
                    tag = (order, L, hop, phase, row.dtype)
                    assert np.all(np.isfinite(want[F32])), tag
                    for npt, w in want.items():
                        g = statement_of(row)(row, coeff, hop=hop, phase=phase, dtype=npt)
                        assert g.dtype == npt and g.shape == (L,) and np.array_equal(bits(g), bits(w)), tag + (npt,)
                        if row.dtype == np.int16:
                            assert np.array_equal(bits(eng.signalLpcSynthesis(row, coeff, hop=hop, phase=phase, dtype=npt)), bits(w)), tag + (npt, "signal")
                    samples += L
    assert samples > 3000


def test_the_transcription_by_the_fraction_fma():
    """The fast fma of the cross against the Fraction form on one case of each ring's edge."""
    rng = np.random.default_rng(3)
    for order in (8, 9, 32):
        row = rows_for(65)[1]
        coeff = stable(order, t_steps(65, 7, 0), rng)
        a, b = t_synthesis(row, coeff, 7, 0, fma), t_synthesis(row, coeff, 7, 0, fma_int)
        assert np.array_equal(bits(a[F32]), bits(b[F32])) and np.array_equal(a[np.int16], b[np.int16])


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------------------
def test_exact_cases():
    import nvspeechplayer_amd as eng
    # zero coefficients: y is the float32 of e bit for bit -- but for a -0 of e, which fma(-0.0, y, s) turns into +0 once a negative y
    # lies in the history (the int16 rows have no -0; the float32 row has, on purpose)
    def but_for_minus_zero(y, e):
        return np.array_equal(y, e) and np.array_equal(bits(y)[e != 0], bits(e)[e != 0])
    for row in rows_for(700):
        for order in (1, 16, 32):
            zeros = np.zeros((t_steps(700, 160, 0), order))
            y = statement_of(row)(row, zeros, hop=160)
            assert np.array_equal(bits(y), bits(t_x(row))) if row.dtype == np.int16 else but_for_minus_zero(y, t_x(row)), (row.dtype, order)
    # order 1, a_1 = -0.5, a unit impulse: 1, 0.5, 0.25, ... exactly
    e = np.zeros(40, F32)
    e[0] = 1.0
    y = eng.signalLpcSynthesis(e, np.full((1, 1), -0.5), hop=64)
    assert np.array_equal(y, (2.0 ** -np.arange(40)).astype(F32))
    assert np.array_equal(eng.signalLpcSynthesis(e, np.full((1, 1), -0.5), hop=64, dtype=np.int16)[:3], [32767, 16384, 8192])      # (rint(16383.5) to even)
    # a row without steps (length <= phase): coefficients +0, the row itself
    row = rows_for(5)[1]
    assert but_for_minus_zero(eng.signalLpcSynthesis(row, np.zeros((0, 4)), hop=3, phase=5), row)
    assert eng.pcmLpcSynthesis(np.zeros(0, np.int16), np.zeros((0, 4))).shape == (0,)
    # the history is the float32 y, not the int16 of the output: the int16 output is the conversion of the float32 output
    row = rows_for(700)[0]
    coeff = stable(10, t_steps(700, 160, 0), np.random.default_rng(1))
    y = eng.pcmLpcSynthesis(row, coeff, hop=160)
    assert np.array_equal(eng.pcmLpcSynthesis(row, coeff, hop=160, dtype=np.int16), np.array([t_int16(v) for v in y]))
    e = np.zeros(12, F32)
    e[0] = 1.0
    grow = np.full((1, 1), -1.5)      # (unstable, not refused: 1.5^t is exact in float32 here, and the int16 output clips while the history does not)
    assert np.array_equal(eng.signalLpcSynthesis(e, grow, hop=64), (1.5 ** np.arange(12)).astype(F32))
    assert np.all(eng.signalLpcSynthesis(e, grow, hop=64, dtype=np.int16) == 32767)


@pytest.mark.parametrize("order", range(1, 33))
def test_step_up_is_the_levinson_update(order):
    """lpcFromReflection(k) equals the `a` of lpcFromAutocorrelation bit for bit wherever stages == order."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(100 + order)
    full = 0
    for trial in range(6):
        x = rng.standard_normal(400) * np.hanning(400)
        if trial & 1:
            x = np.convolve(x, [1.0, -0.9, 0.4])[:400]
        r = np.array([np.dot(x[k:], x[:400 - k]) for k in range(order + 1)])
        r[0] *= 1.0 + 2.0 ** -12
        a, k, E, stages = eng.lpcFromAutocorrelation(r)
        if stages == order:
            full += 1
            assert np.array_equal(bits(eng.lpcFromReflection(k)), bits(a)), trial
    assert full >= 3
    assert np.array_equal(eng.lpcFromReflection([-0.5] + [0.0] * (order - 1)), [-0.5] + [0.0] * (order - 1))


def test_bandwidth_expansion_is_its_statement():
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(9)
    for shape, gamma in (((16,), 0.994), ((5, 32), 0.9), ((2, 3, 1), 1.0), ((0, 8), 0.5)):
        a = rng.uniform(-2, 2, shape)
        got = eng.lpcBandwidthExpand(a, gamma)
        g, want = 1.0, np.zeros(shape)
        for j in range(shape[-1]):
            g = g * gamma
            want[..., j] = a[..., j] * g
        assert got.dtype == F64 and got.shape == shape and np.array_equal(bits(got), bits(want)), shape
    with pytest.raises(ValueError, match="lpcBandwidthExpand"):
        eng.lpcBandwidthExpand(np.ones(4), math.nan)


# ---- 3. the round trip ------------------------------------------------------------------------------------------------------------------------------
ROUND_TRIP_MEASURED = 4.59e-6                    # max |x^ - x| of the transcription over the segments below (2^-17.7)
ROUND_TRIP_BOUND = 2.0 * ROUND_TRIP_MEASURED     # a factor 2 for other segments
SEGMENTS = ("ipa_l15_s10_c0_p100_i05", "ipa_l3_8k", "ipa_l5_s10_c0_p100_i05", "ipa_l9_s10_c0_p100_i05")


def test_synthesis_of_the_residual_is_the_signal():
    """x^ = synthesis(residual(x)) with the coefficients of pcmLpc (order 16, nWin 512, hop 160, lagWindow(16, 22050)), float32 throughout,
    on golden segments of 700 and 4000 samples of four utterances.  A property of the definition: the residual rounds e(t) to float32
    once and the synthesis y(t) once, and 1 / A(z) carries the first rounding on with the frame's gain, so the figure differs from
    utterance to utterance.  Asserted first, segment by segment: the statement's output is finite and below 2^16 everywhere.  The bound
    was measured on the transcription t_synthesis, the reference, which the statements equal bit for bit on every segment here:
    max |x^ - x| with |x| < 1 is 1.4e-11 and 7.5e-9 (l15, 700 and 4000 samples), 6.0e-8 and 1.2e-7 (l3_8k), 0 and 3.7e-9 (l5), 1.9e-9 and
    4.59e-6 = 2^-17.7 (l9), the worst.  The test allows twice the worst, the factor being room for other segments
    (profiles/lpc_synthesis.txt)."""
    import nvspeechplayer_amd as eng
    lag = eng.lagWindow(16, 22050)
    worst = 0.0
    for name in SEGMENTS:
        for L in (700, 4000):
            row = segment(name, L)
            coeff = np.ascontiguousarray(eng.pcmLpc(row, order=16, nWin=512, hop=160, lagWindow=lag, fields="lpc"))
            e = eng.pcmLpcResidual(row, coeff, hop=160)
            y = eng.signalLpcSynthesis(e, coeff, hop=160)
            assert np.all(np.isfinite(y)) and np.abs(y).max() < 2.0 ** 16, (name, L)
            yt = t_synthesis(e, coeff, 160, 0)[F32]      # the reference
            assert np.array_equal(bits(yt), bits(y)), (name, L)
            d = float(np.abs(yt.astype(F64) - t_x(row).astype(F64)).max())
            worst = max(worst, d)
            print("round trip %s L %d: max |x^ - x| = %.3g = 2^%.1f" % (name, L, d, math.log2(d) if d else -math.inf))
            assert d <= ROUND_TRIP_BOUND, (name, L, d)
    print("round trip: worst %.3g = 2^%.1f, measured %.3g, bound %.3g" % (worst, math.log2(worst), ROUND_TRIP_MEASURED, ROUND_TRIP_BOUND))
    assert worst > 0


# ---- 4. entry points and refusals ------------------------------------------------------------------------------------------------------------------
ENTRIES = (("speechPlayer_pcmLpcSynthesis", 9), ("speechPlayer_signalLpcSynthesis", 10), ("speechPlayer_lpcFromReflection", 3),
           ("speechPlayer_batch_exportLpcSynthesis", 15), ("speechPlayer_batch_exportLpcSynthesisOf", 16))


def test_entry_points_are_declared_exported_and_bound():
    import re
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer as sp
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs in ENTRIES:
        assert name + "(" in header and name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and len(fn.argtypes) == nargs, name
        declared = header.split("long long " + name + "(")[1].split(");")[0]
        assert declared.count(",") + 1 == nargs, name
    residual = header.split("long long speechPlayer_batch_exportLpcResidualOf(")[1].split(");")[0]
    mine = header.split("long long speechPlayer_batch_exportLpcSynthesisOf(")[1].split(");")[0]
    strip = lambda s: re.sub(r"\s+", " ", s).strip()
    assert strip(mine) == strip(residual.replace(" int what,", "")), "the residual export's arguments without `what`"
    assert header.index("speechPlayer_batch_exportLpcResidualOf(") < header.index("LPC synthesis: a row of excitation samples")
    section = header.split("LPC synthesis: a row of excitation samples")[1].split("speechPlayer_batch_exportLpcSynthesisOf(")[0]
    for words in ("1 / A(z)", "(float)s / 32767.0f", "DEVICE tensor [row][step][coeffCols]", "col0 .. col0 + order - 1", "coeffStride in steps", "lpc_frame_of(t, hop, phase, steps)",
                  "ties upward", "A row without steps uses coefficients +0", "y(t) = +0 for t < 0", "s = (double)e(t)", "s = fma(-a_m, (double)y(t - m), s)", "the negation is exact",
                  "y(t) = (float)s", "the history is the float32 y, never the int16 of the output", "m <= order tests", "fma(-0.0, y, s) can change the sign", "resampler's conversion",
                  "Unstable coefficients cannot be refused", "later bits are", "no value steers an address", "initial conditions in or out", "A(z/g1)/A(z/g2)", "order above 32",
                  "a live stage", "NodePlayer", "time-parallel formulations", "a'[j] = fma(k_i, a[i-j], a[j])", "a[i] = k_i", "csrc/klatt_lpcsynth.h"):
        assert words in section, words
    old = header.split("Linear prediction (LPC) of a batch's PCM")[1].split("speechPlayer_batch_exportLpcResidualOf(")[0]
    assert "1 / A(z)" in old and '"LPC synthesis", below' in old      # the old section points here and keeps its words
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_lpcsynth.h")).read()
    for words in ("KLATT_LPC_HD float lpc_synth_step", "lpc_synth_host", "lpc_synth_plan", "filter_pack", "filter_load_rows", "filter_store_rows", "__launch_bounds__(kFilterLanes)",
                  "Out of scope", '#include "klatt_filter.h"'):
        assert words in shared, words
    assert "#if" not in shared.split("namespace klatt {")[1].split("// ---- the device")[0]
    assert "klatt_lpcsynth.h" in open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_lpc.h")).read().split("#pragma once")[0]
    assert '#include "klatt_lpcsynth.h"' in open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_engine.hip")).read()
    assert sp.LPC_SYNTH_HISTORIES == (8, 16, 32) and callable(sp.BatchPlayer.lpcSynthesisTensor)
    for name in ("pcmLpcSynthesis", "signalLpcSynthesis", "lpcFromReflection", "lpcBandwidthExpand", "check_lpc_synthesis_request", "LPC_SYNTH_HISTORIES"):
        assert getattr(nvspeechplayer_amd, name) is getattr(sp, name) and name in nvspeechplayer_amd.__all__, name


def test_binding_request_checks():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    ok = dict(order=16, hop=256, phase=0, column=0, dtype=None)
    assert sp.check_lpc_synthesis_request(**ok) == (16, 256, 0, 0, 1)
    assert sp.check_lpc_synthesis_request(**{**ok, "dtype": torch.int16, "column": 17, "order": 32, "phase": 7}) == (32, 256, 7, 17, 0)
    for kw, error, words in ((dict(order=0), ValueError, "order"), (dict(order=33), ValueError, "order"), (dict(order=8.0), ValueError, "order"), (dict(order=True), ValueError, "order"),
                             (dict(hop=0), ValueError, "hop"), (dict(hop=2.5), ValueError, "hop must be an integer"), (dict(phase=-2), ValueError, "phase"),
                             (dict(phase=True), ValueError, "phase must be an integer"), (dict(column=-1), ValueError, "column"), (dict(column=1.5), ValueError, "column"),
                             (dict(dtype=np.float64), TypeError, "dtype")):
        with pytest.raises(error, match=words):
            sp.check_lpc_synthesis_request(**{**ok, **kw})
    row = np.arange(300, dtype=np.int16)
    with pytest.raises(ValueError, match="2 rows of coefficients for 3 steps"):
        sp.pcmLpcSynthesis(row, np.zeros((2, 4)), hop=100)
    with pytest.raises(ValueError, match=r"\[steps, order\]"):
        sp.pcmLpcSynthesis(row, np.zeros(4), hop=100)
    with pytest.raises(ValueError, match="order"):
        sp.pcmLpcSynthesis(row, np.zeros((3, 33)), hop=100)
    with pytest.raises(TypeError, match="int16"):
        sp.pcmLpcSynthesis(row.astype(np.int32), np.zeros((3, 4)), hop=100)
    with pytest.raises(TypeError, match="int16 or float32"):
        sp.signalLpcSynthesis(row.astype(np.float64), np.zeros((3, 4)), hop=100)
    for bad in (np.zeros(0), np.zeros(33)):
        with pytest.raises(ValueError, match="lpcFromReflection"):
            sp.lpcFromReflection(bad)


def test_every_refusal_of_the_c_entry_points():
    """Every refusal of the three host entry points writes nothing, sets SPEECHPLAYER_ERR_ARGUMENT and names its entry point."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    p = lambda a: None if a is None else a.ctypes.data
    pcm = (np.arange(400) * 37 % 2001 - 1000).astype(np.int16)
    x = np.linspace(-1, 1, 400).astype(F32)
    res = np.full(500, -7, np.int16)
    coeff = np.full((8, 4), 0.125)

    def synth(x=pcm, of_signal=None, length=400, order=4, hop=50, phase=0, coeff=coeff, fmt=0, res=res, capacity=500):
        if of_signal is None:
            return L.speechPlayer_pcmLpcSynthesis(p(x), length, order, hop, phase, p(coeff), fmt, p(res), capacity)
        return L.speechPlayer_signalLpcSynthesis(p(x), of_signal, length, order, hop, phase, p(coeff), fmt, p(res), capacity)

    def refused(call, name, table):
        for case, (kw, words) in table.items():
            assert call(**kw) == -1, (name, case)
            err = L.speechPlayer_lastError()
            assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and name in err and words in err, (name, case, err)
            assert np.all(res == -7), (name, case)
    table = dict(length_negative=(dict(length=-1), b"length -1"), length_above=(dict(length=(1 << 44) + 1), b"length"), no_samples=(dict(x=None), b"with its samples"),
                 hop_0=(dict(hop=0), b"hop 0"), phase_negative=(dict(phase=-1), b"phase -1"), order_0=(dict(order=0), b"order 0"), order_33=(dict(order=33), b"order 33"),
                 format_2=(dict(fmt=2), b"format 2"), format_negative=(dict(fmt=-1), b"format -1"), no_coefficients=(dict(coeff=None), b"no coefficients"),
                 no_output=(dict(res=None), b"no output"), capacity_short=(dict(capacity=399), b"capacity is 399"))
    refused(synth, b"pcmLpcSynthesis", table)
    refused(lambda **kw: synth(**{**dict(x=x, of_signal=1), **kw}), b"signalLpcSynthesis",
            dict(table, in_format_2=(dict(of_signal=2), b"input format 2"), in_format_negative=(dict(of_signal=-1), b"input format -1"),
                 sample_inf=(dict(x=np.where(np.arange(400) == 5, np.inf, x).astype(F32)), b"sample 5 is"),
                 sample_large=(dict(x=np.where(np.arange(400) == 11, -65537.0, x).astype(F32)), b"sample 11 is")))
    assert synth() == 400 and np.all(res[400:] == -7) and res[:400].any()
    assert synth(x=None, length=0, coeff=None, res=None, capacity=0) == 0 and synth(length=3, phase=3, coeff=None) == 3 and L.speechPlayer_lastErrorCode() == 0
    assert synth(hop=1 << 50, phase=1 << 50, coeff=None) == 400      # (beyond any row: no steps)

    a = np.full(4, -7.0)
    k = np.array([0.5, -0.25, 0.125, 0.0])
    for order, kk, aa, words in ((0, k, a, b"order 0"), (33, k, a, b"order 33"), (4, None, a, b"no reflection coefficients"), (4, k, None, b"no output")):
        assert L.speechPlayer_lpcFromReflection(p(kk), order, p(aa)) == -1
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"lpcFromReflection" in L.speechPlayer_lastError() and words in L.speechPlayer_lastError()
        assert np.all(a == -7)
    assert L.speechPlayer_lpcFromReflection(p(k), 4, p(a)) == 4 and a[3] == 0.0 and a[2] == 0.125


# ---- 5. the kernel's walk --------------------------------------------------------------------------------------------------------------------------
def test_the_kernels_walk_under_sanitizers(tmp_path):
    """csrc/klatt_lpcsynth.h in a program of its own, tests/native/check_lpc_synth.cpp, under AddressSanitizer + UBSan: the kernel's walk
    modelled on the host from the shared body against lpc_synth_host -- groups of 64 with fillers, 64-sample tiles, the ring of B slots,
    frame changes inside tiles and on their edges, clamped last frames, in-place staging -- with 1 .. 130 rows of 0 .. 200 samples.  The
    program is run directly: nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_lpc_synth")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_lpc_synth.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and int(out.split()[1]) > 1000000, out
