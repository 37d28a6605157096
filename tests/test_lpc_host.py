"""The linear-prediction exports on the host (include/speechPlayer_batch.h: speechPlayer_lpcFromAutocorrelation, speechPlayer_pcmLpc,
signalLpc, pcmLpcResidual, signalLpcResidual; nvspeechplayer_amd.pcmLpc, signalLpc, lpcFromAutocorrelation, pcmLpcResidual,
signalLpcResidual, lagWindow, LPC_FIELDS; csrc/klatt_lpc.h): the recursion's exact cases, a transcription of the definition written here
in numpy and plain Python, independent of the shared header, held to the statements bit for bit; the coefficients against scipy's
Toeplitz solver within the bound the conditioning gives; every refusal; and a model of both kernels' walks in a program of its own under
the sanitizers (tests/native/check_lpc.cpp).  `golden_pcm`, `segment`, `float_row` and `bits` are what tests/test_gpu_lpc.py shares.
No GPU."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
F32, F64 = np.float32, np.float64
ORDERS = (1, 2, 16, 32)
_pcm = {}


def golden_pcm(name):
    """An utterance of tests/golden/expected_pcm.npz, read once: int16."""
    if name not in _pcm:
        with np.load(os.path.join(ROOT, "tests", "golden", "expected_pcm.npz")) as z:
            _pcm[name] = z[name].copy()
    return _pcm[name]


def segment(name, L, lead=40):
    """L samples of a golden utterance that begin `lead` samples (at most L / 2) before its first silence of 50 samples or more ends: a
    silence, an onset and voiced or fricative sound where L allows."""
    pcm = golden_pcm(name)
    zero = np.concatenate([[0], (pcm == 0).astype(np.int64), [0]])
    starts, ends = np.flatnonzero(np.diff(zero) == 1), np.flatnonzero(np.diff(zero) == -1)
    long = np.flatnonzero(ends - starts >= 50)
    assert len(long), name
    a0 = int(ends[long[0]]) - min(lead, L // 2)
    assert a0 >= 0 and a0 + L <= len(pcm), (name, L)
    return pcm[a0:a0 + L].copy()


def float_row(pcm):
    """A float32 row that is not a scaled int16 row's image: the definition's x times 1.7, every 11th zero of it a -0."""
    x = (pcm.astype(F32) / F32(32767.0)) * F32(1.7)
    z = np.flatnonzero(x == 0)[::11]
    x[z] = F32(-0.0)
    return x


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


# ---- the transcription: sections 1 and 3 of the definition, in numpy and plain Python ------------------------------------------------------
def fma(a, b, c):
    """a * b + c rounded once (Python 3.10 has no math.fma): the exact sum as a Fraction, which float() rounds correctly; a zero takes
    IEEE's sign -- an exact zero product plus a zero is -0 only when both are negative, a sum that cancels is +0."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c      # (an infinity or a NaN: no rounding to fuse)
    s = Fraction(a) * Fraction(b) + Fraction(c)
    if s == 0:
        if a == 0.0 or b == 0.0:
            neg = (math.copysign(1.0, a) * math.copysign(1.0, b)) < 0
            return -0.0 if neg and c == 0.0 and math.copysign(1.0, c) < 0 else (c if c != 0.0 else 0.0)
        return 0.0
    return float(s)


def fma_int(a, b, c):
    """The same by integer ratios (a float is n / 2^k; int / int is correctly rounded): six times faster, for the cross below;
    test_the_two_fmas_agree holds it to fma."""
    if a == 0.0 or b == 0.0 or c == 0.0 or not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return fma(a, b, c)
    an, ad = a.as_integer_ratio()
    bn, bd = b.as_integer_ratio()
    cn, cd = c.as_integer_ratio()
    d = ad * bd
    n, d = (an * bn + cn * (d // cd), d) if d >= cd else (an * bn * (cd // d) + cn, cd)
    return n / d if n else 0.0


def t_steps(L, hop, phase):
    return -(-(L - phase) // hop) if L > phase else 0


def t_x(row):
    """The reader: an int16 s is (float)s / 32767.0f, a float32 is taken as it is."""
    return row.astype(F32) / F32(32767.0) if row.dtype == np.int16 else row.astype(F32)


def t_window(nWin, window):
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nWin, dtype=F64) / nWin) if window is None else np.asarray(window, F64)
    return w.astype(F32)


def t_autocorr(xw, order):
    """r[0 .. order] of one frame: the 64 partials in ascending i from +0.0 and the tree, written out (all lags side by side)."""
    nWin, M = len(xw), -(-len(xw) // 64)
    x = xw.astype(F64)
    back = np.lib.stride_tricks.sliding_window_view(np.concatenate([np.zeros(order), x]), order + 1)[:, ::-1]      # back[i, k] = x[i - k]
    term, there = np.zeros((M * 64, order + 1)), np.zeros((M * 64, order + 1), bool)
    term[:nWin] = x[:, None] * back                                        # (exact: 24 x 24 bits)
    there[:nWin] = np.arange(nWin)[:, None] >= np.arange(order + 1)[None, :]      # the terms of k <= i < nWin
    term, there = term.reshape(M, 64, order + 1), there.reshape(M, 64, order + 1)
    partial = np.zeros((64, order + 1))
    for m in range(M):      # i = 64 m + q ascending; a term that is not there is not added
        partial = np.where(there[m], partial + term[m], partial)
    t = partial
    for _ in range(6):      # t[i] = t[2i] + t[2i+1]
        t = t[0::2] + t[1::2]
    return t[0].copy()


def t_levinson(r, order, f=fma_int):
    a, k = [0.0] * (order + 1), [0.0] * (order + 1)
    E, stages = float(r[0]), 0
    for i in range(1, order + 1):
        if not (E > 0 and math.isfinite(E)):
            break
        acc = float(r[i])
        for j in range(1, i):
            acc = f(a[j], float(r[i - j]), acc)
        kappa = -acc / E
        if not abs(kappa) < 1:
            break
        new = [f(kappa, a[i - j], a[j]) for j in range(1, i)]
        a[1:i] = new
        a[i] = k[i] = kappa
        E = f(kappa, acc, E)
        stages = i
    return a[1:], k[1:], E, stages


def t_columns(what, order):
    return (order + 1 if what & 1 else 0) + (order if what & 2 else 0) + (order if what & 4 else 0) + (1 if what & 8 else 0) + (1 if what & 16 else 0)


def t_lpc(row, order, nWin, hop, phase, window, lag, what):
    """[steps, nCols] float64: the analysis of one row."""
    x, L = t_x(row), len(row)
    w = t_window(nWin, window)
    out = []
    for j in range(t_steps(L, hop, phase)):
        at = phase + j * hop - nWin // 2 + np.arange(nWin)
        inside = (at >= 0) & (at < L)
        frame = np.where(inside, x[np.clip(at, 0, max(L - 1, 0))] if L else F32(0), F32(0)).astype(F32)
        r = t_autocorr(frame * w, order)
        if lag is not None:
            r = r * np.asarray(lag, F64)
        a, k, E, stages = t_levinson(r, order)
        cols = []
        if what & 1:
            cols += list(r)
        if what & 2:
            cols += a
        if what & 4:
            cols += k
        if what & 8:
            cols.append(E)
        if what & 16:
            cols.append(float(stages))
        out.append(cols)
    return np.array(out, F64).reshape(len(out), t_columns(what, order))


def t_int16(y):
    q = F32(y) * F32(32767.0)
    return np.int16(32767 if q >= 32767 else -32768 if q <= -32768 else np.rint(q))


def t_residual(row, coeff, hop, phase, f=fma_int):
    """{(what, type): [L]}: the residual (0) and the prediction (1) of one row, float32 and int16."""
    x, L = t_x(row), len(row)
    steps, order = t_steps(L, hop, phase), coeff.shape[1]
    out = {(what, npt): np.zeros(L, npt) for what in (0, 1) for npt in (F32, np.int16)}
    xd = [float(v) for v in x]
    rows = [[float(v) for v in c] for c in coeff]
    for t in range(L):
        a = rows[min(steps - 1, (max(t - phase, 0) + hop // 2) // hop)] if steps else [0.0] * order
        e, p = xd[t], 0.0
        for m in range(1, order + 1):
            past = xd[t - m] if t - m >= 0 else 0.0
            e, p = f(a[m - 1], past, e), f(a[m - 1], past, p)
        for what, y in ((0, F32(e)), (1, F32(-p))):
            out[what, F32][t], out[what, np.int16][t] = y, t_int16(y)
    return out


# ---- 1. exact cases ------------------------------------------------------------------------------------------------------------------------
def test_exact_cases_of_the_recursion():
    import nvspeechplayer_amd as eng
    a, k, E, stages = eng.lpcFromAutocorrelation(2.0 ** -np.arange(9))
    assert a[0] == -0.5 and k[0] == -0.5 and np.all(a[1:] == 0) and np.all(k[1:] == 0) and E == 0.75 and stages == 8
    a, k, E, stages = eng.lpcFromAutocorrelation([1.0] + [0.0] * 8)
    assert np.all(a == 0) and np.all(k == 0) and E == 1.0 and stages == 8
    a, k, E, stages = eng.lpcFromAutocorrelation([0.0] + [0.5] * 8)
    assert stages == 0 and not bits(a).any() and not bits(k).any() and E == 0.0
    for r in ([1.0] * 9, [1.0, 2.0]):
        a, k, E, stages = eng.lpcFromAutocorrelation(r)
        assert stages == 0 and not bits(a).any() and not bits(k).any() and E == 1.0, r
    for first in (np.inf, np.nan):
        a, k, E, stages = eng.lpcFromAutocorrelation([first, 0.5, 0.25])
        assert stages == 0 and not bits(a).any() and not bits(k).any(), first
    # the transcription says the same
    assert t_levinson(2.0 ** -np.arange(9), 8, fma) == ([-0.5] + [0.0] * 7, [-0.5] + [0.0] * 7, 0.75, 8)
    assert t_levinson([1.0, 1.0, 1.0], 2, fma)[3] == 0 and t_levinson([1.0, 2.0], 1, fma)[3] == 0 and t_levinson([np.nan, 0.0], 1, fma)[3] == 0


def test_the_two_fmas_agree():
    """fma_int, which the cross uses for its speed, against the Fraction form of the definition: random triples over 80 binades, exact
    cancellations, halfway cases and zeros of both signs, compared as bit patterns."""
    rng = np.random.default_rng(5)
    a = rng.uniform(-1, 1, 20000) * 2.0 ** rng.integers(-40, 40, 20000)
    b = rng.uniform(-1, 1, 20000) * 2.0 ** rng.integers(-40, 40, 20000)
    c = rng.uniform(-1, 1, 20000) * 2.0 ** rng.integers(-40, 40, 20000)
    c[::7] = -(a[::7] * b[::7])                     # near cancellation: the low half of the product survives
    a[::13] = np.round(a[::13] * 2 ** 20) / 2 ** 20      # short operands: exact products, halfway sums
    triples = list(zip(a.tolist(), b.tolist(), c.tolist()))
    triples += [(x, y, z) for x in (0.0, -0.0, 1.5, -1.5) for y in (0.0, -0.0, 2.0) for z in (0.0, -0.0, 3.0, -3.0)]
    triples += [(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0), (3.0, 2.0 ** -53, 1.0), (1.0, 2.0 ** -53, 1.0), (0.5, -2.0, 1.0)]
    for t in triples:
        assert np.float64(fma(*t)).view(np.uint64) == np.float64(fma_int(*t)).view(np.uint64), t
    assert math.copysign(1.0, fma(-0.0, 2.0, -0.0)) < 0 and math.copysign(1.0, fma(-0.0, 2.0, 0.0)) > 0 and math.copysign(1.0, fma(0.5, -2.0, 1.0)) > 0
    assert fma(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0) == 2.0 ** -51 + 2.0 ** -104      # one rounding, not two


# ---- 2. the independent transcription --------------------------------------------------------------------------------------------------------
def rows_for(L):
    """An int16 and a float32 row of L samples: two utterances, a silence inside where L allows."""
    return segment("ipa_l15_s10_c0_p100_i05", L), float_row(segment("ipa_l3_8k", L, lead=25))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("win", ["order+1", 63, 64, 65, 400, 512])
def test_the_statements_are_the_transcription(win, order):
    """nWin x order x hop {1, 80, 2 nWin} x phase {0, 7} x lengths {0, 1, order, nWin // 2 - 1, nWin, 3 hop + 5} x int16 and float32
    rows x with and without a lag window: pcmLpc / signalLpc with every field and pcmLpcResidual / signalLpcResidual (both outputs) with
    the coefficients the analysis gave, against the transcription, on integer views.  The int16 rows go through the pcm* statements
    and, without the lag window, through the signal* statements with inFormat 0 as well."""
    import nvspeechplayer_amd as eng
    nWin = order + 1 if win == "order+1" else win
    lag = eng.lagWindow(order, 16000.0, bandwidth=60.0, whiteNoise=2.0 ** -10)
    window = np.hamming(nWin) - 0.2      # (not the default; some values negative)
    frames = 0
    for hop in (1, 80, 2 * nWin):
        for phase in (0, 7):
            for L in sorted({0, 1, order, nWin // 2 - 1, nWin, 3 * hop + 5}):
                for row in rows_for(L):
                    statement, residual = (eng.pcmLpc, eng.pcmLpcResidual) if row.dtype == np.int16 else (eng.signalLpc, eng.signalLpcResidual)
                    for lw in (None, lag):
                        win_ = window if lw is None else None      # (the default window with the lag window, another without)
                        tag = (nWin, order, hop, phase, L, row.dtype, lw is not None)
                        got = statement(row, order=order, nWin=nWin, hop=hop, phase=phase, window=win_, lagWindow=lw, fields=31)
                        want = t_lpc(row, order, nWin, hop, phase, win_, lw, 31)
                        assert got.shape == want.shape == (t_steps(L, hop, phase), 3 * order + 3), tag
                        assert np.array_equal(bits(got), bits(want)), tag
                        frames += len(got)
                        coeff = np.ascontiguousarray(got[:, order + 1:2 * order + 1])
                        inverse = t_residual(row, coeff, hop, phase)
                        for (what, npt), w in inverse.items():
                            g = residual(row, coeff, hop=hop, phase=phase, what=("residual", "prediction")[what], dtype=npt)
                            assert g.dtype == npt and np.array_equal(bits(g), bits(w)), tag + (what, npt)
                        if row.dtype == np.int16 and lw is None:      # an int16 row through the signal* statements (inFormat 0): the pcm* statements' bits
                            assert np.array_equal(bits(eng.signalLpc(row, order=order, nWin=nWin, hop=hop, phase=phase, window=win_, fields=31)), bits(got)), tag
                            for (what, npt), w in inverse.items():
                                assert np.array_equal(bits(eng.signalLpcResidual(row, coeff, hop=hop, phase=phase, what=what, dtype=npt)), bits(w)), tag + (what, npt, "signal")
    assert frames > 50


def test_fields_come_in_the_fixed_order():
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer as sp
    row = segment("ipa_l15_s10_c0_p100_i05", 700)
    every = eng.pcmLpc(row, order=6, nWin=200, hop=90, fields=31)
    at, total = sp.lpcColumns(sp.LPC_FIELDS, 6)
    assert total == 21 and at == {"autocorr": (0, 7), "lpc": (7, 6), "reflection": (13, 6), "error": (19, 1), "stages": (20, 1)}
    for names in (("error", "lpc"), ("stages",), ("reflection", "autocorr"), "lpc", ("lpc", "error")):
        got = eng.pcmLpc(row, order=6, nWin=200, hop=90, fields=names)
        cols = np.concatenate([np.arange(*(at[n][0], sum(at[n]))) for n in sp.LPC_FIELDS if n in ([names] if isinstance(names, str) else names)])
        assert np.array_equal(bits(got), bits(every[:, cols])), names
    assert (every[:, 20] == 0).any() and (every[:, 20] == 6).any()      # silent frames and full recursions


# ---- 3. it is the LPC --------------------------------------------------------------------------------------------------------------------------
def pulse_train(L, sr=16000):
    """A pulse train at 120 Hz through four formant resonators, float32, at most 1 in magnitude."""
    from scipy.signal import lfilter
    x = np.zeros(L)
    x[::sr // 120] = 1.0
    for f, bw in ((700, 80), (1200, 90), (2600, 120), (3500, 150)):
        r = math.exp(-math.pi * bw / sr)
        x = lfilter([1.0], [1.0, -2.0 * r * math.cos(2 * math.pi * f / sr), r * r], x)
    return (x / np.abs(x).max()).astype(F32)


@pytest.mark.parametrize("order", [1, 2, 8, 16, 32])
def test_the_coefficients_solve_the_normal_equations(order):
    """Against scipy.linalg.solve_toeplitz on the AUTOCORR field the statement returned, with lagWindow[0] = 1 + 2^-10: every frame with
    r[0] > 0 has a condition number of at most (order + 1)(1 + eps) / eps < 2^16 (Gershgorin: the eigenvalues of the uncorrected matrix lie
    in [0, (order + 1) r0]) -- asserted, no such frame left out --, so max |a - a_ref| <= 2^-26 max |a_ref|: cond 2^16 times order^2
    2^10 times u 2^-53, doubled for the two solvers.  On the same frames stages == order, |k_i| < 1 and E is positive and does not
    increase along the prefixes.  Silent frames are counted and have stages == 0."""
    from scipy.linalg import solve_toeplitz, toeplitz
    import nvspeechplayer_amd as eng
    eps = 2.0 ** -10
    lag = np.ones(order + 1)
    lag[0] = 1.0 + eps
    silent = voiced = 0
    worst = 0.0
    for row in (pulse_train(6000), golden_pcm("ipa_l15_s10_c0_p100_i05"), float_row(golden_pcm("ipa_l3_8k"))):
        statement = eng.pcmLpc if row.dtype == np.int16 else eng.signalLpc
        got = statement(row, order=order, nWin=400, hop=160, lagWindow=lag, fields=31)
        r, a, k, E, stages = got[:, :order + 1], got[:, order + 1:2 * order + 1], got[:, 2 * order + 1:3 * order + 1], got[:, -2], got[:, -1]
        for j in range(len(got)):
            if not r[j, 0] > 0:
                assert r[j, 0] == 0 and stages[j] == 0 and not bits(got[j]).any(), j
                silent += 1
                continue
            voiced += 1
            R = toeplitz(r[j, :order])
            assert np.linalg.cond(R) <= (order + 1) * (1 + eps) / eps < 2.0 ** 16, (j, np.linalg.cond(R))
            ref = solve_toeplitz(r[j, :order], -r[j, 1:])
            err = np.abs(a[j] - ref).max() / np.abs(ref).max() if np.abs(ref).max() > 0 else np.abs(a[j]).max()
            worst = max(worst, err)
            assert err <= 2.0 ** -26, (j, err)
            assert stages[j] == order and np.all(np.abs(k[j]) < 1) and E[j] > 0, j
            prefix = [r[j, 0]] + [eng.lpcFromAutocorrelation(r[j, :p + 1])[2] for p in range(1, order + 1)]
            assert all(e > 0 for e in prefix) and all(prefix[p + 1] <= prefix[p] for p in range(order)) and prefix[-1] == E[j], j
    assert silent > 5 and voiced > 80
    print("order %d: %d frames, %d silent, worst relative difference 2^%.1f" % (order, voiced, silent, math.log2(worst) if worst else -math.inf))


# ---- 4. refusals and surface -------------------------------------------------------------------------------------------------------------------
ENTRIES = (("speechPlayer_lpcFromAutocorrelation", 6), ("speechPlayer_pcmLpc", 10), ("speechPlayer_signalLpc", 11), ("speechPlayer_pcmLpcResidual", 10),
           ("speechPlayer_signalLpcResidual", 11), ("speechPlayer_batch_exportLpc", 14), ("speechPlayer_batch_exportLpcOf", 15),
           ("speechPlayer_batch_exportLpcResidual", 16), ("speechPlayer_batch_exportLpcResidualOf", 17))


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
    section = header.split("Linear prediction (LPC) of a batch's PCM")[1].split("speechPlayer_batch_exportLpcResidualOf(")[0]
    for word in ("kLpcMaxOrder", "kLpcMaxWin", "periodic Hann", "exact in binary64", "i mod 64 == q", "t[i] = t[2i] + t[2i+1]", "never -0.0", "lagWindow[0] = 1 + eps",
                 "Levinson-Durbin", "kappa = -acc / E", "fma(kappa, a[i-j], a[j])", "A(z) = 1 + sum a_j z^-j", "1 AUTOCORR", "2 LPC", "4 REFLECTION", "8 ERROR", "16 STAGES",
                 "ties upward", "e(t) = (float)s", "p(t) = (float)(-s)", "line spectral frequencies", "Burg", "1 / A(z)", "order above 32", "pre-emphasis", "live handles",
                 "NodePlayer", "kLpcTile = 1024", "overlaps the", "coeffStride below the largest step count"):
        assert word in section, word
    assert "tests/test_gpu_lpc.py" in header.split("Limits      A row has at most")[1].split("Out of scope")[0]
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_lpc.h")).read()
    assert "KLATT_LPC_HD" in shared and "Out of scope" in shared and "Lemma" in shared and '#include "klatt_tiles.h"' in shared
    between = shared.split("namespace klatt {")[1].split("// ---- the device")[0]
    assert "#if" not in between      # nothing between the shared functions changes arithmetic from one side to the other
    for const, value in (("kLpcMaxOrder", sp.LPC_MAX_ORDER), ("kLpcMaxWin", sp.LPC_MAX_WIN), ("kLpcTile", sp.LPC_TILE)):
        assert int(re.search(r"\b%s = (\d+)" % const, shared).group(1)) == value, const
    assert sp.LPC_FIELDS == ["autocorr", "lpc", "reflection", "error", "stages"] and callable(sp.BatchPlayer.lpcTensor) and callable(sp.BatchPlayer.lpcResidualTensor)
    for name in ("pcmLpc", "signalLpc", "lpcFromAutocorrelation", "pcmLpcResidual", "signalLpcResidual", "lagWindow", "LPC_FIELDS", "check_lpc_request",
                 "check_lpc_residual_request"):
        assert getattr(nvspeechplayer_amd, name) is getattr(sp, name) and name in nvspeechplayer_amd.__all__, name
    engine = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_engine.hip")).read()
    assert '#include "klatt_lpc.h"' in engine


def test_the_lag_window_designer():
    import nvspeechplayer_amd as eng
    for order, sr, bw, wn in ((16, 16000.0, 60.0, 2.0 ** -30), (32, 22050, 100.0, 0.0), (1, 8000, 0.0, 1e-4)):
        w = eng.lagWindow(order, sr, bandwidth=bw, whiteNoise=wn)
        want = np.array([math.exp(-0.5 * (2.0 * math.pi * bw * k / sr) ** 2) for k in range(order + 1)])
        want[0] *= 1.0 + wn
        assert w.dtype == F64 and w.shape == (order + 1,) and np.allclose(w, want, rtol=4e-16, atol=0) and w[0] == 1.0 + wn
    assert np.array_equal(eng.lagWindow(16, 16000.0), eng.lagWindow(16, 16000.0, 60.0, 2.0 ** -30))
    for bad in (dict(order=0), dict(order=33), dict(sampleRate=0.0), dict(bandwidth=-1.0), dict(whiteNoise=-1e-9), dict(sampleRate=math.nan)):
        with pytest.raises(ValueError, match="lagWindow"):
            eng.lagWindow(**{**dict(order=8, sampleRate=16000.0), **bad})


def test_binding_request_checks():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    ok = dict(order=16, nWin=512, hop=256, phase=0, window=None, lagWindow=None, fields=("lpc", "error"), dtype=None)
    assert sp.check_lpc_request(**ok)[6:] == (10, 17, 1) and sp.check_lpc_request(**{**ok, "dtype": torch.float64, "fields": 31})[6:] == (31, 51, 0)
    for kw, error, words in ((dict(order=0), ValueError, "order"), (dict(order=33), ValueError, "order"), (dict(order=2.0), ValueError, "order"), (dict(order=True), ValueError, "order"),
                             (dict(nWin=16), ValueError, "nWin"), (dict(nWin=4097), ValueError, "nWin"), (dict(nWin=400.0), ValueError, "nWin"), (dict(hop=0), ValueError, "hop"), (dict(hop=2.5), ValueError, "hop must be an integer"),
                             (dict(phase=-1), ValueError, "phase"), (dict(phase=1.0), ValueError, "phase must be an integer"), (dict(window=np.ones(511)), ValueError, "window needs 512"),
                             (dict(window=np.where(np.arange(512) == 3, np.inf, 1.0)), ValueError, "window value must be finite"),
                             (dict(lagWindow=np.ones(16)), ValueError, "lagWindow needs 17"), (dict(lagWindow=np.where(np.arange(17) == 3, np.nan, 1.0)), ValueError, "lagWindow value"),
                             (dict(fields=()), ValueError, "no fields"), (dict(fields=("lpc", "lsf")), KeyError, "lsf"), (dict(fields=0), ValueError, "fields 0"),
                             (dict(fields=32), ValueError, "fields 32"), (dict(dtype=torch.int16), TypeError, "dtype")):
        with pytest.raises(error, match=words):
            sp.check_lpc_request(**{**ok, **kw})
    ok = dict(order=16, hop=256, phase=0, column=0, what_="residual", dtype=None)
    assert sp.check_lpc_residual_request(**ok) == (16, 256, 0, 0, 0, 1) and sp.check_lpc_residual_request(**{**ok, "what_": 1, "dtype": np.int16, "column": 17}) == (16, 256, 0, 17, 1, 0)
    for kw, error, words in ((dict(order=0), ValueError, "order"), (dict(order=33), ValueError, "order"), (dict(hop=0), ValueError, "hop"), (dict(hop=2.5), ValueError, "hop must be an integer"), (dict(phase=-2), ValueError, "phase"),
                             (dict(phase=True), ValueError, "phase must be an integer"), (dict(column=-1), ValueError, "column"), (dict(column=1.5), ValueError, "column"), (dict(what_="excitation"), KeyError, "excitation"),
                             (dict(what_=2), KeyError, "what 2"), (dict(dtype=np.float64), TypeError, "dtype")):
        with pytest.raises(error, match=words):
            sp.check_lpc_residual_request(**{**ok, **kw})
    row = np.arange(300, dtype=np.int16)
    with pytest.raises(ValueError, match="2 rows of coefficients for 3 steps"):
        sp.pcmLpcResidual(row, np.zeros((2, 4)), hop=100)
    with pytest.raises(ValueError, match=r"\[steps, order\]"):
        sp.pcmLpcResidual(row, np.zeros(4), hop=100)
    with pytest.raises(TypeError, match="int16"):
        sp.pcmLpc(row.astype(np.int32))
    with pytest.raises(TypeError, match="int16 or float32"):
        sp.signalLpc(row.astype(np.float64))


def test_every_refusal_of_the_c_entry_points():
    """Every refusal of the five host entry points writes nothing, sets SPEECHPLAYER_ERR_ARGUMENT and names its entry point."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    p = lambda a: None if a is None else a.ctypes.data
    pcm = (np.arange(400) * 37 % 2001 - 1000).astype(np.int16)
    x = np.linspace(-1, 1, 400).astype(F32)
    out = np.full(4000, -7.0)
    window, lag = np.ones(64), np.ones(5)

    def refused(call, name, table):
        for case, (kw, words) in table.items():
            assert call(**kw) == -1, (name, case)
            err = L.speechPlayer_lastError()
            assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and name in err and words in err, (name, case, err)
            assert np.all(out == -7.0), (name, case)

    def analysis(x=pcm, of_signal=None, length=400, order=4, nWin=64, hop=50, phase=0, window=window, lag=lag, what=31, out=out):
        if of_signal is None:
            return L.speechPlayer_pcmLpc(p(x), length, order, nWin, hop, phase, p(window), p(lag), what, p(out))
        return L.speechPlayer_signalLpc(p(x), of_signal, length, order, nWin, hop, phase, p(window), p(lag), what, p(out))
    common = dict(length_negative=(dict(length=-1), b"length -1"), length_above=(dict(length=(1 << 44) + 1), b"length"), no_samples=(dict(x=None), b"with its samples"),
                  hop_0=(dict(hop=0), b"hop 0"), phase_negative=(dict(phase=-1), b"phase -1"), order_0=(dict(order=0), b"order 0"), order_33=(dict(order=33), b"order 33"))
    table = dict(common, nwin_order=(dict(nWin=4), b"nWin 4"), nwin_4097=(dict(nWin=4097), b"nWin 4097"),
                 window_inf=(dict(window=np.where(np.arange(64) == 9, np.inf, 1.0)), b"window[9] is not finite"),
                 lag_nan=(dict(lag=np.where(np.arange(5) == 2, np.nan, 1.0)), b"lagWindow[2] is not finite"), what_0=(dict(what=0), b"what 0"), what_32=(dict(what=32), b"what 32"),
                 what_negative=(dict(what=-1), b"what -1"), no_output=(dict(out=None), b"no output"))
    refused(analysis, b"pcmLpc", table)
    refused(lambda **kw: analysis(**{**dict(x=x, of_signal=1), **kw}), b"signalLpc",
            dict(table, in_format_2=(dict(of_signal=2), b"input format 2"), in_format_negative=(dict(of_signal=-1), b"input format -1"),
                 sample_nan=(dict(x=np.where(np.arange(400) == 9, np.nan, x).astype(F32)), b"sample 9 is"),
                 sample_large=(dict(x=np.where(np.arange(400) == 11, -65537.0, x).astype(F32)), b"sample 11 is")))
    assert analysis() == 8 * 15 and np.all(out[120:] == -7.0) and out[:120].any()
    assert analysis(x=None, length=0, out=None) == 0 and analysis(length=3, phase=3, out=None) == 0 and L.speechPlayer_lastErrorCode() == 0
    out[:] = -7.0

    res = np.full(500, -7, np.int16)
    coeff = np.full((8, 4), 0.25)

    def inverse(x=pcm, of_signal=None, length=400, order=4, hop=50, phase=0, coeff=coeff, what=0, fmt=0, res=res, capacity=500):
        if of_signal is None:
            return L.speechPlayer_pcmLpcResidual(p(x), length, order, hop, phase, p(coeff), what, fmt, p(res), capacity)
        return L.speechPlayer_signalLpcResidual(p(x), of_signal, length, order, hop, phase, p(coeff), what, fmt, p(res), capacity)

    def refused_inverse(call, name, table):
        for case, (kw, words) in table.items():
            assert call(**kw) == -1, (name, case)
            err = L.speechPlayer_lastError()
            assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and name in err and words in err, (name, case, err)
            assert np.all(res == -7), (name, case)
    table = dict(common, what_2=(dict(what=2), b"what 2"), what_negative=(dict(what=-1), b"what -1"), format_2=(dict(fmt=2), b"format 2"), no_coefficients=(dict(coeff=None), b"no coefficients"),
                 no_output=(dict(res=None), b"no output"), capacity_short=(dict(capacity=399), b"capacity is 399"))
    refused_inverse(inverse, b"pcmLpcResidual", table)
    refused_inverse(lambda **kw: inverse(**{**dict(x=x, of_signal=1), **kw}), b"signalLpcResidual",
                    dict(table, in_format_2=(dict(of_signal=2), b"input format 2"), sample_inf=(dict(x=np.where(np.arange(400) == 5, np.inf, x).astype(F32)), b"sample 5 is")))
    assert inverse() == 400 and np.all(res[400:] == -7) and res[:400].any()
    assert inverse(x=None, length=0, coeff=None, res=None, capacity=0) == 0 and inverse(length=3, phase=3, coeff=None) == 3 and L.speechPlayer_lastErrorCode() == 0

    a, k, e, st = np.full(4, -7.0), np.full(4, -7.0), np.full(1, -7.0), np.full(1, -7, np.int32)
    r = np.array([1.0, 0.5, 0.25, 0.125, 0.0625])
    for order, rr, words in ((0, r, b"order 0"), (33, r, b"order 33"), (4, None, b"no autocorrelation")):
        assert L.speechPlayer_lpcFromAutocorrelation(p(rr), order, p(a), p(k), p(e), p(st)) == -1
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"lpcFromAutocorrelation" in L.speechPlayer_lastError() and words in L.speechPlayer_lastError()
        assert np.all(a == -7) and np.all(k == -7) and e[0] == -7 and st[0] == -7
    assert L.speechPlayer_lpcFromAutocorrelation(p(r), 4, None, None, None, None) == 4
    assert L.speechPlayer_lpcFromAutocorrelation(p(r), 4, p(a), p(k), p(e), p(st)) == 4 and a[0] == -0.5 and st[0] == 4 and e[0] == 0.75


# ---- 5. the kernels' walks ---------------------------------------------------------------------------------------------------------------------
def test_the_kernels_walks_under_sanitizers(tmp_path):
    """csrc/klatt_lpc.h and klatt_tiles.h in a program of its own, tests/native/check_lpc.cpp, under AddressSanitizer + UBSan: both kernels'
    walks modelled on the host against brute force -- 64-step groups, lane-strided partials, the tree, a lane per step, tiles with their
    coefficient-row staging, padded and packed outputs, misaligned first elements, rows of 0, 1, 63, 64 and 65 steps and of the tile's
    length and one either side.  The program is run directly: nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_lpc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_lpc.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and int(out.split()[1]) > 1000000, out
