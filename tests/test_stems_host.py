"""The signal stems of a batch on the host (include/speechPlayer_batch.h: speechPlayer_batch_exportStems,
speechPlayer_resonatorCoefficients): declarations and bindings, the argument checks of BatchPlayer.stemTensor, the host coefficients
against the C library's formula within a derived bound -- and `stems`, the comparand of tests/test_gpu_stems.py: the header's definition
restated one sample at a time in plain Python floats over `walk` (tests/test_timeline_host.py) and the glottal phase of `source`
(tests/test_source_host.py), itself held to the oracle's PCM here on every sample.  No GPU."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import oracle, scenarios
from tests.test_source_host import PHASE, source
from tests.test_timeline_host import utterance, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
VOICE, ASPIRATION, SOURCE, FRICATION, CASCADE, PARALLEL, OUTPUT = range(7)
# resonator r (N0, NP, c6 .. c1, p1 .. p6) reads frequency parameter RES_F[r] and bandwidth parameter RES_B[r]
RES_F = (13, 14, 12, 11, 10, 9, 8, 7, 25, 26, 27, 28, 29, 30)
RES_B = (21, 22, 20, 19, 18, 17, 16, 15, 31, 32, 33, 34, 35, 36)
NAN = float("nan")


def same(got, want):
    """Equality of bits, NaN standing for NaN and zeros equal whatever their sign."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    g, w = np.where(got == 0, 0, got).astype(got.dtype), np.where(want == 0, 0, want).astype(want.dtype)      # -0 -> +0
    return bool(np.array_equal(gn, wn) and np.array_equal(g.view(bits)[~gn], w.view(bits)[~wn]))


def c_exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def c_cos(x):
    return math.cos(x) if math.isfinite(x) else NAN


def libm_coefficients(f, bw, anti, sr):
    """(a, b, c) of reference src/speechWaveGenerator.cpp:116-124 with the C library's exp and cos, one IEEE operation at a time:
    arrays f, bw -> float64 [n, 3]."""
    out = np.zeros((len(f), 3))
    with np.errstate(all="ignore"):
        for i, (fi, bi) in enumerate(zip(np.asarray(f, dtype=np.float64).tolist(), np.asarray(bw, dtype=np.float64).tolist())):
            rad = c_exp(-math.pi / sr * bi)
            c = -(rad * rad)
            b = rad * c_cos((math.pi * 2) / sr * -fi) * 2.0
            a = 1.0 - b - c
            if anti and fi != 0:
                a = float(np.float64(1.0) / np.float64(a))      # (a plain Python division raises at zero)
                c *= -a
                b *= -a
            out[i] = (a, b, c)
    return out


def native_coefficients(f, bw, anti, sr):
    """speechPlayer_resonatorCoefficients: the product's statement of the device's coefficients."""
    from nvspeechplayer_amd import speechPlayer
    return speechPlayer.resonatorCoefficients(f, bw, sr, anti=anti)


def in_documented_range(cur, sr):
    """Every frequency and bandwidth of cur [L, 47] is finite and inside the range in which speechPlayer_resonatorCoefficients returns
    the device's bits: |pi bw / sr| <= 700 and |2 pi f / sr| <= 1e4."""
    f, bw = cur[:, list(RES_F)], cur[:, list(RES_B)]
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.isfinite(f)) and np.all(np.isfinite(bw)) and np.all(np.abs(math.pi * bw / sr) <= 700.0) and
                    np.all(np.abs(2 * math.pi * f / sr) <= 1.0e4))


@functools.lru_cache(maxsize=None)
def noise_uniform(seed, count):
    """u(k) = n(k) / 2147483647 for k < count, n(k) the oracle's klatt_noise31 (frozen by tests/test_oracle_golden.py)."""
    n31 = oracle.lib().klatt_noise31
    return [n31(seed, k) / 2147483647 for k in range(count)]


def hold_lerp(frm, to, r):
    return frm if to != to else frm + (to - frm) * r


def stems(cur, P, seed, sr, coef):
    """The definition of include/speechPlayer_batch.h over cur [L, 47] (walk) and the glottal phase P [L]: -> float64 [L, 7].  Plain
    Python floats: every operation is one IEEE binary64 operation, in the order the header gives.  coef(f [L], bw [L], anti, sr) ->
    [L, 3]: the resonator coefficients of every sample."""
    cur = np.asarray(cur, dtype=np.float64)
    L = len(cur)
    u = noise_uniform(int(seed), 2 * L)
    abc = [np.asarray(coef(cur[:, RES_F[r]], cur[:, RES_B[r]], r == 0, sr), dtype=np.float64).tolist() for r in range(14)]
    z1, z2 = [0.0] * 14, [0.0] * 14
    A = F = 0.0
    out = np.zeros((L, 7))

    def res(r, t, x):
        a, b, c = abc[r][t]
        y = (a * x + b * z1[r]) + c * z2[r]
        z2[r] = z1[r]
        z1[r] = x if r == 0 else y      # the anti-resonator's memory takes the input
        return y

    for t, (f, p) in enumerate(zip(cur.tolist(), np.asarray(P, dtype=np.float64).tolist())):
        A = u[2 * t] + 0.75 * A
        asp = A * 0.2
        turb = asp * f[3]
        if not p >= f[4]:
            turb = turb * 0.01
        voice = ((p * 2 - 1) + turb) * f[5]
        aspiration = asp * f[6]
        src = aspiration + voice
        x = (src * f[44]) * 0.5
        n0 = res(0, t, x)
        np_ = res(1, t, n0)
        o = hold_lerp(x, np_, f[23])
        for r in range(2, 8):
            o = res(r, t, o)
        F = u[2 * t + 1] + 0.75 * F
        fric = F * 0.3 * f[24]
        y = (fric * f[44]) * 0.5
        par = 0.0
        for k in range(6):
            par = par + (res(8 + k, t, y) - y) * f[37 + k]
        par = hold_lerp(par, y, f[43])
        out[t] = (voice, aspiration, src, fric, o, par, ((o + par) * f[45]) * 4000.0)
    return out


def to_pcm(output):
    """(int)max(min(OUTPUT, 32000), -32000) with windows.h's min / max (NaN becomes 32000), truncated toward zero."""
    v = np.asarray(output, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lo = np.where(v < 32000.0, v, 32000.0)
        cl = np.where(lo > -32000.0, lo, -32000.0)
    return np.trunc(cl).astype(np.int16)


class Stemmed:
    """A batch at a sample rate: per utterance the walk's frames, and the oracle's PCM of the whole batch, computed when first asked for."""

    def __init__(self, batch, sr=22050):
        self.b, self.sr = batch, sr
        self.n = len(batch["frame_start"]) - 1
        self._cur, self._pcm = {}, None

    def cur(self, u):
        if u not in self._cur:
            self._cur[u] = walk(*utterance(self.b, u))[0]
        return self._cur[u]

    def seed(self, u):
        return int(self.b["seeds"][u])

    def length(self, u):
        return len(self.cur(u))

    def pcm(self, u):
        if self._pcm is None:
            self._pcm = oracle.batch_synthesize(self.sr, self.b)[:2]
        pcm, start = self._pcm
        return pcm[int(start[u]):int(start[u + 1])]


@functools.lru_cache(maxsize=None)
def compared(name):
    """The batches tests/test_gpu_stems.py compares, computed once per process."""
    if name == "plain":
        return Stemmed(scenarios.random_batch(np.random.default_rng(21), 10))
    if name == "plain16k":
        return Stemmed(scenarios.random_batch(np.random.default_rng(21), 10), sr=16000)
    if name == "wild":
        return Stemmed(scenarios.random_batch(np.random.default_rng(22), 10, wild=True))
    raise KeyError(name)


def test_entry_points_are_declared_exported_and_bound():
    from nvspeechplayer_amd import _native, speechPlayer
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name in ("speechPlayer_batch_exportStems", "speechPlayer_resonatorCoefficients"):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and fn.argtypes, name
    assert len(L.speechPlayer_batch_exportStems.argtypes) == 9 and len(L.speechPlayer_resonatorCoefficients.argtypes) == 6
    for k, name in enumerate(("VOICE", "ASPIRATION", "SOURCE", "FRICATION", "CASCADE", "PARALLEL", "OUTPUT", "COLUMNS")):
        assert any(line.split()[:3] == ["#define", "SPEECHPLAYER_STEM_" + name, str(k)] for line in header.splitlines()), name
    assert speechPlayer.STEM_COLUMNS == ["voice", "aspiration", "source", "frication", "cascade", "parallel", "output"]
    assert callable(speechPlayer.BatchPlayer.stemTensor) and callable(speechPlayer.resonatorCoefficients)
    import nvspeechplayer_amd
    assert nvspeechplayer_amd.resonatorCoefficients is speechPlayer.resonatorCoefficients


def test_a_null_batch_is_an_argument_error():
    from nvspeechplayer_amd import _native
    L = _native.load()
    cols = np.array([6], np.int32)
    assert L.speechPlayer_batch_exportStems(None, None, 0, cols.ctypes.data, 1, None, 1, 0, None) == -1
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"exportStems" in L.speechPlayer_lastError()
    assert L.speechPlayer_resonatorCoefficients(None, None, 1, 0, 22050, None) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT
    assert L.speechPlayer_resonatorCoefficients(None, None, 0, 0, 22050, None) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert L.speechPlayer_resonatorCoefficients(None, None, 0, 0, 0, None) == -1


def test_stem_request_checks():
    import torch
    from nvspeechplayer_amd.speechPlayer import STEM_COLUMNS, check_stem_request
    cols, fmt = check_stem_request(STEM_COLUMNS, None)
    assert cols.dtype == np.int32 and list(cols) == list(range(7)) and fmt == 1
    cols, fmt = check_stem_request(["output", 2, np.int64(2), "voice"], torch.float64)
    assert list(cols) == [6, 2, 2, 0] and fmt == 0
    assert list(check_stem_request("source", torch.float32)[0]) == [2] and list(check_stem_request(5, None)[0]) == [5]
    with pytest.raises(KeyError):
        check_stem_request(["wave"], None)
    for bad in ([7], [-1], [0, 7], []):
        with pytest.raises(ValueError):
            check_stem_request(bad, None)
    for dtype in (torch.float16, torch.int16, np.float32):
        with pytest.raises(TypeError):
            check_stem_request([0], dtype)


@pytest.mark.parametrize("name", ["plain", "plain16k", "wild"])
def test_the_restatement_gives_the_oracles_pcm_on_every_sample(name):
    """With the C library's coefficients (reference :116-124) and P from source(), the truncated OUTPUT is the oracle's PCM on every
    sample of random_batch(default_rng(21), 10) at 22 050 and 16 000 Hz and of random_batch(default_rng(22), 10, wild=True); and the
    columns obey the definition's own identities."""
    s = compared(name)
    samples = 0
    for u in range(s.n):
        cur = s.cur(u)
        st = stems(cur, source(cur, s.sr)[0][:, PHASE], s.seed(u), s.sr, libm_coefficients)
        want = s.pcm(u)
        assert len(st) == len(want), u
        differ = np.flatnonzero(to_pcm(st[:, OUTPUT]) != want)
        assert len(differ) == 0, (u, len(differ), int(differ[0]))
        with np.errstate(all="ignore"):
            assert same(st[:, SOURCE], st[:, ASPIRATION] + st[:, VOICE]), u
            assert same(st[:, OUTPUT], (st[:, CASCADE] + st[:, PARALLEL]) * cur[:, 45] * 4000.0), u
        samples += len(st)
    assert samples == (61253 if name == "wild" else 22473)


def test_host_coefficients_special_cases():
    from nvspeechplayer_amd.speechPlayer import resonatorCoefficients
    assert resonatorCoefficients(0.0, 0.0, 22050).tolist() == [[0.0, 2.0, -1.0]]
    assert resonatorCoefficients(0.0, 0.0, 22050, anti=True).tolist() == [[0.0, 2.0, -1.0]]
    # an anti-resonator at f == 0 is not inverted: the pole form's coefficients
    assert resonatorCoefficients([0.0, 0.0], [90.0, 300.0], 22050, anti=True).tolist() == resonatorCoefficients([0.0, 0.0], [90.0, 300.0], 22050).tolist()
    inv, pole = resonatorCoefficients(270.0, 100.0, 22050, anti=True)[0], resonatorCoefficients(270.0, 100.0, 22050)[0]
    assert inv[0] == 1.0 / pole[0] and inv[1] == pole[1] * -inv[0] and inv[2] == pole[2] * -inv[0]
    assert resonatorCoefficients([], [], 16000).shape == (0, 3)
    with pytest.raises(ValueError):
        resonatorCoefficients([1.0, 2.0], [1.0], 22050)
    with pytest.raises(ValueError):
        resonatorCoefficients([1.0], [1.0], 0)
    # outside the documented range: the C library's exp and cos
    far = resonatorCoefficients([5.0e7], [-6.0e6], 22050)
    assert np.array_equal(far, libm_coefficients([5.0e7], [-6.0e6], False, 22050))


def test_host_coefficients_against_the_c_library():
    """f in [0, 5500] Hz, bw in [30, 1000] Hz at 22 050 Hz.  Pole resonators: each of a, b, c within 2^-47 ABSOLUTE of the C library's
    formula -- rad = exp(.) <= 1 with <= 1 ulp (2^-53 relative to a value below 1: 2^-53) against glibc's < 1 ulp, cos <= 1.5 ulp against
    < 1 ulp, so b = 2 rad cos differs by less than 2 (2 + 2.5) 2^-53 and c = rad^2 by less than 2 * 2 * 2^-53, plus the five roundings
    of values of magnitude <= 2 (|b| <= 2, |c| <= 1, |a| <= 4): below 2^-47 in all.  The anti-resonator with f != 0 inverts a: the relative
    error of 1 / a is that of a, so each coefficient is within 2^-44 * max(1, |1 / a|) RELATIVE."""
    from nvspeechplayer_amd.speechPlayer import resonatorCoefficients
    rng = np.random.default_rng(31)
    f = np.concatenate([[0.0, 5500.0, 0.0, 5500.0], rng.uniform(0.0, 5500.0, 4000)])
    bw = np.concatenate([[30.0, 30.0, 1000.0, 1000.0], rng.uniform(30.0, 1000.0, 4000)])
    got, want = resonatorCoefficients(f, bw, 22050), libm_coefficients(f, bw, False, 22050)
    assert np.all(np.isfinite(got)) and float(np.abs(got - want).max()) <= 2.0 ** -47
    nz = f != 0
    got_anti, want_anti = resonatorCoefficients(f[nz], bw[nz], 22050, anti=True), libm_coefficients(f[nz], bw[nz], True, 22050)
    tol = 2.0 ** -44 * np.maximum(1.0, np.abs(1.0 / want[nz, 0]))[:, None]
    assert np.all(np.isfinite(got_anti)) and np.all(np.abs(got_anti - want_anti) <= tol * np.abs(want_anti))
