"""The tempo exports on the host (include/speechPlayer_batch.h: speechPlayer_tempoLength, tempoFrames, pcmTempo, signalTempo;
nvspeechplayer_amd.pcmTempo, signalTempo, tempoLength, tempoFrames, tempoMap, check_tempo_request; csrc/klatt_tempo.h): a transcription of
the definition written here in numpy, independent of the shared header, held to the statements bit for bit, positions and samples; the
exact cases; the periodic and the pitch property, each with plain overlap-add failing it; every refusal; tempoMap against a loop; and a
model of both kernels' walks in a program of its own under the sanitizers (tests/native/check_tempo.cpp).  `transcription` and `same`
are what tests/test_gpu_tempo.py shares.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_lpc_host import bits, float_row, golden_pcm, segment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
F32, F64 = np.float32, np.float64
SPEECH = "ipa_l15_s10_c0_p100_i05"
VOWEL = "cfg0_a_1s"
TEMPOS = (0.25, 0.8, 1.0, 1.1, 4.0)


def same(got, want):
    """Equality of type, shape and every bit."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- the transcription of the definition, in numpy -------------------------------------------------------------------------------------------
def t_x(row):
    return row.astype(F32) / F32(32767.0) if row.dtype == np.int16 else row.astype(F32)


def t_at(x, s, n=None):
    """x(s .. s + n - 1), or x at the int64 array s: +0 outside the row."""
    idx = np.arange(s, s + n, dtype=np.int64) if n is not None else np.asarray(s, np.int64)
    ok = (idx >= 0) & (idx < len(x))
    out = np.zeros(idx.shape, F32)
    out[ok] = x[idx[ok]]
    return out


def t_window(N):
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / N) for i in range(N)], F64).astype(F32)


def t_lengths(L, tempo, N):
    Lout = int(math.ceil(float(L) / tempo)) if L else 0
    return Lout, (-(-Lout // (N // 2)) + 1 if Lout else 0)


def t_scores(T, R, N, D):
    """score(d) for d = -D .. D: the four chains of exact products, each summed in ascending i from +0.0."""
    C = np.lib.stride_tricks.sliding_window_view(R.astype(F64), N)[:2 * D + 1]
    terms = T.astype(F64)[None, :] * C      # exact: 24 x 24 bits
    c = np.zeros((2 * D + 1, 4), F64)
    for i in range(0, N - N % 4, 4):
        c = c + terms[:, i:i + 4]
    if N % 4:
        c[:, :2] = c[:, :2] + terms[:, N - 2:]
    return (c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3])


def t_positions(x, tempo, N, D, K):
    Hs = N // 2
    p = np.zeros(K, np.int64)
    d = np.arange(-D, D + 1)
    rank = 2 * np.abs(d) - (d < 0)
    for k in range(1, K):
        a = int(math.floor(float(k * Hs) * tempo))
        s = t_scores(t_at(x, int(p[k - 1]), N), t_at(x, a - Hs - D, N + 2 * D), N, D)
        best = np.flatnonzero(s == s.max())
        p[k] = a + d[best[np.argmin(rank[best])]]
    return p


def fmaf(a, b, c):
    """float32 a * b + c rounded once, elementwise: the product is exact in binary64; the binary64 sum is rounded twice on the way to
    binary32 only where it lands on a binary32 tie that the exact sum is not -- TwoSum's error says which way that one goes."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (err != 0)
    s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def t_int16(y):
    q = y * F32(32767.0)
    return np.where(q >= F32(32767.0), 32767, np.where(q <= F32(-32768.0), -32768, np.rint(q))).astype(np.int16)


def t_render(x, N, Lout, p, dtype):
    Hs, w = N // 2, t_window(N)
    P = np.clip(np.asarray(p, np.int64), -(1 << 45), 1 << 45)
    m = np.arange(Lout, dtype=np.int64)
    q, i = m // Hs, m % Hs
    if not Lout:
        return np.zeros(0, dtype)
    y = fmaf(w[Hs + i], t_at(x, P[q] + i), w[i] * t_at(x, P[q + 1] - Hs + i)) + F32(0.0)
    return y if dtype == F32 else t_int16(y)


def transcription(row, tempo, N, D, dtype=F32, positions=None):
    """-> (y, p) of a row by the definition."""
    x = t_x(row)
    Lout, K = t_lengths(len(x), tempo, N)
    p = t_positions(x, tempo, N, D, K) if positions is None else np.asarray(positions, np.int64)
    return t_render(x, N, Lout, p, dtype), p


def statement(row, *args, **kw):
    import nvspeechplayer_amd as eng
    return (eng.pcmTempo if row.dtype == np.int16 else eng.signalTempo)(row, *args, **kw)


# ---- 1. the statements against the transcription ------------------------------------------------------------------------------------------------
def test_fmaf_of_the_transcription():
    """The rounding of the transcription's fmaf against exact rational arithmetic, on values made to land near binary32 ties."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.uniform(-2, 2, 4000).astype(F32)
    b = rng.uniform(-2, 2, 4000).astype(F32)
    c = rng.uniform(-2, 2, 4000).astype(F32)
    c[:2000] = (np.ldexp(F32(1.0), rng.integers(-30, 0, 2000)) * 1.5).astype(F32)      # half ulps of small products
    a[:2000] = np.ldexp(F32(1.0), rng.integers(-3, 3, 2000)).astype(F32) * F32(1.0000001)
    got = fmaf(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = sorted((float(np.nextafter(got[i], F32(-np.inf))), float(np.nextafter(got[i], F32(np.inf)))))
        assert abs(exact - Fraction(float(got[i]))) <= min(abs(exact - Fraction(lo)), abs(exact - Fraction(hi))), i


@pytest.mark.parametrize("D", [0, 1, 31, 160])
@pytest.mark.parametrize("N", [64, 512])
def test_the_statements_are_the_transcriptions_bits(N, D):
    """Rows of length 0, 1, Hs - 1, Hs, Hs + 1, N and 5N + 3 cut from a golden utterance (a silence, an onset, voiced sound), int16 and
    float32, at every tempo: positions and samples, float32 and int16 outputs in turn."""
    import nvspeechplayer_amd as eng
    Hs, k = N // 2, 0
    for L in (0, 1, Hs - 1, Hs, Hs + 1, N, 5 * N + 3):
        seg = segment(SPEECH, L)
        for row in (seg, float_row(seg)):
            for tempo in TEMPOS:
                dtype = (F32, np.int16)[k % 2]
                k += 1
                y, p = statement(row, tempo, N, D, dtype=dtype, returnPositions=True)
                wy, wp = transcription(row, tempo, N, D, dtype)
                tag = (N, D, L, row.dtype, tempo)
                assert len(p) == eng.tempoFrames(L, tempo, N) == len(wp) and len(y) == eng.tempoLength(L, tempo) == len(wy), tag
                assert np.array_equal(p, wp), tag
                assert same(y, wy), tag
    assert k == 70


def test_the_widest_search():
    """N = 2048, D = 1024 on 5N + 3 samples of the vowel."""
    row = golden_pcm(VOWEL)[3000:3000 + 5 * 2048 + 3].copy()
    for r, tempo, dtype in ((row, 1.1, F32), (float_row(row), 0.8, np.int16)):
        y, p = statement(r, tempo, 2048, 1024, dtype=dtype, returnPositions=True)
        wy, wp = transcription(r, tempo, 2048, 1024, dtype)
        assert np.array_equal(p, wp) and same(y, wy) and np.any(p[1:] != np.floor(np.arange(1, len(p)) * 1024 * tempo)), tempo


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------------
def nominal(K, Hs, tempo):
    return np.array([int(math.floor(float(k * Hs) * tempo)) for k in range(K)], np.int64)


def test_silent_and_constant_rows_take_lag_zero():
    """Zeros and -0.0: every score is +0 and every frame of every tempo takes d = 0.  A constant: every frame at tempo 1 -- where the
    template runs off the row's end the candidates tie over its support -- and, at other tempos, every frame whose template and
    candidates lie inside the row (a candidate that hangs over the row's start scores less: that is no tie)."""
    for row in (np.zeros(3000, np.int16), np.full(3000, 1234, np.int16), np.full(3000, -0.0, F32), np.full(3000, 0.37, F32)):
        p = statement(row, 1.0, 256, 40, returnPositions=True)[1]
        assert np.array_equal(p, nominal(len(p), 128, 1.0)), row.dtype
        for tempo in (0.8, 1.1):
            y, p = statement(row, tempo, 256, 40, returnPositions=True)
            inner = [k for k in range(1, len(p)) if p[k - 1] >= 0 and p[k - 1] + 256 <= 3000 and nominal(len(p), 128, tempo)[k] - 128 - 40 >= 0
                     and nominal(len(p), 128, tempo)[k] + 128 + 40 <= 3000]
            full = np.array_equal(p, nominal(len(p), 128, tempo))
            if not row.any():
                assert full and not bits(y).any(), (row.dtype, tempo)      # every score +0: rank 0, and +0 samples even of -0
            else:
                assert len(inner) > 5 and np.array_equal(p[inner], nominal(len(p), 128, tempo)[inner]), (row.dtype, tempo)      # (at the row's ends a constant's score falls off: not a tie)


def test_no_search_at_tempo_one_is_the_input_within_two_roundings():
    """D = 0, tempo 1: y(m) = w[Hs + i] x + w[i] x with w[i] + w[i + Hs] = 1 +- 2^-24: |y - x| <= 4 * 2^-24 |x|."""
    for N in (64, 512, 2048):
        seg = segment(SPEECH, 4000)
        for row in (seg, float_row(seg)):
            y, p = statement(row, 1.0, N, 0, returnPositions=True)
            x = t_x(row).astype(F64)
            assert np.array_equal(p, np.arange(len(p)) * (N // 2)) and len(y) == len(x)
            assert np.all(np.abs(y.astype(F64) - x) <= 4 * 2.0 ** -24 * np.abs(x)), N


def test_rendering_the_searchs_positions_and_positions_far_outside():
    row = segment(SPEECH, 3000)
    for r in (row, float_row(row)):
        for dtype in (F32, np.int16):
            y, p = statement(r, 0.8, 128, 31, dtype=dtype, returnPositions=True)
            y2, p2 = statement(r, 0.8, 128, 31, positions=p, dtype=dtype, returnPositions=True)
            assert same(y, y2) and np.array_equal(p, p2)
            for far in (1 << 62, -(1 << 62), (1 << 63) - 1, -(1 << 63)):
                z = statement(r, 0.8, 128, 0, positions=np.full(len(p), far, np.int64), dtype=dtype)
                assert len(z) == len(y) and not bits(z).any(), far
            mixed = p.copy()
            mixed[3], mixed[7] = 1 << 62, -(1 << 62)
            assert same(statement(r, 0.8, 128, 0, positions=mixed, dtype=dtype), transcription(r, 0.8, 128, 0, dtype, positions=mixed)[0])


# ---- 3. the periodic property ----------------------------------------------------------------------------------------------------------------
def test_a_periodic_row_keeps_its_phase():
    """A table of period 32 repeated to 6000 samples, N = 256, D = 40: every inner frame advances by Hs modulo the period, and between two
    inner frames the output is the input's own segment but for the window's two roundings.  Plain overlap-add (D = 0) is off phase on
    more than half of the frames: the property is not vacuous."""
    N, Hs, D, P, L = 256, 128, 40, 32, 6000
    row = np.round(12000 * np.sin(2 * np.pi * np.arange(L) / P)).astype(np.int16)
    assert np.array_equal(row[:-P], row[P:])
    x = t_x(row).astype(F64)
    for tempo in (0.8, 1.1):
        y, p = statement(row, tempo, N, D, returnPositions=True)
        a = nominal(len(p), Hs, tempo)
        inner = np.zeros(len(p), bool)
        for k in range(1, len(p)):
            inner[k] = p[k - 1] >= 0 and p[k - 1] + N <= L and a[k] - Hs - D >= 0 and a[k] - Hs + D + N <= L
        assert inner.sum() > 20
        step = (p[1:] - p[:-1] - Hs) % P
        assert np.all(step[inner[1:]] == 0), tempo
        checked = 0
        for q in range(1, len(p) - 1):
            if inner[q] and inner[q + 1]:      # block q blends the segments of frames q and q + 1: equal samples, weights summing to one
                m = np.arange(q * Hs, min((q + 1) * Hs, len(y)))
                ref = x[p[q] + (m - q * Hs)]
                assert np.all(np.abs(y[m].astype(F64) - ref) <= 4 * 2.0 ** -24 * np.abs(ref)), (tempo, q)
                checked += 1
        assert checked > 20
        _, p0 = statement(row, tempo, N, 0, returnPositions=True)
        off = ((p0[1:] - p0[:-1] - Hs) % P != 0)[inner[1:]]
        assert off.sum() > len(off) / 2, tempo


# ---- 4. the pitch property -------------------------------------------------------------------------------------------------------------------
def pitch_lag(y):
    """The lag in 55 .. 440 of the greatest normalised autocorrelation of the 4000 samples around the middle."""
    mid = len(y) // 2
    s = np.asarray(y[mid - 2000:mid + 2000], F64)
    best, at = -2.0, 0
    for lag in range(55, 441):
        u, v = s[:-lag], s[lag:]
        r = float(u @ v) / math.sqrt(float(u @ u) * float(v @ v))
        if r > best:
            best, at = r, lag
    return at


def test_the_pitch_stays_and_plain_overlap_add_moves_it():
    row = golden_pcm(VOWEL)
    period = pitch_lag(t_x(row))
    assert period == 184
    for tempo in (0.8, 1.25):
        assert abs(pitch_lag(statement(row, tempo, 512, 160)) - period) <= 1, tempo
        assert abs(pitch_lag(statement(row, tempo, 512, 0)) - period) > 1, tempo


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_statements():
    from nvspeechplayer_amd import _native
    L = _native.load()
    pcm = np.arange(-500, 500, dtype=np.int16)
    x = pcm.astype(F32) / F32(32767.0)
    out, pos = np.full(5000, -7, np.int16), np.full(200, -7, np.int64)
    p = lambda a: None if a is None else a.ctypes.data

    def pcm_call(length=1000, tempo=1.0, nWin=64, search=4, posIn=None, fmt=0, o=out, cap=5000, samples=pcm):
        return L.speechPlayer_pcmTempo(p(samples), length, tempo, nWin, search, p(posIn), p(pos), fmt, p(o), cap)

    def signal_call(inFormat=1, length=1000, tempo=1.0, nWin=64, search=4, posIn=None, fmt=0, o=out, cap=5000, samples=x):
        return L.speechPlayer_signalTempo(p(samples), inFormat, length, tempo, nWin, search, p(posIn), p(pos), fmt, p(o), cap)

    bad = x.copy()
    bad[17] = np.inf
    cases = [(dict(length=-1), b"length -1"), (dict(length=(1 << 44) + 1), b"length"), (dict(samples=None), b"without samples"), (dict(tempo=0.2), b"tempo 0.2"),
             (dict(tempo=4.5), b"tempo 4.5"), (dict(tempo=float("nan")), b"tempo nan"), (dict(tempo=float("inf")), b"tempo inf"), (dict(nWin=62), b"nWin 62"),
             (dict(nWin=65), b"nWin 65"), (dict(nWin=2050), b"nWin 2050"), (dict(search=-1), b"search -1"), (dict(search=1025), b"search 1025"), (dict(fmt=2), b"format 2"),
             (dict(cap=999), b"capacity is 999")]
    for fn, entry, more in ((pcm_call, b"pcmTempo", []), (signal_call, b"signalTempo", [(dict(inFormat=2), b"input format 2"), (dict(samples=bad), b"sample 17")])):
        for kw, words in cases + more:
            assert fn(**kw) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, (entry, kw)
            assert entry in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (kw, L.speechPlayer_lastError())
            assert np.all(out == -7) and np.all(pos == -7), kw
    # a null output only sizes, and still fills the positions; an empty row needs nothing
    assert pcm_call(o=None, cap=0, tempo=0.8) == 1250 and pos[0] == 0 and np.all(pos[1:1250 // 32 + 2] > 0) and np.all(pos[1250 // 32 + 2:] == -7) and np.all(out == -7)
    assert pcm_call(length=0, samples=None, o=None, cap=0) == 0 and signal_call(length=0, samples=None, o=None, cap=0) == 0 and L.speechPlayer_lastErrorCode() == 0
    for fn, entry in ((L.speechPlayer_tempoLength, b"tempoLength"), (lambda n, t: L.speechPlayer_tempoFrames(n, t, 64), b"tempoFrames")):
        for n, t in ((-1, 1.0), ((1 << 44) + 1, 1.0), (10, 0.24), (10, 4.01), (10, float("nan"))):
            assert fn(n, t) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and entry in L.speechPlayer_lastError(), (entry, n, t)
    for nWin in (62, 63, 2050, 0, -64):
        assert L.speechPlayer_tempoFrames(10, 1.0, nWin) == -1 and b"nWin" in L.speechPlayer_lastError()
    assert L.speechPlayer_tempoLength(0, 2.0) == 0 and L.speechPlayer_tempoFrames(0, 2.0, 64) == 0
    assert L.speechPlayer_tempoLength(1 << 44, 0.25) == 1 << 46 and L.speechPlayer_tempoFrames(1 << 44, 0.25, 64) == (1 << 41) + 1
    assert L.speechPlayer_tempoLength(10, 3.0) == 4 and L.speechPlayer_tempoFrames(10, 3.0, 64) == 2 and L.speechPlayer_tempoFrames(65, 1.0, 64) == 4


def test_binding_request_checks():
    import torch
    import nvspeechplayer_amd
    from nvspeechplayer_amd import speechPlayer as sp
    ok = dict(tempo=0.8, nWin=512, search=160, dtype=None)
    assert sp.check_tempo_request(**ok) == (0.8, 512, 160, 1) and sp.check_tempo_request(**{**ok, "dtype": torch.int16, "tempo": 4}) == (4.0, 512, 160, 0)
    t, n, d, f = sp.check_tempo_request(1.1, 64, 0, np.int16, rows=3)
    assert t.dtype == F64 and list(t) == [1.1] * 3 and (n, d, f) == (64, 0, 0)
    assert list(sp.check_tempo_request([0.25, 4, 1], 2048, 1024, np.float32, rows=3)[0]) == [0.25, 4.0, 1.0]
    for kw, error, words in ((dict(nWin=62), ValueError, "nWin"), (dict(nWin=513), ValueError, "nWin"), (dict(nWin=2050), ValueError, "nWin"), (dict(nWin=512.0), ValueError, "nWin"),
                             (dict(nWin=True), ValueError, "nWin"), (dict(search=-1), ValueError, "search"), (dict(search=1025), ValueError, "search"), (dict(search=1.5), ValueError, "search"),
                             (dict(tempo=0.2), ValueError, "tempo of row 0 is 0.2"), (dict(tempo=float("nan")), ValueError, "tempo of row 0"), (dict(tempo=4.1), ValueError, "tempo of row 0"),
                             (dict(tempo=[1.0, 2.0]), ValueError, "one number"), (dict(tempo="fast"), TypeError, "tempo must be a number"), (dict(dtype=np.float64), TypeError, "dtype"),
                             (dict(tempo=[1.0, 2.0], rows=3), ValueError, "one per row"), (dict(tempo=[1.0, 9.0, 1.0], rows=3), ValueError, "tempo of row 1 is 9.0")):
        with pytest.raises(error, match=words):
            sp.check_tempo_request(**{**ok, **kw})
    row = np.arange(300, dtype=np.int16)
    with pytest.raises(ValueError, match="3 positions for 11 frames"):
        sp.pcmTempo(row, 1.0, 64, 0, positions=[0, 1, 2])
    with pytest.raises(TypeError, match="int16"):
        sp.pcmTempo(row.astype(np.int32), 1.0)
    with pytest.raises(TypeError, match="int16 or float32"):
        sp.signalTempo(row.astype(F64), 1.0)
    with pytest.raises(ValueError, match="tempo"):
        sp.tempoLength(10, 5.0)
    with pytest.raises(ValueError, match="nWin"):
        sp.tempoFrames(10, 1.0, 63)
    for L in (0, 1, 31, 32, 33, 1000, 22050, (1 << 44) - 1):      # numpy's lengths are the library's
        for tempo in TEMPOS + (1.0 / 3, 3.9999999):
            assert int(sp._tempo_lengths(L, tempo)) == sp.tempoLength(L, tempo) == t_lengths(L, tempo, 64)[0]
            assert int(sp._tempo_frames(sp._tempo_lengths(L, tempo), 64)) == sp.tempoFrames(L, tempo, 64) == t_lengths(L, tempo, 64)[1]
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_tempo.h")).read()
    import re
    for const, value in (("kTempoMaxWin", sp.TEMPO_MAX_WIN), ("kTempoMaxSearch", sp.TEMPO_MAX_SEARCH), ("kTempoTile", sp.TEMPO_TILE)):
        assert int(re.search(r"\b%s = (\d+)" % const, shared).group(1)) == value, const
    between = shared.split("namespace klatt {")[1].split("// ---- the device")[0]
    assert "#if" not in between      # nothing between the shared functions changes arithmetic from one side to the other
    for name in ("check_tempo_request", "tempoLength", "tempoFrames", "pcmTempo", "signalTempo", "tempoMap", "TEMPO_MAX_WIN", "TEMPO_MAX_SEARCH", "TEMPO_TILE"):
        assert getattr(nvspeechplayer_amd, name) is getattr(sp, name) and name in nvspeechplayer_amd.__all__, name
    assert callable(sp.BatchPlayer.tempoTensor) and callable(sp.BatchPlayer.tempoPositionsTensor)


# ---- 6. the time map -------------------------------------------------------------------------------------------------------------------------
def test_the_time_map_against_a_loop():
    import nvspeechplayer_amd as eng
    row = segment(SPEECH, 3000)
    for tempo, N in ((0.8, 64), (1.1, 512), (4.0, 66), (1.0, 2048)):
        y, p = eng.pcmTempo(row, tempo, N, 20, returnPositions=True)
        Hs = N // 2
        want = []
        for m in range(len(y)):
            q, i = divmod(m, Hs)
            want.append(p[q] + i if i < Hs / 2 else p[q + 1] - Hs + i)
        got = eng.tempoMap(p, N, len(y))
        assert got.dtype == np.int64 and list(got) == want, (tempo, N)
        assert abs(int(got[-1]) - 3000) < N + 20 and np.all(np.diff(got[:len(got) // 2]) >= -N)
    assert len(eng.tempoMap([], 64, 0)) == 0
    with pytest.raises(ValueError, match="positions"):
        eng.tempoMap([0, 32], 64, 65)
    with pytest.raises(ValueError, match="nWin"):
        eng.tempoMap([0, 32], 63, 10)


# ---- 7. the kernels' walks -------------------------------------------------------------------------------------------------------------------
def test_the_kernels_walks_under_sanitizers(tmp_path):
    """csrc/klatt_tempo.h and klatt_tiles.h in a program of its own, tests/native/check_tempo.cpp, under AddressSanitizer + UBSan: the
    search's lanes over lags, its butterfly and its reduction across wavefronts against a linear scan with planted ties; the render's
    tiles with staged positions, padded and packed, misaligned first elements, rows around the tile's length and row offsets beyond
    2^32.  The program is run directly: nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_tempo")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_tempo.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and int(out.split()[1]) > 100000, out
