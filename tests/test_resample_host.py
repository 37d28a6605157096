"""The resampler on the host (include/speechPlayer_batch.h: speechPlayer_pcmResample, speechPlayer_resampleKernel,
speechPlayer_resampledLength; nvspeechplayer_amd.pcmResample, resampleKernel, check_resample_request; csrc/klatt_resample.h): the table
against a numpy float64 restatement of the header's formulas, the filter's passband and stopband, the product's CPU statement against
the float64 sum of the same float32 operands within the inner-product bound, a sine that pins the time origin, the int16 conversion,
equal rates, lengths and every refusal.  `restated`, `reference`, `PAIRS` and `FILTERS` are the comparands tests/test_gpu_resample.py
shares.  No GPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_spectrogram_host import signals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
U = 2.0 ** -24
PAIRS = [(22050, 16000), (22050, 24000), (22050, 44100), (22050, 11025), (16000, 22050), (44100, 48000), (7, 5)]
FILTERS = [dict(zeros=6, window="hann"), dict(zeros=2, window="hann"), dict(zeros=16, window="kaiser", beta=8.6), dict(zeros=64, window="kaiser", beta=8.6)]


def ratio(sr, out):
    g = math.gcd(sr, out)
    return out // g, sr // g


def restated(sr, out, zeros=6, rolloff=0.99, window="hann", beta=8.6):
    """The header's table in numpy float64, written from its formulas: -> (h [up, taps], up, down, Z, Wd)."""
    up, down = ratio(sr, out)
    c = rolloff * min(1.0, up / down)
    Wd = zeros / c
    Z = math.ceil(Wd)
    i = np.arange(2 * Z) - Z + 1
    t = i[None, :] - np.arange(up)[:, None] / up
    if window == "hann":
        w = np.cos(np.pi * t / (2 * Wd)) ** 2
    else:
        w = np.i0(beta * np.sqrt(np.maximum(0.0, 1 - (t / Wd) ** 2))) / np.i0(beta)
    w = np.where(np.abs(t) >= Wd, 0.0, w)
    return c * np.sinc(c * t) * w, up, down, Z, Wd


def reference(pcm, table, up, down):
    """The definition's sum in float64 over the float32 operands (the float32 products are exact in binary64): -> (y [Lout], sum |x| |h|)."""
    L, taps = len(pcm), table.shape[1]
    Z = taps // 2
    Lout = -(-L * up // down)
    x = np.zeros(L + 2 * Z, np.float32)
    x[Z:Z + L] = pcm.astype(np.float32) / np.float32(32767.0)
    m = np.arange(Lout, dtype=np.int64)
    n0, p = m * down // up, m * down % up
    at = n0[:, None] + np.arange(taps)[None, :] - Z + 1 + Z
    terms = x[at].astype(np.float64) * table[p]
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def gamma(taps):
    """gamma_K of Higham, Accuracy and Stability of Numerical Algorithms, chapter 3: the inner product of K float32 terms."""
    return taps * U / (1 - taps * U)


def gains(table, up, f, sr):
    """G_p(f) = sum_k h[p][k] exp(j 2 pi f (i - p / up) / sr) for every phase p."""
    taps = table.shape[1]
    t = (np.arange(taps) - taps // 2 + 1)[None, :] - np.arange(up)[:, None] / up
    return (table * np.exp(2j * np.pi * f * t / sr)).sum(axis=1)


def to_int16(y):
    """Format 0 of float32 values, as the header states it."""
    q = y.astype(np.float32) * np.float32(32767.0)
    return np.where(q >= 32767, 32767, np.where(q <= -32768, -32768, np.rint(q))).astype(np.int16)


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs in (("speechPlayer_batch_exportResampled", 12), ("speechPlayer_pcmResample", 11), ("speechPlayer_resampleKernel", 11),
                        ("speechPlayer_resampledLength", 3)):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and len(fn.argtypes) == nargs, name
    section = header.split("A batch's PCM at another sample rate")[1].split("speechPlayer_resampledLength(")[0]
    assert "MODE_FAST" in section and "depends on the" in section      # the dependence on the PCM, and so on the mode, is stated
    for word in ("live handles", "NodePlayer", "label grid"):           # what is out of scope
        assert word in section, word
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_resample.h")).read()
    tile = int(re.search(r"constexpr int kResampleTile = (\d+);", shared).group(1))
    assert speechPlayer.RESAMPLE_TILE == tile and tile & (tile - 1) == 0 and tile <= 4096
    assert "kResampleTile = %d" % tile in header
    assert callable(speechPlayer.BatchPlayer.resampledTensor)
    assert nvspeechplayer_amd.pcmResample is speechPlayer.pcmResample and nvspeechplayer_amd.resampleKernel is speechPlayer.resampleKernel


@pytest.mark.parametrize("sr,out", PAIRS)
def test_the_table_against_the_formulas(sr, out):
    """Every tap within np.spacing(|h32|) + 2^-44 of the float64 restatement rounded to float32: two binary64 evaluations may straddle a
    float32 rounding boundary, and the argument of the sinc is rounded (at most 8 * 2^-52 per tap, with margin for sin and I0)."""
    import nvspeechplayer_amd as eng
    for kw in FILTERS:
        table, up, down = eng.resampleKernel(sr, out, **kw)
        want, wup, wdown, Z, Wd = restated(sr, out, **kw)
        assert (up, down) == (wup, wdown) == ratio(sr, out)
        assert table.shape == (up, 2 * Z) == want.shape and table.dtype == np.float64
        assert np.array_equal(table, table.astype(np.float32).astype(np.float64))      # float32 values, widened
        h32 = want.astype(np.float32).astype(np.float64)
        err = np.abs(table - h32)
        assert np.all(err <= np.spacing(np.abs(h32)) + 2.0 ** -44), (kw, float(err.max()))
        assert np.count_nonzero(err) <= 0.01 * err.size + 2, (kw, int(np.count_nonzero(err)))      # (straddling is rare)
    # the values of the ratio and the width at the defaults
    up, down = ratio(sr, out)
    c = 0.99 * min(1.0, up / down)
    assert eng.resampleKernel(sr, out)[0].shape == (up, 2 * math.ceil(6 / c))
    if (sr, out) == (22050, 16000):
        assert (up, down) == (320, 441) and eng.resampleKernel(sr, out, **FILTERS[3])[0].size == 57600


def test_the_filter_is_a_resampler():
    """Properties of the definition (float64, from the library's table): the passband gain at 1 kHz and the rejection at 1.3 times the
    new Nyquist frequency, over every phase."""
    import nvspeechplayer_amd as eng
    table, up, down = eng.resampleKernel(22050, 16000)
    passband = np.abs(gains(table, up, 1000.0, 22050) - 1).max()
    alias = np.abs(gains(table, up, 10400.0, 22050)).max()
    print("default filter: passband %.2e, aliasing %.2e" % (passband, alias))
    assert passband < 1e-3 and alias < 1e-2
    table, up, down = eng.resampleKernel(22050, 16000, zeros=16, window="kaiser", beta=8.6)
    passband = np.abs(gains(table, up, 1000.0, 22050) - 1).max()
    alias = np.abs(gains(table, up, 10400.0, 22050)).max()
    print("Kaiser, zeros 16: passband %.2e, aliasing %.2e" % (passband, alias))
    assert passband < 1e-4 and alias < 1e-4


@pytest.mark.parametrize("sr,out", PAIRS)
def test_the_statement_against_numpy_float64(sr, out):
    """pcmResample in float32 within gamma_K sum |x| |h| of the float64 sum of the same float32 operands, K = taps; lengths
    0, 1, 2, 3, down, down + 1 and 3 down + 37 of every signal; the lengths are ceil(Lin up / down)."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer
    up, down = ratio(sr, out)
    rng = np.random.default_rng(sr + out)
    worst = 0.0
    for kw in FILTERS:
        table = eng.resampleKernel(sr, out, **kw)[0]
        for name, full in signals(2 * down, rng).items():
            for L in (0, 1, 2, 3, down, down + 1, 3 * down + 37):
                pcm = full[:L]
                got = eng.pcmResample(pcm, sr, out, **kw)
                want, mag = reference(pcm, table, up, down)
                assert got.dtype == np.float32 and len(got) == -(-L * up // down) == speechPlayer.resampledLength(L, sr, out), (kw, name, L)
                err = np.abs(got.astype(np.float64) - want)
                lim = gamma(table.shape[1]) * mag
                assert np.all(err <= lim), (kw, name, L, float((err / np.maximum(lim, 1e-300)).max()))
                if len(got):
                    worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
    print("%d -> %d: largest error over the bound: %.3f" % (sr, out, worst))
    assert not eng.pcmResample(np.zeros(3 * down, np.int16), sr, out).view(np.uint32).any()      # silence is +0 on its bits


def test_a_sine_pins_the_time_origin():
    """A 1 kHz sine of amplitude 0.5, rounded to int16, from 22 050 to 16 000 Hz: away from the first and last Z source samples output m
    is 0.5 sin(2 pi 1000 m / 16000) within 0.5 max |G_p - 1| (the filter's gain error) + 0.5 / 32767 max sum |h| (the rounding to
    int16) + (gamma_K + u) 0.5 max sum |h| (the float32 sum, and the rounding of x)."""
    import nvspeechplayer_amd as eng
    sr, out = 22050, 16000
    for kw in (FILTERS[0], FILTERS[2]):
        table, up, down = eng.resampleKernel(sr, out, **kw)
        taps = table.shape[1]
        Z = taps // 2
        L = 4 * down + 3 * taps
        pcm = np.rint(0.5 * 32767 * np.sin(2 * np.pi * 1000.0 * np.arange(L) / sr)).astype(np.int16)
        got = eng.pcmResample(pcm, sr, out, **kw).astype(np.float64)
        m = np.arange(len(got))
        n0 = m * down // up
        inner = (n0 - Z + 1 >= Z) & (n0 + Z <= L - 1 - Z)
        assert inner.sum() > 2 * up
        sums = np.abs(table).sum(axis=1).max()
        lim = 0.5 * np.abs(gains(table, up, 1000.0, sr) - 1).max() + 0.5 / 32767 * sums + (gamma(taps) + U) * 0.5 * sums
        err = np.abs(got - 0.5 * np.sin(2 * np.pi * 1000.0 * m / out))[inner]
        print("%s: largest error %.3e of %.3e" % (kw, err.max(), lim))
        assert np.all(err <= lim), (kw, float(err.max()), lim)


def test_format_0_is_the_stated_conversion():
    """int16: one float32 product by 32767, clipped to 32767 and -32768, rounded to nearest even -- of format 1's values, value for value;
    full-scale noise makes both clips occur."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(9)
    noise = rng.choice(np.array([-32768, 32767], np.int16), 4000)
    quiet = rng.integers(-3, 4, 4000).astype(np.int16)
    for sr, out in PAIRS[:5]:
        for kw in (FILTERS[0], FILTERS[2]):
            for name, pcm in (("noise", noise), ("quiet", quiet), ("random", signals(1000, rng)["random"])):
                y = eng.pcmResample(pcm, sr, out, **kw)
                q = eng.pcmResample(pcm, sr, out, dtype=np.int16, **kw)
                assert q.dtype == np.int16 and np.array_equal(q, to_int16(y)), (sr, out, kw, name)
                if name == "noise":
                    assert np.abs(y).max() > 1 and (q == 32767).any() and (q == -32768).any()


def test_equal_rates_and_lengths():
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer
    rng = np.random.default_rng(10)
    pcm = rng.integers(-32768, 32768, 1000).astype(np.int16)
    for rate in (22050, 16000, 1):
        assert np.array_equal(eng.pcmResample(pcm, rate, rate, dtype=np.int16), pcm)
        assert np.array_equal(eng.pcmResample(pcm, rate, rate).view(np.uint32), (pcm.astype(np.float32) / np.float32(32767.0)).view(np.uint32))
        assert len(eng.pcmResample(pcm[:0], rate, rate)) == 0
    for sr, out in PAIRS + [(22050, 8000), (8000, 48000), (48000, 8000)]:
        up, down = ratio(sr, out)
        for L in (0, 1, 2, down - 1, down, down + 1, 999):
            want = -(-L * up // down)
            assert speechPlayer.resampledLength(L, sr, out) == want and len(eng.pcmResample(pcm[:L], sr, out)) == want, (sr, out, L)
    assert speechPlayer.resampledLength(1 << 40, 2, 3) == 3 * (1 << 39) and speechPlayer.resampledLength((1 << 40) + 1, 3, 2) == -(-((1 << 41) + 2) // 3) and speechPlayer.resampledLength(0, 22050, 16000) == 0


REFUSED = dict(
    src_zero=dict(src=0), src_negative=dict(src=-22050), dst_zero=dict(dst=0), dst_negative=dict(dst=-1),
    zeros_zero=dict(zeros=0), zeros_negative=dict(zeros=-6),
    rolloff_zero=dict(rolloff=0.0), rolloff_negative=dict(rolloff=-0.5), rolloff_above_one=dict(rolloff=1.0000001), rolloff_nan=dict(rolloff=float("nan")),
    rolloff_inf=dict(rolloff=float("inf")), window_2=dict(window=2), window_negative=dict(window=-1),
    beta_negative=dict(window=1, beta=-1.0), beta_nan=dict(window=1, beta=float("nan")), beta_inf=dict(window=1, beta=float("inf")),
    up_4097=dict(src=4096, dst=4097), up_22051=dict(dst=22051), taps_1026=dict(zeros=372), taps_ratio=dict(src=48000, dst=50, zeros=1),
    table=dict(src=4096, dst=4095, zeros=128, rolloff=1.0))


def test_every_refusal_of_the_c_entry_points():
    from nvspeechplayer_amd import _native
    L = _native.load()
    pcm = np.arange(200, dtype=np.int16)
    out = np.full(400, -7.0, np.float32)
    table = np.full(1 << 20, -7.0)
    three = [ctypes.c_int(-7) for _ in range(3)]

    def resample(src=22050, dst=16000, zeros=6, rolloff=0.99, window=0, beta=0.0, pcm=pcm, length=200, fmt=1, out=out, capacity=400):
        p = lambda a: None if a is None else a.ctypes.data
        return L.speechPlayer_pcmResample(p(pcm), length, src, dst, zeros, rolloff, window, beta, fmt, p(out), capacity)

    def kernel(src=22050, dst=16000, zeros=6, rolloff=0.99, window=0, beta=0.0, capacity=1 << 20):
        return L.speechPlayer_resampleKernel(src, dst, zeros, rolloff, window, beta, ctypes.byref(three[0]), ctypes.byref(three[1]), ctypes.byref(three[2]),
                                             table.ctypes.data, capacity)

    for name, kw in REFUSED.items():
        for what, fn in ((b"pcmResample", resample), (b"resampleKernel", kernel)):
            assert fn(**kw) == -1, (name, what)
            assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and what in L.speechPlayer_lastError(), (name, what)
        assert np.all(out == -7.0) and np.all(table == -7.0) and all(v.value == -7 for v in three), name
    for name, kw in dict(length_negative=dict(length=-1), no_pcm=dict(pcm=None), format_2=dict(fmt=2), format_negative=dict(fmt=-1),
                         capacity_short=dict(capacity=145)).items():
        assert resample(**kw) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"pcmResample" in L.speechPlayer_lastError(), name
        assert np.all(out == -7.0), name
    assert kernel(capacity=320 * 18 - 1) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and np.all(table == -7.0)
    for bad in ((-1, 22050, 16000), (10, 0, 16000), (10, 22050, 0), (10, -5, 16000)):
        assert L.speechPlayer_resampledLength(*bad) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, bad
    # sizing, nothing to compute, and the entry points are as usable as before
    assert resample(out=None, capacity=0) == 146 and L.speechPlayer_lastErrorCode() == 0
    assert resample(pcm=None, length=0, out=None) == 0 and resample(pcm=None, length=0) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert L.speechPlayer_resampleKernel(22050, 16000, 6, 0.99, 0, 0.0, None, None, None, None, 0) == 320 * 18
    assert resample(capacity=146) == 146 and np.all(out[:146] != -7.0) and np.all(out[146:] == -7.0)
    assert resample(zeros=367) == 146 and resample(src=4096, dst=4095, zeros=127, rolloff=1.0, capacity=400) == 200      # the largest the limits admit
    assert kernel() == 320 * 18 and [v.value for v in three] == [320, 441, 18] and np.all(table[320 * 18:] == -7.0)
    assert kernel(window=0, beta=float("nan")) == 320 * 18      # Hann does not look at beta


def test_resample_request_checks():
    import torch
    from nvspeechplayer_amd.speechPlayer import check_resample_request
    ok = dict(srcRate=22050, dstRate=16000, zeros=6, rolloff=0.99, window="hann", beta=None, dtype=None)

    def check(**kw):
        a = dict(ok)
        a.update(kw)
        return check_resample_request(**a)

    assert check() == (22050, 16000, 6, 0.99, 0, 0.0, 1, 320, 441, 18)
    assert check(window="kaiser") == (22050, 16000, 6, 0.99, 1, 8.6, 1, 320, 441, 18)
    assert check(dstRate=np.int64(44100), zeros=np.int32(2), rolloff=1, window=1, beta=5, dtype=torch.int16) == (22050, 44100, 2, 1.0, 1, 5.0, 0, 2, 1, 4)
    assert check(dtype=np.int16)[6] == 0 and check(dtype=np.float32)[6] == 1 and check(dtype=torch.float32)[6] == 1
    assert check(beta=float("nan"))[5] == 0.0      # Hann does not look at beta
    words = dict(src="srcRate", dst="dstRate", window="window")
    for name, kw in REFUSED.items():
        kw = {words.get(k, k): v for k, v in kw.items()}
        with pytest.raises(ValueError):
            check(**kw)
            pytest.fail(name)
    for name, kw in dict(window_name=dict(window="blackman"), window_bool=dict(window=True), zeros_huge=dict(zeros=1 << 40)).items():
        with pytest.raises(ValueError):
            check(**kw)
            pytest.fail(name)
    for kw in (dict(dtype=torch.float64), dict(dtype=torch.int32), dict(dtype=np.float64), dict(dtype="pcm"), dict(zeros=6.0), dict(dstRate=16000.0),
               dict(srcRate=True)):
        with pytest.raises(TypeError):
            check(**kw)
    import nvspeechplayer_amd as eng
    for bad in (np.zeros(10, np.float32), np.zeros((2, 10), np.int16), [1, 2, 3]):
        with pytest.raises(TypeError):
            eng.pcmResample(bad, 22050, 16000)
    with pytest.raises(ValueError):
        eng.pcmResample(np.zeros(10, np.int16), 22050, 22051)
    with pytest.raises(ValueError):
        eng.resampleKernel(22050, 16000, zeros=0)


def test_the_statement_under_sanitizers(tmp_path):
    """csrc/klatt_resample.h (the plan, the statement, the int16 conversion, the kernel's span and transposed table) in a program of its
    own, tests/native/check_resample.cpp, against a brute-force double loop under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "check_resample")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_resample.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out
