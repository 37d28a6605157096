"""The convolution export on the host (include/speechPlayer_batch.h: speechPlayer_pcmConvolve; nvspeechplayer_amd.pcmConvolve,
check_convolve_request; csrc/klatt_convolve.h): the product's CPU statement against numpy's float64 convolution within the inner-product
bound, the cases the definition makes exact -- bit for bit --, the lemma about terms whose product is zero, lengths, the int16
conversion and every refusal.  `decaying`, `reference` and `gamma` are the comparands tests/test_gpu_convolve.py shares.  No GPU."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
U = 2.0 ** -24


def gamma(taps):
    """gamma_K of Higham, Accuracy and Stability of Numerical Algorithms, chapter 3: K roundings in a chain."""
    return taps * U / (1 - taps * U)


def decaying(K, seed):
    """A seeded, exponentially decaying response of K float32 taps: noise under exp(-5 k / K), 0.5 at its largest."""
    rng = np.random.default_rng(1000 + seed)
    return (0.5 * rng.uniform(-1, 1, K) * np.exp(-5.0 * np.arange(K) / K)).astype(np.float32)


def x_of(pcm):
    """The definition's input: (float)s / 32767.0f."""
    return np.asarray(pcm).astype(np.float32) / np.float32(32767.0)


def reference(pcm, h, tail=True):
    """numpy's float64 convolution of the float32 operands (their products are exact in binary64): -> (y [Lout], conv(|x|, |h|))."""
    x, h = x_of(pcm).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
    if len(x) == 0:
        return np.zeros(0), np.zeros(0)
    y, mag = np.convolve(x, h), np.convolve(np.abs(x), np.abs(h))
    return (y, mag) if tail else (y[:len(x)], mag[:len(x)])


def to_int16(y):
    """Format 0 of float32 values, as the header states it."""
    q = y.astype(np.float32) * np.float32(32767.0)
    return np.where(q >= 32767, 32767, np.where(q <= -32768, -32768, np.rint(q))).astype(np.int16)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def constants():
    from nvspeechplayer_amd import speechPlayer as sp
    return sp.CONVOLVE_TILE, sp.CONVOLVE_BLOCK


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs in (("speechPlayer_batch_exportConvolved", 12), ("speechPlayer_pcmConvolve", 8)):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and len(fn.argtypes) == nargs, name
    section = header.split("A batch's PCM convolved with impulse responses")[1].split("speechPlayer_batch_exportConvolved(")[0]
    for word in ("fmaf", "Lemma", "+ 0.0f", "MODE_FAST", "live handles", "NodePlayer", "wet/dry", "FFT or MFMA", "spectrogram or resampling"):
        assert word in section, word
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_convolve.h")).read()
    assert '#include "klatt_resample.h"' in shared and "__builtin_fmaf" in shared
    values = {}
    for name, pattern in (("kConvolveTile", r"constexpr int kConvolveTile = (\d+);"), ("kConvolveBlock", r"constexpr int kConvolveBlock = (\d+);"),
                          ("kConvolveMaxTaps", r"constexpr int kConvolveMaxTaps = (\d+);"),
                          ("kConvolveMaxTable", r"constexpr long long kConvolveMaxTable = 1ll << (\d+);")):
        values[name] = int(re.search(pattern, shared).group(1))
    values["kConvolveMaxTable"] = 1 << values["kConvolveMaxTable"]
    assert (speechPlayer.CONVOLVE_TILE, speechPlayer.CONVOLVE_BLOCK, speechPlayer.CONVOLVE_MAX_TAPS, speechPlayer.CONVOLVE_MAX_TABLE) == \
        (values["kConvolveTile"], values["kConvolveBlock"], values["kConvolveMaxTaps"], values["kConvolveMaxTable"])
    assert "kConvolveTile = %d" % values["kConvolveTile"] in header and "kConvolveBlock = %d" % values["kConvolveBlock"] in header
    assert "kConvolveMaxTaps = %d" % values["kConvolveMaxTaps"] in header and "kConvolveMaxTable = 2^20" in header and values["kConvolveMaxTable"] == 2 ** 20
    assert callable(speechPlayer.BatchPlayer.convolvedTensor) and callable(speechPlayer.check_convolve_request)
    assert nvspeechplayer_amd.pcmConvolve is speechPlayer.pcmConvolve


def test_the_statement_against_numpy_float64():
    """pcmConvolve in float32 within gamma_K conv(|x|, |h|) of numpy's float64 convolution, on seeded noise at full scale, both tails."""
    import nvspeechplayer_amd as eng
    T, B = constants()
    rng = np.random.default_rng(77)
    for i, K in enumerate((1, 2, 5, B - 1, B, B + 1, 2 * B + 3)):
        h = decaying(K, i)
        pcm = rng.integers(-32768, 32768, 1500 if K < 100 else 700).astype(np.int16)
        worst = 0.0
        for tail in (True, False):
            got = eng.pcmConvolve(pcm, h, tail=tail)
            want, mag = reference(pcm, h, tail)
            assert got.dtype == np.float32 and got.shape == want.shape == ((len(pcm) + K - 1,) if tail else (len(pcm),))
            err, lim = np.abs(got.astype(np.float64) - want), gamma(K) * mag
            assert np.all(err <= lim), (K, tail, float((err / np.maximum(lim, 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        print("K %d: largest error over the bound: %.3f" % (K, worst))


def test_identity_is_the_pcm_for_every_sample_value():
    """h = [1.0]: the float32 PCM of res_input and, in int16, the PCM itself: rint((float)s / 32767 * 32767) == s for all 65 536 values."""
    import nvspeechplayer_amd as eng
    pcm = np.arange(-32768, 32768).astype(np.int16)
    one = np.ones(1, np.float32)
    for tail in (True, False):
        assert np.array_equal(bits(eng.pcmConvolve(pcm, one, tail=tail)), bits(x_of(pcm)))
        assert np.array_equal(eng.pcmConvolve(pcm, one, tail=tail, dtype=np.int16), pcm)


def test_delayed_scaled_impulses_are_exact():
    """h = [0] * d + [2^e] returns 2^e x[m - d], bit for bit, for d in {0, 1, B, B + 1}."""
    import nvspeechplayer_amd as eng
    T, B = constants()
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, B + 300).astype(np.int16)
    x = x_of(pcm)
    for d in (0, 1, B, B + 1):
        for e in (-3, 0, 5):
            h = np.zeros(d + 1, np.float32)
            h[d] = 2.0 ** e
            want = np.zeros(len(pcm) + d, np.float32)
            want[d:] = x * np.float32(2.0 ** e)
            assert np.array_equal(bits(eng.pcmConvolve(pcm, h)), bits(want)), (d, e)
            assert np.array_equal(bits(eng.pcmConvolve(pcm, h, tail=False)), bits(want[:len(pcm)])), (d, e)


def test_silence_is_plus_zero():
    import nvspeechplayer_amd as eng
    for K in (1, 5, 1030):
        for h in (decaying(K, 3), -np.abs(decaying(K, 4))):
            assert not bits(eng.pcmConvolve(np.zeros(40, np.int16), h)).any()
            assert not eng.pcmConvolve(np.zeros(40, np.int16), h, dtype=np.int16).any()
    # a signal that cancels exactly, and products of either sign of zero
    assert not bits(eng.pcmConvolve(np.array([5, 0, -5], np.int16), np.array([0.0, -0.0], np.float32))).any()
    assert not bits(eng.pcmConvolve(np.array([-7, -7], np.int16), np.array([1.0, -1.0], np.float32)))[1:2].any()


def subnormal_chain(pcm, h, tail):
    """The definition in exact arithmetic where every product and sum stays below 2^-126: every fmaf rounds acc + x h to the nearest
    multiple of 2^-149, ties to even."""
    x = [Fraction(float(v)) for v in x_of(pcm)]
    hh = [Fraction(float(v)) for v in h]
    unit = Fraction(1, 2 ** 149)
    out = []
    for m in range(len(x) + len(hh) - 1 if tail else len(x)):
        acc = Fraction(0)
        for k in range(len(hh)):
            if 0 <= m - k < len(x):
                q = (acc + x[m - k] * hh[k]) / unit
                f = q.numerator // q.denominator
                r = q - f
                acc = (f + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2) else 0)) * unit
                assert abs(acc) < Fraction(1, 2 ** 126)
        out.append(float(acc))
    return np.array(out, np.float64).astype(np.float32)


def test_subnormal_products_round_gradually():
    """A response scaled by 2^-130: every product is subnormal.  Where the operands make every step exact at both scales (samples 0 and
    +-32767, taps that are eighths) the result is the unscaled one times 2^-130 exactly; on noise it is the chain in exact arithmetic
    with every step rounded to the subnormal grid -- nothing is flushed to zero."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(6)
    scale = np.float32(2.0 ** -130)
    pcm = rng.choice(np.array([0, 32767, -32767], np.int16), 300)
    g = (rng.integers(-8, 9, 7) / 8.0).astype(np.float32)
    for tail in (True, False):
        plain = eng.pcmConvolve(pcm, g, tail=tail)
        small = eng.pcmConvolve(pcm, g * scale, tail=tail)
        assert plain.any() and np.array_equal(bits(small), bits(plain * scale)) and np.array_equal(small.astype(np.float64), plain.astype(np.float64) * 2.0 ** -130)
    noise = rng.integers(-32768, 32768, 200).astype(np.int16)
    h = decaying(5, 9) * scale
    assert np.all(np.abs(h) < 2.0 ** -130) and h.all()
    for tail in (True, False):
        got = eng.pcmConvolve(noise, h, tail=tail)
        assert np.count_nonzero(got) > 150 and np.array_equal(bits(got), bits(subnormal_chain(noise, h, tail))), tail


def test_the_lemma():
    """Terms whose product is zero change nothing (tail = 0): trailing zero taps, -0.0 taps, and leading zero taps with the signal
    delayed to match."""
    import nvspeechplayer_amd as eng
    T, B = constants()
    rng = np.random.default_rng(8)
    pcm = rng.integers(-32768, 32768, 900).astype(np.int16)
    pcm[100:140] = 0
    for K in (1, 5, B - 1):
        h = decaying(K, 20 + K)
        h[K // 2] = 0.0
        base = eng.pcmConvolve(pcm, h, tail=False)
        for extra in (1, 3, B + 2):
            assert np.array_equal(bits(eng.pcmConvolve(pcm, np.concatenate([h, np.zeros(extra, np.float32)]), tail=False)), bits(base)), (K, extra)
            assert np.array_equal(bits(eng.pcmConvolve(pcm, np.concatenate([h, np.full(extra, -0.0, np.float32)]), tail=False)), bits(base)), (K, extra)
        minus = h.copy()
        minus[K // 2] = -0.0
        assert np.signbit(minus[K // 2]) and np.array_equal(bits(eng.pcmConvolve(pcm, minus, tail=False)), bits(base)), K
        for d in (1, 4, B + 1):
            zeros = np.zeros(d, np.int16)
            a = eng.pcmConvolve(np.concatenate([zeros, pcm]), h, tail=False)                                   # the signal delayed
            b = eng.pcmConvolve(np.concatenate([pcm, zeros]), np.concatenate([np.zeros(d, np.float32), h]), tail=False)      # the response delayed
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a[d:]), bits(base)) and not bits(a[:d]).any(), (K, d)


def test_lengths():
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(11)
    pcm = rng.integers(-32768, 32768, 3).astype(np.int16)
    for L in (0, 1, 2, 3):
        for K in (1, 2, 4, 9):
            h = decaying(K, K)
            full = eng.pcmConvolve(pcm[:L], h)
            first = eng.pcmConvolve(pcm[:L], h, tail=False)
            assert len(full) == L + K - 1 and len(first) == L and np.array_equal(bits(first), bits(full[:L])), (L, K)
            want, mag = reference(pcm[:L], h) if L else (np.zeros(K - 1), np.zeros(K - 1))
            assert np.all(np.abs(full.astype(np.float64) - want) <= gamma(K) * mag), (L, K)
            if L == 0:
                assert not bits(full).any()


def test_format_0_is_the_stated_conversion():
    """int16: one float32 product by 32767, clipped on both sides, rounded to nearest even -- of format 1's values, value for value."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(9)
    noise = rng.choice(np.array([-32768, 32767], np.int16), 3000)
    ramp = np.arange(-3000, 3000).astype(np.int16)
    for h in (decaying(40, 1) * 8, np.array([2.0], np.float32), np.array([0.5], np.float32), np.array([-1.0], np.float32)):
        for pcm in (noise, ramp):
            for tail in (True, False):
                y = eng.pcmConvolve(pcm, h, tail=tail)
                q = eng.pcmConvolve(pcm, h, tail=tail, dtype=np.int16)
                assert q.dtype == np.int16 and np.array_equal(q, to_int16(y))
    q = eng.pcmConvolve(noise, np.array([2.0], np.float32), dtype=np.int16)
    assert (q == 32767).any() and (q == -32768).any() and set(np.unique(q)) == {-32768, 32767}
    y = eng.pcmConvolve(ramp, np.array([0.5], np.float32))
    halves = y * np.float32(32767.0)
    ties = np.flatnonzero(halves - np.floor(halves) == 0.5)
    assert len(ties) > 1000 and not (eng.pcmConvolve(ramp, np.array([0.5], np.float32), dtype=np.int16)[ties] & 1).any()      # ties go to even


REFUSED_HOST = dict(
    tail_2=dict(tail=2), tail_negative=dict(tail=-1), no_ir=dict(ir=None), taps_zero=dict(taps=0), taps_negative=dict(taps=-4), taps_65537=dict(taps=65537),
    tap_nan=dict(bad=float("nan")), tap_inf=dict(bad=float("inf")), tap_minus_inf=dict(bad=-float("inf")), tap_above_2_32=dict(bad=2.0 ** 32 * (1 + 2.0 ** -23)),
    tap_below_minus_2_32=dict(bad=-2.0 ** 33), format_2=dict(fmt=2), format_negative=dict(fmt=-1), length_negative=dict(length=-1), no_pcm=dict(pcm=None),
    capacity_short=dict(capacity=208))


def test_every_refusal_of_the_c_entry_point():
    from nvspeechplayer_amd import _native
    L = _native.load()
    pcm = np.arange(200, dtype=np.int16)
    out = np.full(70000, -7.0, np.float32)
    ir = np.full(65537, 0.25, np.float32)

    def convolve(pcm=pcm, length=200, ir=ir, taps=10, tail=1, fmt=1, out=out, capacity=70000, bad=None):
        p = lambda a: None if a is None else a.ctypes.data
        h = ir
        if bad is not None:
            h = ir.copy()
            h[7] = bad
        return L.speechPlayer_pcmConvolve(p(pcm), length, p(h), taps, tail, fmt, p(out), capacity)

    for name, kw in REFUSED_HOST.items():
        assert convolve(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"pcmConvolve" in L.speechPlayer_lastError(), name
        assert np.all(out == -7.0), name
    assert convolve(bad=float("nan")) == -1 and b"tap 7 of response 0" in L.speechPlayer_lastError()
    # sizing, nothing to compute, the limits themselves, and the entry point is as usable as before
    assert convolve(out=None, capacity=0) == 209 and convolve(out=None, capacity=0, tail=0) == 200 and L.speechPlayer_lastErrorCode() == 0
    assert convolve(pcm=None, length=0, out=None) == 9 and convolve(pcm=None, length=0, tail=0) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert convolve(capacity=209) == 209 and np.all(out[:209] != -7.0) and np.all(out[209:] == -7.0)
    assert convolve(bad=2.0 ** 32) == 209 and convolve(bad=-2.0 ** 32) == 209
    assert convolve(pcm=pcm[:2], length=2, taps=65536, tail=0) == 2 and np.all(out[2:209] != -7.0) and np.all(out[209:] == -7.0)      # the longest response
    assert convolve(pcm=pcm[:2], length=2, taps=65536, out=None) == 65537


def test_convolve_request_checks():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    check = sp.check_convolve_request
    h, start, of, tail, fmt = check(np.array([1.0, 0.5]), None, 3, True, None)
    assert h.dtype == np.float32 and list(h) == [1.0, 0.5] and start.dtype == np.int64 and list(start) == [0, 2] and of is None and (tail, fmt) == (1, 1)
    h, start, of, tail, fmt = check([np.ones(3, np.float64), torch.ones(2), [0.25]], [2, 0, 1, 2], 4, 0, torch.int16)
    assert list(start) == [0, 3, 5, 6] and of.dtype == np.int64 and list(of) == [2, 0, 1, 2] and (tail, fmt) == (0, 0) and h[5] == 0.25
    assert check([1.0, 2.0, 3.0], None, 1, False, np.int16)[1:] [0].tolist() == [0, 3]
    assert check(np.ones(sp.CONVOLVE_MAX_TAPS), None, 1, np.True_, np.float32)[4] == 1
    assert len(check([np.ones(sp.CONVOLVE_MAX_TAPS)] * 16, np.zeros(2, np.int32), 2, True, torch.float32)[0]) == sp.CONVOLVE_MAX_TABLE
    bad = np.ones(8, np.float64)
    value = dict(
        no_responses=([], None), empty_response=([np.ones(2), np.ones(0)], [0, 0]), taps_65537=(np.ones(sp.CONVOLVE_MAX_TAPS + 1), None),
        table=([np.ones(sp.CONVOLVE_MAX_TAPS)] * 16 + [np.ones(1)], [0, 0]), irOf_beyond=([bad, bad], [0, 2]), irOf_negative=([bad, bad], [-1, 0]),
        irOf_missing=([bad, bad], None), irOf_short=([bad, bad], [0]), irOf_long=(bad, [0, 0, 0]))
    for name, (irs, of) in value.items():
        with pytest.raises(ValueError):
            check(irs, of, 2, True, None)
            pytest.fail(name)
    for name, tap in dict(nan=float("nan"), inf=float("inf"), minus_inf=-float("inf"), above=2.0 ** 32 * (1 + 2.0 ** -23), below=-2.0 ** 33, float64_only=1e300).items():
        h = bad.copy()
        h[5] = tap
        with pytest.raises(ValueError, match="tap 5 of response 1"):
            check([bad, h], [0, 1], 2, True, None)
            pytest.fail(name)
    h = bad.copy()
    h[5] = -2.0 ** 32
    check([bad, h], [0, 1], 2, True, None)
    for name, t in dict(two=2, negative=-1, text="yes", none=None, real=1.0).items():
        with pytest.raises(ValueError):
            check(bad, None, 2, t, None)
            pytest.fail(name)
    for name, (irs, of, dtype) in dict(two_d=(np.ones((2, 3)), None, None), scalar=(1.0, None, None), text=(["a", "b"], None, None), complex_=(np.ones(3, np.complex64), None, None),
                                       irOf_real=([bad, bad], [0.0, 1.0], None), irOf_2d=([bad, bad], [[0, 1]], None), float64=(bad, None, torch.float64),
                                       int32=(bad, None, np.int32), name=(bad, None, "pcm")).items():
        with pytest.raises(TypeError):
            check(irs, of, 2, True, dtype)
            pytest.fail(name)
    import nvspeechplayer_amd as eng
    for pcm in (np.zeros(10, np.float32), np.zeros((2, 10), np.int16), [1, 2, 3]):
        with pytest.raises(TypeError):
            eng.pcmConvolve(pcm, bad)
    with pytest.raises(ValueError):
        eng.pcmConvolve(np.zeros(10, np.int16), [bad, bad])


def test_the_statement_under_sanitizers(tmp_path):
    """csrc/klatt_convolve.h (the plan, the statement, the kernel's tile / block / skip arithmetic) in a program of its own,
    tests/native/check_convolve.cpp, against brute force under AddressSanitizer + UBSan.  Nothing loaded into python is run under one."""
    exe = str(tmp_path / "check_convolve")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_convolve.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out
