"""The filter export on the host (include/speechPlayer_batch.h: speechPlayer_pcmFilter, speechPlayer_signalFilter;
nvspeechplayer_amd.pcmFilter, signalFilter, check_filter_request, biquad, preEmphasis, dcBlock, resonatorSections; csrc/klatt_filter.h):
the product's CPU statement against a transcription of the definition's five lines -- bit for bit --, against a plain binary64
recursion within a bound derived per filter, the lemma about identity sections, subnormal results, the designers, every refusal, and
the packing of rows into wavefronts with a model of the kernel (tests/native/check_filter_pack.cpp).  `stable`, `seven` and
`impulse_rows` are what tests/test_gpu_filter.py shares.  No GPU."""
import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.test_convolve_host import bits, to_int16, x_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
U = 2.0 ** -24
IDENTITY = np.array([1, 0, 0, 0, 0], np.float32)
# scipy.signal.butter(4, [300, 3400], "bandpass", fs=22050, output="sos"): the telephone band, four sections
TELEPHONE = np.array([
    [0.015031869558932728, 0.030063739117865456, 0.015031869558932728, 1.0, -0.790740694160057, 0.1990626472143866],
    [1.0, 2.0, 1.0, 1.0, -0.9114585623463567, 0.5756179539149701],
    [1.0, -2.0, 1.0, 1.0, -1.829051960405075, 0.8381042282374366],
    [1.0, -2.0, 1.0, 1.0, -1.9368246537081515, 0.9441864241806792]])


def stable(K, seed):
    """K seeded float32 sections b0 b1 b2 a1 a2 with poles at radius 0.3 .. 0.93 and any angle, each scaled to pass white noise at its
    power (a root-mean-square gain of 1), so that a cascade of sixteen neither dies away nor grows."""
    rng = np.random.default_rng(4000 + seed)
    out = np.zeros((K, 5))
    z = np.exp(-1j * np.linspace(0, np.pi, 512))
    for j in range(K):
        r, th = rng.uniform(0.3, 0.93), rng.uniform(0.05, 0.95) * np.pi
        b = np.array([1.0, rng.uniform(-1, 1), rng.uniform(-1, 1)])
        a1, a2 = -2 * r * np.cos(th), r * r
        gain = np.sqrt(np.mean(np.abs((b[0] + b[1] * z + b[2] * z * z) / (1 + a1 * z + a2 * z * z)) ** 2))
        out[j] = [*(b / gain), a1, a2]
    return out.astype(np.float32)


def seven():
    """Seven seeded filters of 1, 2, 3, 5, 8, 9 and 16 sections: every bucket, and rows the kernel pads with identity sections."""
    return [stable(K, i) for i, K in enumerate((1, 2, 3, 5, 8, 9, 16))]


def fmaf(a, b, c):
    """fmaf of three binary32 values held in Python floats, through binary64: the product is exact there; the sum is rounded to odd
    (TwoSum gives the error, an inexact even result moves to its odd neighbour on the error's side), after which the rounding to
    binary32 -- gradual underflow included -- is the single correct one (53 >= 2 * 24 + 2)."""
    p = a * b
    s = p + c
    if math.isfinite(s):
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        if err != 0.0 and not struct.unpack("<q", struct.pack("<d", s))[0] & 1:
            s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return float(np.float32(s))


def transcribed(x, sections, tail=0):
    """The definition, line for line: x float32 [L], sections float32 [K, 5] -> float32 [L + tail]."""
    sec = [[float(v) for v in s] for s in np.asarray(sections, np.float32)]
    s1, s2 = [0.0] * len(sec), [0.0] * len(sec)
    out = np.zeros(len(x) + tail, np.float32)
    for n in range(len(out)):
        v = float(x[n]) if n < len(x) else 0.0
        for j, (b0, b1, b2, a1, a2) in enumerate(sec):
            na1, na2 = -a1, -a2
            y = fmaf(b0, v, s1[j])
            t = fmaf(b1, v, s2[j])
            s1[j] = fmaf(na1, y, t)
            w = float(np.float32(b2 * v))      # (the product of two binary32 values is exact in binary64: one rounding)
            s2[j] = fmaf(na2, y, w)
            v = y
        out[n] = np.float32(v) + np.float32(0.0)
    return out


def recursion64(x, sos):
    """The same recursion in plain binary64 on binary64 copies of the float32 coefficients: -> (y, m) with m[j] the largest
    |y| + |t| + |s1| + |v| + |s2| section j saw."""
    v = np.asarray(x, np.float64).copy()
    m = []
    for b0, b1, b2, a1, a2 in np.asarray(sos, np.float32).astype(np.float64):
        s1 = s2 = 0.0
        most = 0.0
        y_all = np.zeros(len(v))
        for n, xn in enumerate(v):
            y = b0 * xn + s1
            t = b1 * xn + s2
            s1 = t - a1 * y
            w = b2 * xn
            s2 = w - a2 * y
            most = max(most, abs(y) + abs(t) + abs(s1) + abs(w) + abs(s2))
            y_all[n] = y
        v = y_all
        m.append(most)
    return v, m


def l1(b, a, n=6000):
    """The l1 norm of the impulse response of b(z) / a(z), second order, from n binary64 samples (poles within radius 0.98 have
    decayed by 1e-50 there)."""
    d = np.zeros(n)
    d[0] = 1.0
    return float(np.abs(recursion64(d, [[b[0], b[1], b[2], a[0], a[1]]])[0]).sum())


def five(sections):
    """float32 [K, 5] of [K, 5] or sos [K, 6], as the binding makes it."""
    from nvspeechplayer_amd import speechPlayer as sp
    return sp.check_filter_request(sections, None, 1, 0, None)[0].reshape(-1, 5)


def impulse_rows():
    """The two impulse rows of the subnormal tests: (int16 samples, sections) for the halving section over 400 samples and for the
    resonator at 300 Hz, 400 Hz wide, at 22 050 Hz over 2000."""
    from nvspeechplayer_amd import speechPlayer as sp
    a = np.zeros(400, np.int16)
    b = np.zeros(2000, np.int16)
    a[0] = b[0] = 32767      # x = 1.0f exactly
    return [(a, np.array([[1, 0, 0, -0.5, 0]], np.float32)), (b, five(sp.resonatorSections(300, 400, 22050)))]


def subnormal(y):
    return (y != 0) & (np.abs(y) < np.float32(2.0 ** -126))


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer as sp
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs in (("speechPlayer_pcmFilter", 8), ("speechPlayer_signalFilter", 9), ("speechPlayer_batch_exportFiltered", 12),
                        ("speechPlayer_batch_exportFilteredOf", 13)):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and len(fn.argtypes) == nargs, name
    section = header.split("through cascades of second-order recursive")[1].split("speechPlayer_batch_exportFiltered(")[0]
    for word in ("fmaf(b0,  x, s1)", "fmaf(na2, y, v)", "Lemma", "+ 0.0f", "overflows", "live handles", "NodePlayer", "zero-phase", "initial conditions", "scan",
                 "a2 < 1 and |a1| < 1 + a2"):
        assert word in section, word
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_filter.h")).read()
    assert '#include "klatt_resample.h"' in shared and "__builtin_fmaf" in shared and "Out of scope" in shared and "lemma" in shared
    value = lambda pattern: int(re.search(pattern, shared).group(1))
    assert sp.FILTER_MAX_SECTIONS == value(r"constexpr int kFilterMaxSections = (\d+);") == 16
    assert sp.FILTER_TILE == value(r"constexpr int kFilterTile = (\d+);") and sp.FILTER_TILE in (32, 64)
    assert sp.FILTER_MAX_TABLE == 1 << value(r"constexpr long long kFilterMaxTable = 1ll << (\d+);") == 1 << 16
    assert sp.FILTER_MAX_TAIL == 1 << value(r"constexpr long long kFilterMaxTail = 1ll << (\d+);") == 1 << 20
    assert "kFilterMaxSections = 16" in header and "kFilterTile = %d" % sp.FILTER_TILE in header
    assert callable(sp.BatchPlayer.filteredTensor)
    for name in ("pcmFilter", "signalFilter", "biquad", "preEmphasis", "dcBlock", "resonatorSections"):
        assert getattr(nvspeechplayer_amd, name) is getattr(sp, name), name


@pytest.mark.parametrize("K", [1, 3, 16])
def test_the_statement_is_the_transcription(K):
    """Seeded int16 rows of 0, 1, 2 and 257 samples through K sections: float32 bit for bit, int16 the stated conversion; with a tail."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(50 + K)
    sec = stable(K, 10 + K)
    for L in (0, 1, 2, 257):
        pcm = rng.integers(-32768, 32768, L).astype(np.int16)
        for tail in (0, 5):
            want = transcribed(x_of(pcm), sec, tail)
            got = eng.pcmFilter(pcm, sec, tail=tail)
            assert got.dtype == np.float32 and got.shape == (L + tail,)
            assert np.array_equal(bits(got), bits(want)), (K, L, tail)
            assert np.array_equal(eng.pcmFilter(pcm, sec, tail=tail, dtype=np.int16), to_int16(want)), (K, L, tail)
            assert np.array_equal(bits(eng.signalFilter(pcm, sec, tail=tail)), bits(want)), (K, L, tail)
            assert np.array_equal(bits(eng.signalFilter(x_of(pcm), sec, tail=tail)), bits(want)), (K, L, tail)
        if L == 257:
            assert np.abs(want).max() > 1e-3      # (the cascade passes the signal: nothing here is a row of zeros)
    # scipy's layout: divided by a0 in binary64, rounded to float32 once
    sos = np.concatenate([sec[:, :3].astype(np.float64) * 1.7, np.full((K, 1), 1.7), sec[:, 3:].astype(np.float64) * 1.7], axis=1)
    pcm = rng.integers(-32768, 32768, 40).astype(np.int16)
    again = (np.concatenate([sos[:, :3], sos[:, 4:]], axis=1) / sos[:, 3:4]).astype(np.float32)
    assert np.array_equal(bits(eng.pcmFilter(pcm, sos)), bits(transcribed(x_of(pcm), again)))


def test_independent_of_the_shared_code():
    """The statement against a plain binary64 recursion of the same float32-rounded coefficients, on 6000 full-scale random samples.
    The bound is derived per filter: E <- E ||H_j||_1 + u m_j ||1 / A_j||_1 over the sections, u = 2^-24 -- the error that enters a
    section is carried through its impulse response, and its own five roundings, each at most u times the magnitude of the value
    rounded, reach the output through its recursive part.  Only filters whose bound is below 1e-3 of the output's peak are taken, so
    the check cannot be vacuous.  Measured: pre-emphasis 0.97 error 8.9e-08 over bound 2.3e-07; the fourth-order Butterworth
    300 - 3400 Hz band-pass (four sections) error 2.4e-06 over bound 1.7e-04 (profiles/filter_host_bounds.txt)."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(91)
    pcm = rng.integers(-32768, 32768, 6000).astype(np.int16)
    for name, sos in (("preEmphasis(0.97)", eng.preEmphasis(0.97)), ("telephone band, 4 sections", TELEPHONE)):
        sec = five(sos)
        want, m = recursion64(x_of(pcm), sec)
        bound = 0.0
        for (b0, b1, b2, a1, a2), mj in zip(sec.astype(np.float64), m):
            bound = bound * l1([b0, b1, b2], [a1, a2]) + U * mj * l1([1.0, 0.0, 0.0], [a1, a2])
        peak = np.abs(want).max()
        err = np.abs(eng.pcmFilter(pcm, sos).astype(np.float64) - want).max()
        print("%s: error %.3g, bound %.3g (%.3f of it), peak %.3g" % (name, err, bound, err / bound, peak))
        assert bound < 1e-3 * peak, (name, bound, peak)
        assert err <= bound, (name, err, bound)


def test_the_lemma():
    """A filter and the same filter with identity sections in front, in the middle and behind give the same bits, on inputs that
    contain zeros of both signs and runs of zeros."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(17)
    x = rng.uniform(-1, 1, 700).astype(np.float32)
    x[100:140] = 0.0
    x[200:230] = -0.0
    x[300:340:2] = -0.0
    x[301:340:2] = 0.0
    x[0] = -0.0
    assert np.signbit(x[210]) and x[210] == 0
    pcm = rng.integers(-32768, 32768, 700).astype(np.int16)
    pcm[50:90] = 0
    for K in (1, 2, 5):
        sec = stable(K, 30 + K)
        forms = [np.concatenate([IDENTITY[None]] * 2 + [sec]), np.concatenate([sec, IDENTITY[None]]),
                 np.concatenate([sec[:(K + 1) // 2], IDENTITY[None], sec[(K + 1) // 2:]]),
                 np.concatenate([IDENTITY[None], sec[:1], IDENTITY[None], sec[1:]] + [IDENTITY[None]] * (16 - K - 2))]
        for tail in (0, 9):
            base, base16 = eng.signalFilter(x, sec, tail=tail), eng.pcmFilter(pcm, sec, tail=tail)
            assert base.any() and base16.any()
            for i, f in enumerate(forms):
                assert np.array_equal(bits(eng.signalFilter(x, f, tail=tail)), bits(base)), (K, tail, i)
                assert np.array_equal(bits(eng.pcmFilter(pcm, f, tail=tail)), bits(base16)), (K, tail, i)
    # silence is +0 whatever the filter, and the identity alone returns the samples with every zero +0
    assert not bits(eng.signalFilter(np.full(50, -0.0, np.float32), stable(3, 1), tail=4)).any()
    assert np.array_equal(bits(eng.signalFilter(x, IDENTITY[None])), bits(x + np.float32(0.0)))


def test_subnormal_results_are_kept():
    """An impulse through y[n] = x[n] + 0.5 y[n-1] halves down through the subnormal range to +0; an impulse through the resonator at
    300 Hz ends in a subnormal limit cycle and never reaches zero: its last 8 values' bits are the transcription's."""
    import nvspeechplayer_amd as eng
    (a, half), (b, res) = impulse_rows()
    y = eng.pcmFilter(a, half)
    assert np.array_equal(bits(y), bits(transcribed(x_of(a), half)))
    assert np.array_equal(y[:150].astype(np.float64), 0.5 ** np.arange(150))
    assert np.count_nonzero(subnormal(y)) == 23 and not bits(y[150:]).any() and y[149] == 2.0 ** -149
    y = eng.pcmFilter(b, res)
    want = transcribed(x_of(b), res)
    assert np.array_equal(bits(y), bits(want))
    assert np.all(subnormal(y[-200:])), "the limit cycle"
    assert [int(v) for v in bits(y[-8:])] == [int(v) for v in bits(want[-8:])]
    print("the limit cycle's last 8 values: %s" % " ".join("%08x" % v for v in bits(y[-8:])))


def test_designers():
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer as sp

    def response(sos, f, rate):
        z = np.exp(-2j * np.pi * np.asarray(f, np.float64) / rate)
        h = np.ones(len(z), complex)
        for b0, b1, b2, a0, a1, a2 in sos:
            h *= (b0 + b1 * z + b2 * z * z) / (a0 + a1 * z + a2 * z * z)
        return h

    rate = 22050
    for kind in sp.BIQUAD_KINDS:
        s = eng.biquad(kind, rate, 1000.0, q=2.0, gainDb=6.0)
        assert s.shape == (1, 6) and s.dtype == np.float64 and s[0, 3] == 1.0
        assert s[0, 5] < 1 and abs(s[0, 4]) < 1 + s[0, 5], kind      # stable
    db = lambda h: 20 * np.log10(np.maximum(np.abs(h), 1e-300))
    at = lambda sos, f: float(db(response(sos, [f], rate))[0])
    assert abs(at(eng.biquad("lowpass", rate, 1000.0), 1000.0) + 3.0103) < 1e-3 and abs(at(eng.biquad("lowpass", rate, 1000.0), 1.0)) < 1e-3
    assert abs(at(eng.biquad("highpass", rate, 80.0), 80.0) + 3.0103) < 1e-3 and abs(at(eng.biquad("highpass", rate, 80.0), 11000.0)) < 1e-3
    assert abs(at(eng.biquad("peaking", rate, 2000.0, q=1.5, gainDb=-7.0), 2000.0) + 7.0) < 1e-9
    assert abs(at(eng.biquad("bandpass", rate, 1500.0, q=3.0), 1500.0)) < 1e-9 and at(eng.biquad("notch", rate, 1500.0, q=3.0), 1500.0) < -200
    assert abs(at(eng.biquad("lowshelf", rate, 500.0, gainDb=5.0), 1.0) - 5.0) < 1e-3 and abs(at(eng.biquad("lowshelf", rate, 500.0, gainDb=5.0), 11000.0)) < 1e-3
    assert abs(at(eng.biquad("highshelf", rate, 3000.0, gainDb=-4.0), 11020.0) + 4.0) < 1e-3 and abs(at(eng.biquad("highshelf", rate, 3000.0, gainDb=-4.0), 1.0)) < 1e-3
    assert np.array_equal(eng.preEmphasis(0.9), [[1, -0.9, 0, 1, 0, 0]]) and np.array_equal(eng.dcBlock(0.99), [[1, -1, 0, 1, -0.99, 0]])
    for bad in (dict(kind="lowpass", f0=0.0), dict(kind="lowpass", f0=rate / 2), dict(kind="peaking", f0=100.0, q=0.0), dict(kind="peaking", f0=100.0, gainDb=float("nan"))):
        with pytest.raises(ValueError):
            eng.biquad(bad.pop("kind"), rate, **bad)
    with pytest.raises(KeyError):
        eng.biquad("allpass", rate, 100.0)
    # the synthesiser's resonator: frameResponse's parallel branch with p1 alone at amplitude 1 is (H - 1) / 2
    freqs = np.array([0.0, 250.0, 300.0, 1234.5, 11025.0])
    for f, bw, sr in ((300.0, 400.0, 22050), (2500.0, 90.0, 16000)):
        frame = np.zeros(len(sp.FRAME_FIELDS))
        frame[sp.FRAME_FIELDS.index("pf1")], frame[sp.FRAME_FIELDS.index("pb1")], frame[sp.FRAME_FIELDS.index("pa1")] = f, bw, 1.0
        r = eng.frameResponse(frame, sr, freqs, kinds=("parallel_re", "parallel_im"))[0]
        want = 2 * (r[0] + 1j * r[1]) + 1
        sos = eng.resonatorSections(f, bw, sr)
        abc = eng.resonatorCoefficients(f, bw, sr)[0]
        assert sos.shape == (1, 6) and list(sos[0]) == [abc[0], 0, 0, 1, -abc[1], -abc[2]]
        got = response(sos, freqs, sr)
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (f, bw, sr)
    assert eng.resonatorSections([300, 900, 2500], [60, 90, 150], 22050).shape == (3, 6)


def test_biquads_against_scipy():
    """biquad magnitudes against scipy.signal.sosfreqz: -3 dB at f0 for low-pass and high-pass, gainDb at f0 for peaking."""
    signal = pytest.importorskip("scipy.signal")
    import nvspeechplayer_amd as eng
    rate = 16000
    for kind, f0, kw, want in (("lowpass", 3400.0, {}, -10 * np.log10(2.0)), ("highpass", 300.0, {}, -10 * np.log10(2.0)),
                               ("peaking", 1200.0, dict(q=2.0, gainDb=4.5), 4.5), ("peaking", 700.0, dict(q=0.8, gainDb=-9.0), -9.0)):
        sos = eng.biquad(kind, rate, f0, **kw)
        w, h = signal.sosfreqz(sos, worN=[f0], fs=rate)
        assert abs(20 * np.log10(abs(h[0])) - want) < 1e-9, (kind, f0)


def test_filter_request_checks():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    import nvspeechplayer_amd as eng
    check = sp.check_filter_request
    one = stable(2, 1)
    sec, start, of, tail, fmt = check(one, None, 3, 0, None)
    assert sec.dtype == np.float32 and sec.shape == (2, 5) and list(start) == [0, 2] and of is None and (tail, fmt) == (0, 1)
    sec, start, of, tail, fmt = check([one, TELEPHONE, torch.tensor(stable(16, 2))], [2, 0, 1, 1], 4, 7, torch.int16)
    assert sec.shape == (22, 5) and list(start) == [0, 2, 6, 22] and of.dtype == np.int64 and list(of) == [2, 0, 1, 1] and (tail, fmt) == (7, 0)
    assert np.array_equal(sec[2:6], (TELEPHONE[:, [0, 1, 2, 4, 5]] / TELEPHONE[:, 3:4]).astype(np.float32))
    assert check([[1, 0, 0, 0, 0]], None, 1, sp.FILTER_MAX_TAIL, np.int16)[0].shape == (1, 5)
    assert len(check([stable(16, 3)] * 4096, np.zeros(2, np.int32), 2, 0, torch.float32)[0]) == sp.FILTER_MAX_TABLE
    value = dict(no_filters=([], None, 0), seventeen=(np.tile(IDENTITY, (17, 1)), None, 0), table=([stable(16, 3)] * 4097, [0, 0], 0), of_beyond=([one, one], [0, 2], 0),
                 of_negative=([one, one], [-1, 0], 0), of_missing=([one, one], None, 0), of_short=([one, one], [0], 0), of_long=(one, [0, 0, 0], 0),
                 tail_negative=(one, None, -1), tail_large=(one, None, sp.FILTER_MAX_TAIL + 1), tail_real=(one, None, 1.0), tail_bool=(one, None, True),
                 a0_zero=(np.array([[1, 0, 0, 0, 0, 0.0]]), None, 0))
    for name, (filters, of, tail) in value.items():
        with pytest.raises(ValueError):
            check(filters, of, 2, tail, None)
            pytest.fail(name)
    for name, (filters, of, dtype) in dict(one_d=(np.ones(5), None, None), four=(np.ones((2, 4)), None, None), seven=(np.ones((2, 7)), None, None), scalar=(1.0, None, None),
                                           complex_=(np.ones((1, 5), np.complex64), None, None), of_real=([one, one], [0.0, 1.0], None), float64=(one, None, torch.float64),
                                           int32=(one, None, np.int32)).items():
        with pytest.raises(TypeError):
            check(filters, of, 2, 0, dtype)
            pytest.fail(name)
    for pcm in (np.zeros(10, np.float32), np.zeros((2, 10), np.int16), [1, 2, 3]):
        with pytest.raises(TypeError):
            eng.pcmFilter(pcm, one)
    with pytest.raises(TypeError):
        eng.signalFilter(np.zeros(10, np.float64), one)
    with pytest.raises(ValueError):
        eng.pcmFilter(np.zeros(10, np.int16), [one, one])
    # the values are the library's to refuse, with the filter and the section in its words
    for name, (q, v) in dict(nan=(1, np.nan), inf=(0, np.inf), on_the_circle=(4, 1.0), a1_at_the_edge=(3, 1.25)).items():
        bad = one.copy()
        bad[1, 3:] = [0.5, 0.25]
        bad[1, q] = v
        with pytest.raises(RuntimeError, match="section 1 of filter 0"):
            eng.pcmFilter(np.zeros(10, np.int16), bad)
            pytest.fail(name)
    with pytest.raises(RuntimeError, match="sample 3 is"):
        x = np.zeros(10, np.float32)
        x[3] = np.inf
        eng.signalFilter(x, one)


REFUSED_HOST = dict(
    tail_negative=dict(tail=-1), tail_above=dict(tail=(1 << 20) + 1), no_sections=dict(sections=None), sections_zero=dict(n=0), sections_negative=dict(n=-3),
    sections_17=dict(n=17), b0_nan=dict(bad=(0, float("nan"))), b1_inf=dict(bad=(1, float("inf"))), b2_minus_inf=dict(bad=(2, -float("inf"))), a1_nan=dict(bad=(3, float("nan"))),
    a2_inf=dict(bad=(4, float("inf"))), a2_one=dict(bad=(4, 1.0)), a2_above=dict(bad=(4, 1.5)), a1_edge=dict(bad=(3, 1.25)), a1_minus_edge=dict(bad=(3, -1.25)),
    a1_beyond=dict(bad=(3, 3.0)), a2_minus_one=dict(bad=(4, -1.0), a1=0.0), format_2=dict(fmt=2), format_negative=dict(fmt=-1), length_negative=dict(length=-1),
    no_pcm=dict(pcm=None), capacity_short=dict(capacity=204))


def test_every_refusal_of_the_c_entry_points():
    """Every refusal of speechPlayer_pcmFilter and signalFilter writes nothing and names what it refuses; a pole exactly on the circle
    (a2 = 1) and |a1| = 1 + a2 are among them, and the nearest float32 values inside are admitted."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    pcm = np.arange(200, dtype=np.int16)
    out = np.full(400, -7.0, np.float32)
    base = np.tile(np.array([0.5, 0.25, 0.125, 0.5, 0.25], np.float32), (17, 1))      # |a1| < 1 + a2 = 1.25

    def run(pcm=pcm, length=200, sections=base, n=3, tail=5, fmt=1, out=out, capacity=400, bad=None, a1=None, of_signal=None):
        p = lambda a: None if a is None else a.ctypes.data
        s = sections
        if bad is not None:
            s = sections.copy()
            s[2, bad[0]] = bad[1]
            if a1 is not None:
                s[2, 3] = a1
        if of_signal is None:
            return L.speechPlayer_pcmFilter(p(pcm), length, p(s), n, tail, fmt, p(out), capacity)
        return L.speechPlayer_signalFilter(p(pcm), of_signal, length, p(s), n, tail, fmt, p(out), capacity)

    for name, kw in REFUSED_HOST.items():
        assert run(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"pcmFilter" in L.speechPlayer_lastError(), name
        if "bad" in kw:
            assert b"section 2 of filter 0" in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        assert np.all(out == -7.0), name
    assert run(bad=(1, float("nan"))) == -1 and b"b1 of section 2 of filter 0" in L.speechPlayer_lastError()
    assert run(bad=(4, 1.0)) == -1 and b"unit circle" in L.speechPlayer_lastError()
    x = np.linspace(-1, 1, 200).astype(np.float32)
    for name, kw in dict(in_format_2=dict(of_signal=2), in_format_negative=dict(of_signal=-1), sample_nan=dict(pcm=np.where(np.arange(200) == 9, np.nan, x).astype(np.float32), of_signal=1),
                         sample_large=dict(pcm=np.where(np.arange(200) == 9, 65537.0, x).astype(np.float32), of_signal=1), a2_one=dict(pcm=x, of_signal=1, bad=(4, 1.0))).items():
        assert run(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"signalFilter" in L.speechPlayer_lastError(), name
        assert np.all(out == -7.0), name
    # sizing, nothing to compute, the limits themselves, and the entry points are as usable as before
    assert run(out=None, capacity=0) == 205 and run(out=None, capacity=0, tail=1 << 20) == 200 + (1 << 20) and L.speechPlayer_lastErrorCode() == 0
    assert run(pcm=None, length=0, out=None) == 5 and run(pcm=None, length=0, tail=0) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert run(capacity=205) == 205 and np.all(out[:205] != -7.0) and np.all(out[205:] == -7.0)
    inside = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert run(bad=(4, inside), a1=0.0, n=16) == 205 and run(bad=(3, np.nextafter(np.float32(1.25), np.float32(0.0)))) == 205
    assert run(bad=(3, -np.nextafter(np.float32(1.25), np.float32(0.0)))) == 205 and run(bad=(4, np.nextafter(np.float32(-1.0), np.float32(0.0))), a1=0.0) == 205
    assert run(pcm=x, of_signal=1) == 205 and np.isfinite(out[:205]).all()


def test_the_packing_and_the_kernels_walk_under_sanitizers(tmp_path):
    """csrc/klatt_filter.h (filter_pack, filter_bucket, the statement and a model of the kernel's loads, in-place staging and stores) in a
    program of its own, tests/native/check_filter_pack.cpp, under AddressSanitizer + UBSan: 0, 1, 63, 64, 65 and 130 rows of mixed K and
    lengths -- every row once, one bucket per group, lengths within a group non-increasing, the rows untouched.  Nothing loaded into
    python is run under a sanitizer."""
    exe = str(tmp_path / "check_filter_pack")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_filter_pack.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out
