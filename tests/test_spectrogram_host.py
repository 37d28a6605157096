"""The STFT / band spectrogram on the host (include/speechPlayer_batch.h: speechPlayer_pcmSpectrogram; nvspeechplayer_amd.pcmSpectrogram,
melFilterbank, check_spectrogram_request; csrc/klatt_spectrum.h): the product's CPU statement of the definition against numpy's float64
rfft within the forward error bound of a float32 radix-2 transform, its framing, its band sums, its logarithm, the mel filterbank and
every refusal.  `bound` and `frames_of` are the comparands tests/test_gpu_spectrogram.py shares.  No GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
U = 2.0 ** -24
SIZES = [64, 256, 1024, 4096]


def hann(n):
    """The default window as the library makes it: periodic Hann in float64, rounded to float32."""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def frames_of(pcm, n, hop, phase, window32):
    """x w of every step, float64 [steps, n]: the float32 products of the definition (s / 32767 and the window product are single
    float32 operations, which numpy performs exactly so), zeros outside the signal."""
    L = len(pcm)
    steps = -(-(L - phase) // hop) if L > phase else 0
    x = np.zeros(L + 2 * n + steps * hop + phase, np.float32)
    x[n:n + L] = pcm.astype(np.float32) / np.float32(32767.0)
    at = n + phase + np.arange(steps)[:, None] * hop - n // 2 + np.arange(n)[None, :]
    return (x[at] * window32[None, :]).astype(np.float64)


def bound(xw, n):
    """B of the issue per step: (8 log2 n + 8) u sqrt(n) ||x w||_2 (Higham Thm 24.2 with eta <= 8 u, 8 u more for the scaling, the
    window product and the unpacking pass; csrc/klatt_spectrum.h derives that the half-length factorisation keeps the constant)."""
    return (8 * math.log2(n) + 8) * U * math.sqrt(n) * np.sqrt((xw * xw).sum(axis=-1))


def check_against_rfft(got, pcm, n, hop, phase, window32=None):
    """got [steps, n / 2 + 1] (power 1, linear) within B + 4 u |X_k| of numpy's float64 rfft of the float32 products."""
    xw = frames_of(pcm, n, hop, phase, hann(n) if window32 is None else window32)
    want = np.abs(np.fft.rfft(xw, axis=-1))
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    lim = bound(xw, n)[:, None] + 4 * U * want
    assert np.all(err <= lim), (n, float((err / np.maximum(lim, 1e-300)).max()))
    return float((err / np.maximum(bound(xw, n)[:, None], 1e-300)).max()) if len(got) else 0.0


def signals(n, rng):
    L = 2 * n + 37
    t = np.arange(L)
    return {
        "random": rng.integers(-32767, 32768, L).astype(np.int16),
        "sine": np.round(30000 * np.sin(2 * np.pi * 0.0731 * t)).astype(np.int16),
        "constant": np.full(L, 12345, np.int16),
        "tiny": (t % 2).astype(np.int16),
        "full_scale": np.where(t % 3 == 0, 32767, -32767).astype(np.int16),
    }


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs in (("speechPlayer_pcmSpectrogram", 12), ("speechPlayer_batch_exportSpectrogram", 16)):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and len(fn.argtypes) == nargs, name
    assert "MODE_FAST" in header.split("speechPlayer_pcmSpectrogram(")[0].split("The STFT and band")[1]      # the dependence on the PCM is stated
    assert callable(speechPlayer.BatchPlayer.spectrogramTensor)
    assert nvspeechplayer_amd.pcmSpectrogram is speechPlayer.pcmSpectrogram and nvspeechplayer_amd.melFilterbank is speechPlayer.melFilterbank


@pytest.mark.parametrize("n", SIZES)
def test_the_statement_against_numpy_float64(n):
    """power 1, no bank, no log: every bin within B + 4 u |X_k| of np.fft.rfft; silence is +0 on its bits."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(n)
    worst = {}
    for name, pcm in signals(n, rng).items():
        got = eng.pcmSpectrogram(pcm, nFft=n, hop=n // 4, power=1)
        worst[name] = check_against_rfft(got, pcm, n, n // 4, 0)
    print("nFft %d: largest error over B: %s" % (n, ", ".join("%s %.4f" % kv for kv in worst.items())))
    for power in (1, 2):
        zero = eng.pcmSpectrogram(np.zeros(n + 5, np.int16), nFft=n, hop=n // 4, power=power)
        assert zero.shape == (5, n // 2 + 1) and not zero.view(np.uint64).any()
    # power 2 is the float32 sum of squares whose binary64 square root, rounded to float32, power 1 gives
    pcm = signals(n, rng)["random"]
    p2 = eng.pcmSpectrogram(pcm, nFft=n, hop=n, power=2)
    p1 = eng.pcmSpectrogram(pcm, nFft=n, hop=n, power=1)
    assert np.array_equal(p1, np.sqrt(p2).astype(np.float32).astype(np.float64))
    assert np.array_equal(p2, p2.astype(np.float32).astype(np.float64))
    # a window of the caller's
    w = rng.uniform(-1.0, 1.0, n)
    check_against_rfft(eng.pcmSpectrogram(pcm, nFft=n, hop=n // 2, window=w, power=1), pcm, n, n // 2, 0, w.astype(np.float32))


@pytest.mark.parametrize("n", SIZES)
def test_framing(n):
    """Step counts are ceil((L - phase) / hop); the frame of step j is centred on phase + j * hop with zeros outside the signal: an
    impulse at t0 gives |X_k| = w[t0 - c + n / 2] / 32767 in every bin, within B."""
    import nvspeechplayer_amd as eng
    w = hann(n).astype(np.float64)
    for L in (1, n // 2 - 1, n // 2, n + 3):
        for hop in (1, 7, n // 4, n + 5):
            if n == 4096 and hop < 16 and L > 1:
                continue      # (thousands of 4096-point frames: the same code paths run at the smaller sizes)
            for phase in (0, 5, L):
                t0 = L - 1
                pcm = np.zeros(L, np.int16)
                pcm[t0] = 20000
                got = eng.pcmSpectrogram(pcm, nFft=n, hop=hop, phase=phase, power=1)
                steps = -(-(L - phase) // hop) if L > phase else 0
                assert got.shape == (steps, n // 2 + 1), (L, hop, phase)
                for j in range(steps):
                    i = t0 - (phase + j * hop) + n // 2
                    amp = float(np.float32(np.float32(20000) / np.float32(32767.0)) * np.float32(w[i])) if 0 <= i < n else 0.0
                    B = (8 * math.log2(n) + 8) * U * math.sqrt(n) * abs(amp)
                    assert np.all(np.abs(got[j] - abs(amp)) <= B + 4 * U * abs(amp)), (L, hop, phase, j)
                check_against_rfft(got, pcm, n, hop, phase)


def test_bands():
    """A band is the float32 sum, in ascending k, of w[b][k] v[k] over its non-zero column range: within (nnz + 1) u sum |w v| of the
    float64 sum over the statement's own bin values; an all-zero row is +0."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(5)
    n = 256
    pcm = rng.integers(-20000, 20000, 3 * n).astype(np.int16)
    for power in (1, 2):
        bins = eng.pcmSpectrogram(pcm, nFft=n, hop=100, power=power)
        for bank in (eng.melFilterbank(22050, n, 20), eng.melFilterbank(16000, n, 8, norm="slaney"), rng.uniform(-1, 1, (5, n // 2 + 1)),
                     np.concatenate([np.zeros((1, n // 2 + 1)), np.eye(n // 2 + 1)[[0, n // 2]], np.zeros((1, n // 2 + 1))])):
            got = eng.pcmSpectrogram(pcm, nFft=n, hop=100, bank=bank, power=power)
            w32 = bank.astype(np.float32).astype(np.float64)
            want = bins @ w32.T
            nnz = (w32 != 0).sum(axis=1)
            lim = (nnz + 1)[None, :] * U * (bins @ np.abs(w32).T)
            assert got.shape == want.shape and np.all(np.abs(got - want) <= lim)
            empty = nnz == 0
            assert not got[:, empty].view(np.uint64).any()
            assert np.array_equal(got, got.astype(np.float32).astype(np.float64))      # float32 values, widened
    # the order of the sum: one band, ascending k, each step one float32 product and one float32 sum
    bank = rng.uniform(0, 1, (1, n // 2 + 1))
    bank[0, :7] = 0
    bank[0, -3:] = 0
    got = eng.pcmSpectrogram(pcm, nFft=n, hop=100, bank=bank, power=2)
    bins = eng.pcmSpectrogram(pcm, nFft=n, hop=100, power=2).astype(np.float32)
    acc = np.zeros(len(bins), np.float32)
    for k in range(7, n // 2 + 1 - 3):
        acc = acc + np.float32(bank[0, k]) * bins[:, k]
    assert np.array_equal(got[:, 0], acc.astype(np.float64))


def ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_log():
    """logScale log10(max(v, floor)) in binary64, within 4 ulp of numpy's (the bar of tests/test_gpu_response.py for log10); the floor
    clamps zeros to a finite value."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(6)
    n = 256
    pcm = np.concatenate([rng.integers(-20000, 20000, 2 * n), np.zeros(2 * n, np.int64)]).astype(np.int16)
    bank = eng.melFilterbank(22050, n, 12)
    for power in (1, 2):
        for kw in (dict(), dict(bank=bank)):
            lin = eng.pcmSpectrogram(pcm, nFft=n, hop=64, power=power, **kw)
            assert (lin == 0).any() and (lin > 0).any()
            for log, scale, floor in (("db", 10.0 if power == 2 else 20.0, 1e-10), ("ln", math.log(10.0), 1e-5), (3.5, 3.5, 0.25), (-20, -20.0, 1e-300)):
                got = eng.pcmSpectrogram(pcm, nFft=n, hop=64, power=power, log=log, floor=floor, **kw)
                want = scale * np.log10(np.maximum(lin, floor))
                assert np.all(np.isfinite(got)) and ulps(got, want).max() <= 4, (power, log)
                assert np.all(ulps(got[lin == 0], scale * math.log10(floor)) <= 4)
            assert np.array_equal(eng.pcmSpectrogram(pcm, nFft=n, hop=64, power=power, log=0, floor=-1.0, **kw), lin)      # 0: linear, no floor needed


def test_mel_filterbank():
    import nvspeechplayer_amd as eng
    for sr, n, m, fmin, fmax in ((22050, 1024, 80, 0.0, None), (16000, 512, 40, 50.0, 7600.0), (22050, 64, 8, 0.0, None), (44100, 4096, 128, 20.0, 16000.0)):
        bank = eng.melFilterbank(sr, n, m, fmin=fmin, fmax=fmax)
        assert bank.shape == (m, n // 2 + 1) and bank.dtype == np.float64
        assert np.all(bank >= 0) and np.all(bank <= 1)
        for row in bank:
            nz = np.flatnonzero(row)
            assert len(nz) == 0 or np.all(np.diff(nz) == 1)      # one contiguous run
        top = sr / 2.0 if fmax is None else fmax
        mel = np.linspace(2595 * math.log10(1 + fmin / 700), 2595 * math.log10(1 + top / 700), m + 2)
        f = 700 * (10 ** (mel / 2595) - 1)
        bins = np.arange(n // 2 + 1) * sr / n
        between = (bins >= f[1]) & (bins <= f[-2])
        assert between.any() and np.all(np.abs(bank[:, between].sum(axis=0) - 1) <= 1e-12)      # the triangles partition unity
        slaney = eng.melFilterbank(sr, n, m, fmin=fmin, fmax=fmax, norm="slaney")
        assert np.allclose(slaney, bank * (2.0 / (f[2:] - f[:-2]))[:, None], rtol=1e-13, atol=0)
    for bad in (dict(nMels=0), dict(fmin=-1.0), dict(fmin=9000.0, fmax=8000.0), dict(norm="htk")):
        kw = dict(sampleRate=22050, nFft=1024, nMels=80)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.melFilterbank(**kw)


def test_spectrogram_request_checks():
    import torch
    from nvspeechplayer_amd.speechPlayer import check_spectrogram_request
    ok = dict(nFft=1024, hop=256, phase=0, window=None, bank=None, power=2, log=None, floor=1e-10, dtype=None)

    def check(**kw):
        a = dict(ok)
        a.update(kw)
        return check_spectrogram_request(**a)

    assert check() == (1024, 256, 0, None, None, 513, 2, 0.0, 1e-10, 1)
    n, hop, phase, window, bank, bands, power, scale, floor, fmt = check(nFft=np.int64(64), hop=3, phase=7, window=np.ones(64, np.float32), bank=torch.ones(4, 33),
                                                                         power=1, log="db", floor=1e-3, dtype=torch.float64)
    assert (n, hop, phase, bands, power, scale, floor, fmt) == (64, 3, 7, 4, 1, 20.0, 1e-3, 0)
    assert window.dtype == np.float64 and window.shape == (64,) and bank.dtype == np.float64 and bank.shape == (4, 33) and bank.flags.c_contiguous
    assert check(log="db")[7] == 10.0 and check(log="ln")[7] == math.log(10.0) and check(log=-3)[7] == -3.0 and check(log=0, floor=0.0)[7] == 0.0
    assert check(floor=-1.0)[8] == -1.0      # no logarithm: the floor is not looked at
    refused = dict(
        nfft_small=dict(nFft=32), nfft_large=dict(nFft=8192), nfft_not_a_power=dict(nFft=1000), nfft_float=dict(nFft=1024.0), nfft_bool=dict(nFft=True),
        hop_zero=dict(hop=0), hop_negative=dict(hop=-4), phase_negative=dict(phase=-1),
        window_short=dict(window=np.ones(1023)), window_nan=dict(window=np.where(np.arange(1024) == 5, np.nan, 1.0)),
        window_inf=dict(window=np.where(np.arange(1024) == 5, np.inf, 1.0)),
        bank_flat=dict(bank=np.ones(513)), bank_narrow=dict(bank=np.ones((80, 512))), bank_empty=dict(bank=np.ones((0, 513))),
        bank_nan=dict(bank=np.where(np.arange(513) == 9, np.nan, np.ones((2, 513)))),
        power_0=dict(power=0), power_3=dict(power=3), power_float=dict(power=1.5), power_bool=dict(power=True),
        log_name=dict(log="log"), log_nan=dict(log=float("nan")), log_inf=dict(log=float("inf")),
        floor_zero=dict(log="db", floor=0.0), floor_negative=dict(log=10, floor=-1e-10), floor_nan=dict(log="ln", floor=float("nan")),
        floor_inf=dict(floor=float("inf")))
    for name, kw in refused.items():
        with pytest.raises(ValueError):
            check(**kw)
            pytest.fail(name)
    for dtype in (torch.float16, torch.int16, np.float32):
        with pytest.raises(TypeError):
            check(dtype=dtype)
    import nvspeechplayer_amd as eng
    for bad in (np.zeros(10, np.float32), np.zeros((2, 10), np.int16), [1, 2, 3]):
        with pytest.raises(TypeError):
            eng.pcmSpectrogram(bad)
    with pytest.raises(ValueError):
        eng.pcmSpectrogram(np.zeros(10, np.int16), nFft=100)


def test_every_refusal_of_the_c_entry_point():
    from nvspeechplayer_amd import _native
    L = _native.load()
    pcm = np.arange(200, dtype=np.int16)
    window = np.ones(64)
    bank = np.ones((3, 33))
    out = np.full(200 * 33 + 1, -7.0)
    nan, inf = float("nan"), float("inf")

    def call(pcm=pcm, length=200, nfft=64, hop=16, phase=0, window=None, bank=None, nbands=0, power=2, scale=0.0, floor=0.0, out=out):
        p = lambda a: None if a is None else a.ctypes.data
        return L.speechPlayer_pcmSpectrogram(p(pcm), length, nfft, hop, phase, p(window), p(bank), nbands, power, scale, floor, p(out))

    refused = dict(
        nfft_32=dict(nfft=32), nfft_8192=dict(nfft=8192), nfft_96=dict(nfft=96), nfft_zero=dict(nfft=0), nfft_negative=dict(nfft=-64),
        hop_zero=dict(hop=0), hop_negative=dict(hop=-1), phase_negative=dict(phase=-1), length_negative=dict(length=-1), no_pcm=dict(pcm=None),
        no_output=dict(out=None), power_0=dict(power=0), power_3=dict(power=3), bands_zero=dict(bank=bank, nbands=0), bands_negative=dict(bank=bank, nbands=-3),
        window_nan=dict(window=np.where(np.arange(64) == 63, nan, 1.0)), window_inf=dict(window=np.where(np.arange(64) == 0, -inf, 1.0)),
        bank_nan=dict(bank=np.where(np.arange(33) == 32, nan, bank), nbands=3), bank_inf=dict(bank=np.where(np.arange(33) == 0, inf, bank), nbands=3),
        floor_zero=dict(scale=10.0, floor=0.0), floor_negative=dict(scale=10.0, floor=-1.0), floor_nan=dict(scale=10.0, floor=nan),
        floor_inf=dict(floor=inf), scale_nan=dict(scale=nan, floor=1.0), scale_inf=dict(scale=inf, floor=1.0))
    for name, kw in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"pcmSpectrogram" in L.speechPlayer_lastError(), name
        assert np.all(out == -7.0), name
    # nothing to compute: 0, and neither PCM nor output needed
    assert call(pcm=None, length=0, out=None) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert call(phase=200, out=None) == 0 and call(phase=1 << 62, out=None) == 0
    # the entry point is as usable as before, and writes what it says
    assert call(window=window, bank=bank, nbands=3, power=1, scale=20.0, floor=1e-7) == 13 * 3
    assert np.all(out[:39] != -7.0) and np.all(out[39:] == -7.0)
    assert call(hop=1 << 50) == 33 and call(length=1, hop=1) == 33


def test_the_statement_under_sanitizers(tmp_path):
    """csrc/klatt_spectrum.h (the plan, the framing, the transform, the bands, the logarithm) in a program of its own,
    tests/native/check_spectrum.cpp, against a direct float64 DFT under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "check_spectrum")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_spectrum.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out
