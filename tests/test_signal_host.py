"""The signal-reading exports on the host (include/speechPlayer_batch.h: speechPlayer_signalSpectrogram, speechPlayer_signalResample,
speechPlayer_signalConvolve; nvspeechplayer_amd.signalSpectrogram / signalResample / signalConvolve, check_signal_request;
csrc/klatt_tiles.h: the reader): on int16 input and on its float32 form the statements give speechPlayer_pcm*'s bits; on float32 input
that is not of PCM form they stay within the float64 bounds the three host test modules state for these definitions; every refusal;
and the reader's index functions against brute force in a program of their own under the sanitizers.  `x_signals`, `conv_reference`,
`res_reference` and `check_spectrum` are the comparands tests/test_gpu_signal.py shares.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.test_convolve_host import decaying, gamma, to_int16
from tests.test_resample_host import FILTERS
from tests.test_resample_host import gamma as res_gamma
from tests.test_spectrogram_host import U, bound, hann

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
PAIRS = [(22050, 16000), (16000, 22050), (32000, 16000)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def float_form(pcm):
    """(s / 32767) in float32 division: the pool's samples as format 1 gives them."""
    return np.asarray(pcm).astype(np.float32) / np.float32(32767.0)


def x_signals(L, seed):
    """Seeded float32 signals that no int16 PCM gives: uniform noise beyond full scale, a decaying burst (its products stay normal
    numbers: the bounds are relative ones, which underflow is outside of) and noise at 2^16, the bound of the promise."""
    rng = np.random.default_rng(4000 + seed)
    t = np.arange(L)
    return {
        "noise": rng.uniform(-1.5, 1.5, L).astype(np.float32),
        "burst": (rng.standard_normal(L) * 3.0 * np.exp(-t / 200.0)).astype(np.float32),
        "large": (rng.uniform(-1.0, 1.0, L) * 65536.0).astype(np.float32),
    }


def conv_reference(x, h, tail=True):
    """tests/test_convolve_host.py's reference on float32 samples: numpy's float64 convolution -> (y, conv(|x|, |h|))."""
    x, h = np.asarray(x, np.float32).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
    if len(x) == 0:
        return np.zeros(0), np.zeros(0)
    y, mag = np.convolve(x, h), np.convolve(np.abs(x), np.abs(h))
    return (y, mag) if tail else (y[:len(x)], mag[:len(x)])


def res_reference(x, table, up, down):
    """tests/test_resample_host.py's reference on float32 samples: the float64 sum over the float32 operands -> (y, sum |x| |h|)."""
    L, taps = len(x), table.shape[1]
    Z = taps // 2
    Lout = -(-L * up // down)
    xp = np.zeros(L + 2 * Z, np.float32)
    xp[Z:Z + L] = x
    m = np.arange(Lout, dtype=np.int64)
    n0, p = m * down // up, m * down % up
    at = n0[:, None] + np.arange(taps)[None, :] + 1
    terms = xp[at].astype(np.float64) * table[p]
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def check_spectrum(got, x, n, hop, phase):
    """tests/test_spectrogram_host.py's check_against_rfft on float32 samples (power 1, linear): within B + 4 u |X_k| of numpy's rfft."""
    L = len(x)
    steps = -(-(L - phase) // hop) if L > phase else 0
    xp = np.zeros(L + 2 * n + steps * hop + phase, np.float32)
    xp[n:n + L] = x
    at = n + phase + np.arange(steps)[:, None] * hop - n // 2 + np.arange(n)[None, :]
    xw = (xp[at] * hann(n)[None, :]).astype(np.float64)
    want = np.abs(np.fft.rfft(xw, axis=-1))
    assert got.shape == want.shape, (got.shape, want.shape)
    err, lim = np.abs(got - want), bound(xw, n)[:, None] + 4 * U * want
    assert np.all(err <= lim), (n, float((err / np.maximum(lim, 1e-300)).max()))


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs in (("speechPlayer_batch_exportSpectrogramOf", 17), ("speechPlayer_batch_exportResampledOf", 14), ("speechPlayer_batch_exportConvolvedOf", 13),
                        ("speechPlayer_signalSpectrogram", 13), ("speechPlayer_signalResample", 12), ("speechPlayer_signalConvolve", 9)):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and len(fn.argtypes) == nargs, name
    section = header.split("The exports of a signal:")[1].split("speechPlayer_batch_device(")[0]
    for word in ("speechPlayer_signal_t", "2^16", "steers an address", "never read as signal", "the caller's job", "never been set", "names the row"):
        assert word in section, word
    for name in ("signalSpectrogram", "signalResample", "signalConvolve", "check_signal_request"):
        assert getattr(nvspeechplayer_amd, name) is getattr(speechPlayer, name), name
    # the conversion of an int16 sample is written once, in the reader, and the three kernels read through it
    csrc = os.path.join(ROOT, "nvspeechplayer_amd", "csrc")
    assert open(os.path.join(csrc, "klatt_tiles.h")).read().count("/ 32767.0f;") == 1
    for kernel, reader in (("klatt_resample.h", "tile_read<1>"), ("klatt_convolve.h", "tile_read<-1>"), ("klatt_spectrum.h", "tile_sample(")):
        text = open(os.path.join(csrc, kernel)).read()
        assert "/ 32767.0f;" not in text and reader in text, kernel


def test_int16_and_its_float_form_give_the_pcm_statements_bits():
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(21)
    pcm = rng.integers(-32768, 32768, 1500).astype(np.int16)
    pcm[:3] = (-32768, 32767, 0)
    x = float_form(pcm)
    for L in (0, 1, 3, 1500):
        for src, dst in PAIRS + [(16000, 16000)]:
            for kw in (FILTERS[0], FILTERS[2]):
                for dtype in (np.float32, np.int16):
                    want = eng.pcmResample(pcm[:L], src, dst, dtype=dtype, **kw)
                    for given in (pcm[:L], x[:L]):
                        got = eng.signalResample(given, src, dst, dtype=dtype, **kw)
                        assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), (L, src, dst, dtype, given.dtype)
        for K in (1, 5, 1025):
            h = decaying(K, K)
            for tail in (True, False):
                for dtype in (np.float32, np.int16):
                    want = eng.pcmConvolve(pcm[:L], h, tail=tail, dtype=dtype)
                    for given in (pcm[:L], x[:L]):
                        got = eng.signalConvolve(given, h, tail=tail, dtype=dtype)
                        assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), (L, K, tail, dtype, given.dtype)
        for n in (64, 256):
            for kw in (dict(power=1), dict(power=2, bank=eng.melFilterbank(16000, n, 8), log="ln", floor=1e-5), dict(hop=n + 5, phase=2)):
                kw = dict(dict(nFft=n, hop=n // 4), **kw)
                want = eng.pcmSpectrogram(pcm[:L], **kw)
                for given in (pcm[:L], x[:L]):
                    got = eng.signalSpectrogram(given, **kw)
                    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (L, n, sorted(kw), given.dtype)


def test_float_signals_against_numpy_float64():
    """Input no PCM gives: each statement within the bound its own host test module states for the definition."""
    import nvspeechplayer_amd as eng
    for name, x in x_signals(1300, 1).items():
        for K in (1, 5, 1025):
            h = decaying(K, 40 + K)
            for tail in (True, False):
                got = eng.signalConvolve(x, h, tail=tail)
                want, mag = conv_reference(x, h, tail)
                assert got.dtype == np.float32 and got.shape == want.shape
                assert np.all(np.abs(got.astype(np.float64) - want) <= gamma(K) * mag), (name, K, tail)
                assert np.array_equal(eng.signalConvolve(x, h, tail=tail, dtype=np.int16), to_int16(got)), (name, K, tail)
        for src, dst in PAIRS:
            for kw in (FILTERS[0], FILTERS[2]):
                table, up, down = eng.resampleKernel(src, dst, **kw)
                got = eng.signalResample(x, src, dst, **kw)
                want, mag = res_reference(x, table, up, down)
                assert got.dtype == np.float32 and got.shape == want.shape
                assert np.all(np.abs(got.astype(np.float64) - want) <= res_gamma(table.shape[1]) * mag), (name, src, dst, kw)
                assert np.array_equal(eng.signalResample(x, src, dst, dtype=np.int16, **kw), to_int16(got)), (name, src, dst)
        # equal rates: the samples themselves, -0.0 included
        y = x.copy()
        y[5] = -0.0
        assert np.array_equal(bits(eng.signalResample(y, 16000, 16000)), bits(y))
        assert np.array_equal(eng.signalResample(y, 16000, 16000, dtype=np.int16), to_int16(y))
        for n in (64, 256):
            for hop, phase in ((n // 4, 0), (37, 5)):
                check_spectrum(eng.signalSpectrogram(x, nFft=n, hop=hop, phase=phase, power=1), x, n, hop, phase)
    # silence is +0 on its bits
    z = np.zeros(300, np.float32)
    assert not bits(eng.signalConvolve(z, decaying(5, 1))).any() and not bits(eng.signalResample(z, 22050, 16000)).any()
    assert not bits(eng.signalSpectrogram(z, nFft=64, hop=16)).any()


def test_every_refusal_of_the_c_entry_points():
    from nvspeechplayer_amd import _native
    L = _native.load()
    p = lambda a: None if a is None else a.ctypes.data
    x = np.linspace(-1, 1, 200).astype(np.float32)
    s = np.arange(200, dtype=np.int16)
    out = np.full(4000, -7.0, np.float32)
    out64 = np.full(4000, -7.0, np.float64)
    ir = np.full(16, 0.25, np.float32)

    def spectrogram(x=x, inFormat=1, length=200, nFft=64, hop=16, phase=0, power=2, out=out64):
        return L.speechPlayer_signalSpectrogram(p(x), inFormat, length, nFft, hop, phase, None, None, 0, power, 0.0, 0.0, p(out))

    def resample(x=x, inFormat=1, length=200, src=22050, dst=16000, zeros=6, fmt=1, out=out, capacity=4000):
        return L.speechPlayer_signalResample(p(x), inFormat, length, src, dst, zeros, 0.99, 0, 0.0, fmt, p(out), capacity)

    def convolve(x=x, inFormat=1, length=200, ir=ir, taps=16, tail=1, fmt=1, out=out, capacity=4000):
        return L.speechPlayer_signalConvolve(p(x), inFormat, length, p(ir), taps, tail, fmt, p(out), capacity)

    def poisoned(value, at=13):
        y = x.copy()
        y[at] = value
        return y

    common = dict(format_2=dict(inFormat=2), format_negative=dict(inFormat=-1), length_negative=dict(length=-1), no_samples=dict(x=None),
                  nan=dict(x=poisoned(np.nan)), inf=dict(x=poisoned(np.inf)), minus_inf=dict(x=poisoned(-np.inf)),
                  above=dict(x=poisoned(np.float32(65536.0) * (1 + np.float32(2.0 ** -23)))), below=dict(x=poisoned(-1e30)))
    own = {
        "signalSpectrogram": (spectrogram, dict(nFft_100=dict(nFft=100), hop_0=dict(hop=0), phase_negative=dict(phase=-1), power_3=dict(power=3), no_output=dict(out=None))),
        "signalResample": (resample, dict(length_huge=dict(length=(1 << 44) + 1), rate_0=dict(src=0), out_rate_0=dict(dst=0), zeros_0=dict(zeros=0), out_format=dict(fmt=2),
                                          capacity=dict(capacity=100))),
        "signalConvolve": (convolve, dict(length_huge=dict(length=(1 << 44) + 1), tail_2=dict(tail=2), no_ir=dict(ir=None), taps_0=dict(taps=0), out_format=dict(fmt=2),
                                          capacity=dict(capacity=100))),
    }
    for what, (call, cases) in own.items():
        for name, kw in list(common.items()) + list(cases.items()):
            assert call(**kw) == -1, (what, name)
            assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and what.encode() in L.speechPlayer_lastError(), (what, name, L.speechPlayer_lastError())
            assert np.all(out == -7.0) and np.all(out64 == -7.0), (what, name)
        assert call(x=poisoned(np.nan)) == -1 and b"sample 13" in L.speechPlayer_lastError() and b"nan" in L.speechPlayer_lastError().lower(), what
        assert call(x=poisoned(1e30, 199)) == -1 and b"sample 199" in L.speechPlayer_lastError() and b"1e+30" in L.speechPlayer_lastError(), what
        # the bound itself passes, int16 input is not looked at, nothing to read needs no samples
        assert call(x=poisoned(65536.0)) > 0 and call(x=poisoned(-65536.0)) > 0 and call(x=s, inFormat=0) > 0 and L.speechPlayer_lastErrorCode() == 0, what
        out[:] = -7.0
        out64[:] = -7.0
        assert call(x=None, length=0) >= 0 and L.speechPlayer_lastErrorCode() == 0, what
    # sizing without an output
    assert resample(out=None, capacity=0) == -(-200 * 320 // 441) and convolve(out=None, capacity=0) == 215 and convolve(out=None, capacity=0, tail=0) == 200


def test_python_host_functions_refuse_what_they_cannot_take():
    import nvspeechplayer_amd as eng
    h = np.ones(3, np.float32)
    for bad in (np.zeros(10, np.float64), np.zeros(10, np.int32), np.zeros((2, 10), np.float32), [0.5, 0.25], np.zeros(10, np.complex64)):
        for call in (lambda v: eng.signalSpectrogram(v, nFft=64, hop=16), lambda v: eng.signalResample(v, 22050, 16000), lambda v: eng.signalConvolve(v, h)):
            with pytest.raises(TypeError):
                call(bad)
    x = np.zeros(10, np.float32)
    x[4] = np.nan
    for call in (lambda v: eng.signalSpectrogram(v, nFft=64, hop=16), lambda v: eng.signalResample(v, 22050, 16000), lambda v: eng.signalConvolve(v, h)):
        with pytest.raises(RuntimeError, match="sample 4"):
            call(x)
    # the int16-only functions stay as they are
    for call in (lambda v: eng.pcmSpectrogram(v, nFft=64, hop=16), lambda v: eng.pcmResample(v, 22050, 16000), lambda v: eng.pcmConvolve(v, h)):
        with pytest.raises(TypeError):
            call(np.zeros(10, np.float32))


def test_signal_request_checks():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    check = sp.check_signal_request
    t2 = torch.zeros((3, 9), dtype=torch.float32)
    lens = torch.tensor([5, 0, 9], dtype=torch.int64)
    tensor, fmt, n, stride, extent, got = check((t2, lens))
    assert tensor is t2 and (fmt, n, stride) == (1, 3, 9) and extent.dtype == np.int64 and list(extent) == [5, 0, 9] and list(got) == [5, 0, 9]
    t1 = torch.zeros(17, dtype=torch.int16)
    tensor, fmt, n, stride, extent, got = check((t1, np.array([0, 5, 5, 14, 17])))
    assert tensor is t1 and (fmt, n, stride) == (0, 4, 0) and list(extent) == [0, 5, 5, 14, 17] and list(got) == [5, 0, 9, 3]
    assert check((t1, [0, 17]))[2] == 1 and check((t1[:0], [0]))[2] == 0 and check([t2, [1, 2, 3]])[2] == 3
    assert check((torch.zeros((0, 0), dtype=torch.int16), []))[2:4] == (0, 0)
    assert check((torch.zeros((2, 0), dtype=torch.int16), [0, 0]))[2:4] == (2, 0)      # rows of nothing: packed offsets would need three entries
    value = dict(
        lens_short=(t2, [5, 0]), lens_long=(t2, [5, 0, 9, 1]), len_negative=(t2, [5, -1, 9]), len_above=(t2, [5, 10, 9]), offsets_late=(t1, [1, 5, 17]),
        offsets_down=(t1, [0, 6, 5, 17]), offsets_beyond=(t1, [0, 5, 18]), no_offsets=(t1, []), lens_2d=(t2, [[5, 0, 9]]),
        not_contiguous=(t2[:, ::2], [1, 1, 1]), transposed=(t2.t(), [1] * 9), cpu=(t2, lens, 0))
    for name, args in value.items():
        with pytest.raises(ValueError):
            check((args[0], args[1]), *args[2:])
            pytest.fail(name)
    kind = dict(
        not_a_pair=t2, a_triple=(t2, lens, lens), numpy_rows=(np.zeros((3, 9), np.float32), lens), float64=(t2.double(), lens), int32=(t2.int(), lens),
        three_d=(torch.zeros((2, 3, 4)), [1, 1]), scalar=(torch.zeros(()), [0]), real_lens=(t2, [5.0, 0.0, 9.0]), no_second=(t2, None), text=(t2, "abc"))
    for name, signal in kind.items():
        with pytest.raises(TypeError):
            check(signal)
            pytest.fail(name)
    with pytest.raises(ValueError, match="row"):
        check((t2, [5, 10, 9]))


def test_the_reader_under_sanitizers(tmp_path):
    """csrc/klatt_tiles.h's reader and the signal's row table, and the three statements on both input types, in a program of its own,
    tests/native/check_signal.cpp, against brute force under AddressSanitizer + UBSan.  Nothing loaded into python is run under one."""
    exe = str(tmp_path / "check_signal")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_signal.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out
