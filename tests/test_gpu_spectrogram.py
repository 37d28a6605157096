"""The STFT / band spectrogram of a batch's PCM (include/speechPlayer_batch.h: speechPlayer_batch_exportSpectrogram;
BatchPlayer.spectrogramTensor; csrc/klatt_spectrum.h) against the host's statement of the definition, speechPlayer_pcmSpectrogram applied to
the PCM the engine reads back -- bit for bit on every linear value, within 4 ulp through the logarithm -- and, independently of the code
the two share, against numpy's float64 rfft within the bound of tests/test_spectrogram_host.py.  Needs a GPU."""
import math

import numpy as np
import pytest

from tests.test_gpu_timeline import set_host
from tests.test_spectrogram_host import SIZES, check_against_rfft, ulps
from tests.test_stems_host import compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64


def short_batch(n):
    """Three hand-made utterances of 3 (the shortest a frame can be: max(M, F + 1) + 1 with F >= 1), n / 2 and n + 3 samples, from voiced
    frames of the plain batch: one frame, and twice a frame of 3 samples and one of the rest, with abrupt fades."""
    b = compared("plain").b
    voiced = [k for k in range(len(b["frames"])) if not b["isnull"][k]][:5]
    lens = [3, n // 2, n + 3]
    mins = [0, 2, n // 2 - 4, 2, n + 3 - 4]
    assert [3, 3 + mins[2] + 1, 3 + mins[4] + 1] == lens
    return dict(frame_start=np.array([0, 1, 3, 5], np.int64), frames=np.ascontiguousarray(b["frames"][voiced]), min=np.array(mins, np.uint32),
                fade=np.ones(5, np.uint32), index=np.full(5, -1, np.int32), isnull=np.zeros(5, np.uint8), seeds=np.array([1, 2, 3], np.uint32)), lens


def player(batch, sr=22050, mode=0):
    """A player with the batch synthesised, and every utterance's PCM as the engine reads it back."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(sr, mode=mode)
    set_host(bp, batch)
    bp.synthesize()
    return bp, [bp.read(u).copy() for u in range(bp.nUtterances)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def rows_of(out, second, padded):
    """The rows of an export, each [steps, bands], and (padded) what lies past them."""
    out, second = out.cpu().numpy(), second.numpy()
    if padded:
        return [out[i, :second[i]] for i in range(len(second))], [out[i, second[i]:] for i in range(len(second))]
    return [out[second[i]:second[i + 1]] for i in range(len(second) - 1)], []


def check_every_form(bp, pcm, n, hop, phase, banks, tag):
    """power 1 and 2, every bank, float64 and float32, padded and packed: the device's bits are the statement's; then the logarithm."""
    import torch
    import nvspeechplayer_amd as eng
    for power in (1, 2):
        for bank in banks:
            kw = dict(nFft=n, hop=hop, phase=phase, bank=bank, power=power)
            want = [eng.pcmSpectrogram(p, **kw) for p in pcm]
            for dtype, npt in ((torch.float64, np.float64), (torch.float32, np.float32)):
                for padded in (True, False):
                    out, second = bp.spectrogramTensor(dtype=dtype, padded=padded, **kw)
                    rows, past = rows_of(out, second, padded)
                    assert len(rows) == len(want), tag
                    for u, (g, w) in enumerate(zip(rows, want)):
                        assert g.shape == w.shape and np.array_equal(bits(g), bits(w.astype(npt))), (tag, power, None if bank is None else len(bank), dtype, padded, u)
                    for u, z in enumerate(past):
                        assert not bits(z).any(), (tag, "padding", u)      # +0, on the bit pattern
            for log, floor in ((("db", 1e-10),) if power == 2 else (("ln", 1e-5),)):
                lw = [eng.pcmSpectrogram(p, log=log, floor=floor, **kw) for p in pcm]
                out, second = bp.spectrogramTensor(dtype=torch.float64, padded=False, log=log, floor=floor, **kw)
                for u, (g, w) in enumerate(zip(rows_of(out, second, False)[0], lw)):
                    assert g.shape == w.shape and (g.size == 0 or ulps(g, w).max() <= 4), (tag, "log", power, log, u)
                out, second = bp.spectrogramTensor(dtype=torch.float32, padded=True, log=log, floor=floor, **kw)
                rows, past = rows_of(out, second, True)
                for u, (g, w) in enumerate(zip(rows, lw)):      # two binary64 values 4 ulp apart round to float32 values at most one float32 ulp apart
                    w32 = w.astype(np.float32)
                    assert g.shape == w.shape and np.all(np.abs(g.astype(np.float64) - w32) <= np.spacing(np.abs(w32)).astype(np.float64)), (tag, "log32", u)
                for z in past:
                    assert not bits(z).any(), (tag, "log padding")


def banks_for(sr, n):
    import nvspeechplayer_amd as eng
    return [None, eng.melFilterbank(sr, n, 8), eng.melFilterbank(sr, n, 80, norm="slaney")]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["plain", "plain16k"])
def test_the_device_gives_the_statements_bits(name, n):
    """The ten-utterance batches at 22 050 and 16 000 Hz: hop 100, n / 4 and n + 5, phase 0 and 37, every form."""
    s = compared(name)
    bp, pcm = player(s.b, s.sr)
    assert [len(p) for p in pcm] == [s.length(u) for u in range(s.n)] and any(p.any() for p in pcm)
    for hop in (100, n // 4, n + 5):
        for phase in (0, 37):
            check_every_form(bp, pcm, n, hop, phase, banks_for(s.sr, n), (name, n, hop, phase))
    bp.close()


@pytest.mark.parametrize("phase", [0, 37])
@pytest.mark.parametrize("hop", ["1", "100", "n/4", "n+5"])
@pytest.mark.parametrize("n", SIZES)
def test_three_short_utterances(n, hop, phase):
    """Utterances of 3, n / 2 and n + 3 samples (shorter than, half of and just over a frame), hop 1 included."""
    batch, lens = short_batch(n)
    bp, pcm = player(batch)
    assert [len(p) for p in pcm] == lens
    hop = {"1": 1, "100": 100, "n/4": n // 4, "n+5": n + 5}[hop]
    check_every_form(bp, pcm, n, hop, phase, banks_for(22050, n), ("short", n, hop, phase))
    bp.close()


@pytest.mark.parametrize("name", ["plain", "plain16k"])
def test_independent_of_the_shared_code(name):
    """nFft 1024, power 1: the device's magnitudes within B + 4 u |X_k| of numpy's float64 rfft of the engine's PCM."""
    import torch
    s = compared(name)
    bp, pcm = player(s.b, s.sr)
    for hop, phase in ((256, 0), (100, 37)):
        out, offsets = bp.spectrogramTensor(nFft=1024, hop=hop, phase=phase, power=1, dtype=torch.float64, padded=False)
        for u, g in enumerate(rows_of(out, offsets, False)[0]):
            check_against_rfft(g, pcm[u], 1024, hop, phase)
    bp.close()


def test_ordering():
    """An export on a side stream right behind synthesize(wait=False), no host wait between; the same after a switch to MODE_FAST; and
    the refusal before any synthesis after a set call."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("plain")
    bank = eng.melFilterbank(s.sr, 256, 8)
    kw = dict(nFft=256, hop=64, phase=3, bank=bank, power=2)
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.spectrogramTensor(**kw)
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT
    side = torch.cuda.Stream(bp.device)
    for mode in (0, 1):
        bp.setOption("mode", mode)
        bp.synthesize(wait=False)
        with torch.cuda.stream(side):
            out, offsets = bp.spectrogramTensor(dtype=torch.float64, padded=False, **kw)
        bp.synthesize(wait=False)      # the next launch waits for the export on the device (and writes the same PCM)
        side.synchronize()
        bp.wait()
        pcm = [bp.read(u) for u in range(s.n)]
        for u, g in enumerate(rows_of(out, offsets, False)[0]):
            assert np.array_equal(bits(g), bits(eng.pcmSpectrogram(pcm[u], **kw))), (mode, u)
    # a set call makes the PCM stale again
    set_host(bp, s.b)
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.spectrogramTensor(**kw)
    bp.close()


def export(L, bp, ptr, utterances, fmt=0, stride=0, n=None, nfft=64, hop=16, phase=0, window=None, bank=None, nbands=0, power=2, scale=0.0, floor=0.0,
           batch=0):
    p = lambda a: None if a is None else a.ctypes.data
    return L.speechPlayer_batch_exportSpectrogram(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, nfft, hop, phase,
                                                  p(window), p(bank), nbands, power, scale, floor, ptr, fmt, stride, None)


def test_selection_and_buffer_safety():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    kw = dict(nFft=64, hop=16, phase=900, power=2)
    full, steps = bp.spectrogramTensor(dtype=torch.float64, **kw)
    pick, psteps = bp.spectrogramTensor(dtype=torch.float64, utterances=[3, 0, 3], **kw)
    assert list(psteps.numpy()) == [int(steps[3]), int(steps[0]), int(steps[3])]
    for i, u in enumerate((3, 0, 3)):
        assert torch.equal(pick[i, :int(steps[u])].view(torch.int64), full[u, :int(steps[u])].view(torch.int64)), i
        assert not pick[i, int(steps[u]):].view(torch.int64).any()
    # utterances 8 and 9 (876 and 840 samples) end at or before the phase: no steps; nothing to write needs no buffer
    assert int(steps[8]) == 0 and int(steps[9]) == 0 and int(steps[0]) == math.ceil((1221 - 900) / 16)
    none = np.array([9, 8], np.int64)
    assert export(L, bp, None, none, phase=900) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert export(L, bp, None, none[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    out, second = bp.spectrogramTensor(utterances=[9, 8], padded=False, **kw)
    assert out.shape == (0, 33) and list(second.numpy()) == [0, 0, 0]
    # guards: 64 elements behind the output keep their pattern, aligned and misaligned by one element (the element-by-element stores)
    sel = np.array([4, 9, 1], np.int64)
    want = [eng.pcmSpectrogram(pcm[u], **kw) for u in sel]
    most = max(len(w) for w in want)
    for fmt, dtype, npt in ((0, torch.float64, np.float64), (1, torch.float32, np.float32)):
        for stride in (0, most + 1):
            elements = (sum(len(w) for w in want) if stride == 0 else len(sel) * stride) * 33
            for shift in (0, 1):
                buf = torch.full((elements + GUARD + 1,), -7.0, dtype=dtype, device="cuda:%d" % bp.device)
                assert export(L, bp, buf.data_ptr() + shift * buf.element_size(), sel, fmt=fmt, stride=stride, phase=900) == elements, (fmt, stride, shift)
                torch.cuda.synchronize()
                got = buf.cpu().numpy()
                assert np.all(got[:shift] == -7.0) and np.all(got[shift + elements:] == -7.0), (fmt, stride, shift)
                got = got[shift:shift + elements].reshape(-1, 33)
                at = 0
                for i, w in enumerate(want):
                    span = len(w) if stride == 0 else stride
                    assert np.array_equal(bits(got[at:at + len(w)]), bits(w.astype(npt))), (fmt, stride, shift, i)
                    assert not bits(got[at + len(w):at + span]).any()
                    at += span
    bp.close()


def test_refusals_write_nothing_and_leave_the_batch_usable():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    utt = np.arange(s.n, dtype=np.int64)
    counts = np.array([math.ceil(len(p) / 16) for p in pcm])
    most, total = int(counts.max()), int(counts.sum())
    out = torch.full((s.n * most * 33 + 4,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel = out.clone()
    host = np.zeros(s.n * most * 33, np.float32)
    bank = np.ones((3, 33))
    nan, inf = float("nan"), float("inf")
    seg = next(g for g in torch.cuda.memory_snapshot() if g["address"] <= out.data_ptr() < g["address"] + g["total_size"])
    one_short = seg["address"] + seg["total_size"] - 4 * (total * 33 - 1)
    assert one_short >= seg["address"]

    def call(**kw):
        a = dict(ptr=out.data_ptr(), utterances=utt, fmt=1, stride=most)
        a.update(kw)
        return export(L, bp, a.pop("ptr"), a.pop("utterances"), **a)

    refused = dict(
        no_batch=dict(batch=None), nfft_32=dict(nfft=32), nfft_8192=dict(nfft=8192), nfft_96=dict(nfft=96), nfft_negative=dict(nfft=-64),
        hop_zero=dict(hop=0), hop_negative=dict(hop=-16), phase_negative=dict(phase=-1), power_0=dict(power=0), power_3=dict(power=3),
        bands_zero=dict(bank=bank, nbands=0), bands_negative=dict(bank=bank, nbands=-1),
        window_nan=dict(window=np.where(np.arange(64) == 63, nan, 1.0)), window_inf=dict(window=np.where(np.arange(64) == 0, inf, 1.0)),
        bank_nan=dict(bank=np.where(np.arange(33) == 32, nan, bank), nbands=3), bank_inf=dict(bank=np.where(np.arange(33) == 0, -inf, bank), nbands=3),
        floor_zero=dict(scale=10.0, floor=0.0), floor_negative=dict(scale=10.0, floor=-1e-10), floor_nan=dict(scale=10.0, floor=nan),
        scale_nan=dict(scale=nan, floor=1.0), scale_inf=dict(scale=inf, floor=1.0), floor_inf=dict(floor=inf),
        format_2=dict(fmt=2), format_negative=dict(fmt=-1), utterance_beyond=dict(utterances=np.array([0, s.n], np.int64)),
        utterance_negative=dict(utterances=np.array([-1], np.int64)), negative_count=dict(n=-1), stride_short=dict(stride=most - 1),
        stride_negative=dict(stride=-1), host_memory=dict(ptr=host.ctypes.data), no_buffer=dict(ptr=None), misaligned=dict(ptr=out.data_ptr() + 2),
        too_small=dict(stride=1 << 34), too_small_packed=dict(stride=0, ptr=one_short),
        misaligned_f64=dict(ptr=out.data_ptr() + 4, fmt=0, utterances=utt[:1], stride=0))
    for name, kw in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportSpectrogram" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), name
    # the batch is as usable as before
    assert call() == s.n * most * 33
    torch.cuda.synchronize()
    got = out[:s.n * most * 33].view(s.n, most, 33).cpu().numpy()
    for u in range(s.n):
        w = eng.pcmSpectrogram(pcm[u], nFft=64, hop=16).astype(np.float32)
        assert np.array_equal(bits(got[u, :len(w)]), bits(w)) and not bits(got[u, len(w):]).any(), u
    assert torch.equal(out[s.n * most * 33:], sentinel[s.n * most * 33:])
    bp.synthesize()
    assert all(np.array_equal(bp.read(u), pcm[u]) for u in range(s.n))
    bp.close()
