"""A batch's PCM at another sample rate (include/speechPlayer_batch.h: speechPlayer_batch_exportResampled; BatchPlayer.resampledTensor;
csrc/klatt_resample.h) against the host's statement of the definition, speechPlayer_pcmResample applied to the PCM the engine reads back
-- bit for bit, float32 and int16 -- and, independently of the code the two share, against the numpy float64 sum of
tests/test_resample_host.py within its inner-product bound.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_gpu_spectrogram import bits, player
from tests.test_gpu_timeline import set_host
from tests.test_resample_host import FILTERS, gamma, ratio, reference
from tests.test_stems_host import Stemmed, compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64
POOL_TILE = 32      # an utterance starts on a multiple of this many samples of the pool (klatt_device.h: kTile)

RATES = {"plain": [16000, 24000, 44100, 11025, 22050], "plain16k": [22050, 8000]}


def same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and (np.array_equal(got, want) if got.dtype == np.int16 else np.array_equal(bits(got), bits(want)))


def rows_of(out, second, padded):
    """The rows of an export and (padded) what lies past them."""
    out, second = out.cpu().numpy(), second.numpy()
    if padded:
        return [out[i, :second[i]] for i in range(len(second))], [out[i, second[i]:] for i in range(len(second))]
    return [out[second[i]:second[i + 1]] for i in range(len(second) - 1)], []


def check_every_form(bp, pcm, sr, rate, kw, tag, selection=None):
    """float32 and int16, padded and packed: every row's bits are the statement's, the padding is +0, the lengths are right."""
    import torch
    import nvspeechplayer_amd as eng
    up, down = ratio(sr, rate)
    sel = list(range(len(pcm))) if selection is None else selection
    for dtype, npt in ((torch.float32, np.float32), (torch.int16, np.int16)):
        want = [eng.pcmResample(pcm[u], sr, rate, dtype=npt, **kw) for u in sel]
        for padded in (True, False):
            out, second = bp.resampledTensor(rate, utterances=selection, dtype=dtype, padded=padded, **kw)
            lens = [-(-len(pcm[u]) * up // down) for u in sel]
            assert list(second.numpy()) == (lens if padded else list(np.concatenate([[0], np.cumsum(lens)]))), tag
            assert out.dtype == dtype and out.shape == ((len(sel), max(lens)) if padded else (sum(lens),)), tag
            rows, past = rows_of(out, second, padded)
            for i, (g, w) in enumerate(zip(rows, want)):
                assert same(g, w), (tag, dtype, padded, i, sel[i])
            for i, z in enumerate(past):
                assert not z.view(np.uint32 if npt == np.float32 else np.uint16).any(), (tag, "padding", i)      # +0, on the bit pattern


@pytest.mark.parametrize("name,rate", [(n, r) for n in RATES for r in RATES[n]])
def test_the_device_gives_the_statements_bits(name, rate):
    """The ten-utterance batches at 22 050 and 16 000 Hz, every filter, every form, and a selection with repeats in reverse order."""
    s = compared(name)
    bp, pcm = player(s.b, s.sr)
    assert [len(p) for p in pcm] == [s.length(u) for u in range(s.n)] and any(p.any() for p in pcm)
    for kw in FILTERS:
        check_every_form(bp, pcm, s.sr, rate, kw, (name, rate, kw["zeros"]))
    check_every_form(bp, pcm, s.sr, rate, FILTERS[0], (name, rate, "selection"), selection=[9, 3, 3, 0, 9, 2])
    bp.close()


@pytest.mark.parametrize("name,rate,kw", [("plain", 16000, FILTERS[0]), ("plain", 24000, FILTERS[2]), ("plain", 44100, FILTERS[1]), ("plain", 11025, FILTERS[3]),
                                          ("plain16k", 22050, FILTERS[2]), ("plain16k", 8000, FILTERS[0])])
def test_independent_of_the_shared_code(name, rate, kw):
    """The device's float32 rows within gamma_K sum |x| |h| of the numpy float64 sum over resampleKernel's table."""
    import nvspeechplayer_amd as eng
    s = compared(name)
    bp, pcm = player(s.b, s.sr)
    table, up, down = eng.resampleKernel(s.sr, rate, **kw)
    out, offsets = bp.resampledTensor(rate, padded=False, **kw)
    for u, g in enumerate(rows_of(out, offsets, False)[0]):
        want, mag = reference(pcm[u], table, up, down)
        assert g.shape == want.shape and np.all(np.abs(g.astype(np.float64) - want) <= gamma(table.shape[1]) * mag), u
    bp.close()


def edge_batch(lens):
    """Single-frame utterances of fade 1 and of lens[i] samples (a frame of M >= 2 samples and fade 1 gives M + 1), each between two
    full-length voiced utterances of the plain batch -- utterances 9 and 1, loud at both ends -- so that a read past a row's end would
    pick up signal: -> (batch, the numbers of the short utterances, their neighbours' numbers)."""
    b = compared("plain").b
    voiced = [k for k in range(len(b["frames"])) if not b["isnull"][k]]
    parts = dict(frames=[], min=[], fade=[], index=[], isnull=[])
    start, seeds, short, full = [0], [], [], []

    def neighbour(u):
        k0, k1 = int(b["frame_start"][u]), int(b["frame_start"][u + 1])
        for key in parts:
            parts[key].append(np.asarray(b[key][k0:k1]))
        start.append(start[-1] + k1 - k0)
        seeds.append(int(b["seeds"][u]))
        full.append(len(seeds) - 1)

    for i, L in enumerate(lens):
        assert L >= 3
        neighbour((9, 1)[i % 2])
        parts["frames"].append(np.asarray(b["frames"][voiced[i % len(voiced)]])[None, :])
        parts["min"].append(np.array([L - 1], np.uint32)); parts["fade"].append(np.ones(1, np.uint32))
        parts["index"].append(np.full(1, -1, np.int32)); parts["isnull"].append(np.zeros(1, np.uint8))
        start.append(start[-1] + 1)
        seeds.append(100 + i)
        short.append(len(seeds) - 1)
    neighbour((9, 1)[len(lens) % 2])
    batch = dict(frame_start=np.array(start, np.int64), frames=np.ascontiguousarray(np.concatenate(parts["frames"])),
                 min=np.concatenate(parts["min"]).astype(np.uint32), fade=np.concatenate(parts["fade"]).astype(np.uint32),
                 index=np.concatenate(parts["index"]).astype(np.int32), isnull=np.concatenate(parts["isnull"]).astype(np.uint8),
                 seeds=np.array(seeds, np.uint32))
    return batch, short, full


def export(L, bp, ptr, utterances, rate=16000, zeros=6, rolloff=0.99, window=0, beta=0.0, fmt=1, stride=0, n=None, batch=0, stream=None):
    p = lambda a: None if a is None else a.ctypes.data
    return L.speechPlayer_batch_exportResampled(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, rate, zeros, rolloff,
                                                window, beta, ptr, fmt, stride, stream)


@pytest.mark.parametrize("rate", [16000, 24000, 44100])
def test_edges(rate):
    """Rows whose output lengths are the shortest an utterance gives (an utterance has at least 3 samples; lengths 1 and 2 are the host
    tests'), taps / 2 (shorter than the filter: everything is halo), T - 1, T, T + 1 and 2 T + 3 for T = RESAMPLE_TILE -- or, where the
    ratio skips a length, the lengths either side of it -- between loud neighbours, through the library's entry point into a buffer with
    guards either side, 16-byte aligned and one element past a 16-byte boundary (no aligned run starts at a row's start)."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    sr, T = 22050, sp.RESAMPLE_TILE
    up, down = ratio(sr, rate)
    filters = [FILTERS[0], FILTERS[3]]
    halves = [eng.resampleKernel(sr, rate, **kw)[0].shape[1] // 2 for kw in filters]
    targets = halves + [T - 1, T, T + 1, 2 * T + 3]
    lens = sorted({3, 4} | {max(3, q) for t in targets for q in (t * down // up, -(-t * down // up))})
    outs = [-(-n * up // down) for n in lens]
    for t in targets:
        assert t in outs or (up > down and any(o < t for o in outs) and any(o > t for o in outs)), (t, outs)
    assert rate != 16000 or set(targets) <= set(outs)
    batch, short, full = edge_batch(lens)
    assert [Stemmed(batch).length(u) for u in short] == lens
    bp, pcm = player(batch, sr)
    assert [len(pcm[u]) for u in short] == lens
    reach = max(halves) - (POOL_TILE - 1)      # samples of a neighbour within the widest filter's reach of a short row, whatever the padding between
    assert reach >= 30
    for u in full:      # the neighbours' PCM is non-zero next to the short rows in the pool
        assert pcm[u][:reach].any() and pcm[u][-reach:].any(), u
    sel = np.array(short + [full[0], short[0]], np.int64)
    for kw in filters:
        win = dict(zeros=kw["zeros"], window=sp.RESAMPLE_WINDOWS.index(kw["window"]), beta=kw.get("beta", 0.0))
        for fmt, dtype, npt in ((1, torch.float32, np.float32), (0, torch.int16, np.int16)):
            want = [eng.pcmResample(pcm[u], sr, rate, dtype=npt, **kw) for u in sel]
            most = max(len(w) for w in want)
            for stride in (0, most, most + 3):
                elements = sum(len(w) for w in want) if stride == 0 else len(sel) * stride
                for shift in (0, 1):
                    buf = torch.full((elements + 2 * GUARD + 1,), -7, dtype=dtype, device="cuda:%d" % bp.device)
                    assert buf.data_ptr() % 16 == 0
                    assert export(L, bp, buf.data_ptr() + (GUARD + shift) * buf.element_size(), sel, rate=rate, fmt=fmt, stride=stride, **win) == elements
                    torch.cuda.synchronize()
                    got = buf.cpu().numpy()
                    tag = (rate, kw["zeros"], fmt, stride, shift)
                    assert np.all(got[:GUARD + shift] == -7) and np.all(got[GUARD + shift + elements:] == -7), tag
                    got = got[GUARD + shift:GUARD + shift + elements]
                    at = 0
                    for i, w in enumerate(want):
                        span = len(w) if stride == 0 else stride
                        assert same(got[at:at + len(w)], w), tag + (i,)
                        assert not got[at + len(w):at + span].view(np.uint32 if fmt else np.uint16).any(), tag + (i, "padding")
                        at += span
    bp.close()


def test_a_tile_in_spans():
    """22 050 to 2 205 Hz: ten inputs per output, so a tile's inputs do not fit the kernel's LDS at once and the tile proceeds in spans
    (787 outputs with 16 zeros, 815 with 2).  One utterance of 20 000 samples gives 2 000 outputs: two tiles, each in two spans."""
    from nvspeechplayer_amd import speechPlayer as sp
    batch, short, full = edge_batch([20000])
    bp, pcm = player(batch)
    assert len(pcm[short[0]]) == 20000 and 2000 > sp.RESAMPLE_TILE + 815
    for kw in (FILTERS[1], FILTERS[2]):
        check_every_form(bp, pcm, 22050, 2205, kw, ("spans", kw["zeros"]))
    bp.close()


def test_mode_fast():
    """A MODE_FAST player's export is the statement applied to that player's own PCM."""
    s = compared("plain")
    bp, pcm = player(s.b, s.sr, mode=1)
    check_every_form(bp, pcm, s.sr, 16000, FILTERS[0], "fast")
    check_every_form(bp, pcm, s.sr, 44100, FILTERS[2], "fast")
    bp.close()


def test_ordering():
    """An export on a side stream right behind synthesize(wait=False); then, with no host wait, the next launch and a second export
    with other parameters, which replaces the table the first one reads; one synchronise, and both are right.  Then the same
    parameters again (the table is kept), and the refusal after a set call."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("plain")
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.resampledTensor(16000)
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT
    side = torch.cuda.Stream(bp.device)
    first, second, third = dict(rate=16000, **FILTERS[3]), dict(rate=24000, **FILTERS[0]), dict(rate=24000, **FILTERS[0])
    bp.synthesize(wait=False)
    with torch.cuda.stream(side):
        a, la = bp.resampledTensor(padded=False, **first)
    bp.synthesize(wait=False)      # the next launch waits for the export on the device (and writes the same PCM)
    with torch.cuda.stream(side):
        b, lb = bp.resampledTensor(padded=False, **second)
    c, lc = bp.resampledTensor(padded=False, dtype=torch.int16, **third)      # (on the default stream: behind the upload on the side stream)
    torch.cuda.synchronize()
    pcm = [bp.read(u) for u in range(s.n)]
    for out, offsets, kw, npt in ((a, la, first, np.float32), (b, lb, second, np.float32), (c, lc, third, np.int16)):
        kw = dict(kw)
        rate = kw.pop("rate")
        for u, g in enumerate(rows_of(out, offsets, False)[0]):
            assert same(g, eng.pcmResample(pcm[u], s.sr, rate, dtype=npt, **kw)), (rate, u)
    set_host(bp, s.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.resampledTensor(16000)
    bp.close()


def test_refusals_write_nothing_and_leave_the_batch_usable():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("plain")
    utt = np.arange(s.n, dtype=np.int64)
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    lens = [-(-s.length(u) * 320 // 441) for u in range(s.n)]
    most, total = max(lens), sum(lens)
    out = torch.full((s.n * most + 8,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel = out.clone()
    host = np.zeros(s.n * most, np.float32)
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        a = dict(ptr=out.data_ptr(), utterances=utt, fmt=1, stride=most)
        a.update(kw)
        return export(L, bp, a.pop("ptr"), a.pop("utterances"), **a)

    def refused(name, **kw):
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportResampled" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), name

    refused("not synthesised since it was set")
    bp.synthesize()
    pcm = [bp.read(u).copy() for u in range(s.n)]
    seg = next(g for g in torch.cuda.memory_snapshot() if g["address"] <= out.data_ptr() < g["address"] + g["total_size"])
    one_short = seg["address"] + seg["total_size"] - 4 * (total - 1)
    assert one_short >= seg["address"]
    cases = dict(
        no_batch=dict(batch=None), rate_zero=dict(rate=0), rate_negative=dict(rate=-16000), zeros_zero=dict(zeros=0), zeros_negative=dict(zeros=-1),
        rolloff_zero=dict(rolloff=0.0), rolloff_above_one=dict(rolloff=1.5), rolloff_nan=dict(rolloff=nan), rolloff_inf=dict(rolloff=inf),
        window_2=dict(window=2), window_negative=dict(window=-1), beta_negative=dict(window=1, beta=-1.0), beta_nan=dict(window=1, beta=nan),
        beta_inf=dict(window=1, beta=inf), up_above_4096=dict(rate=22051), taps_above_1024=dict(zeros=372), table_above_2_20=dict(rate=22040, zeros=250),
        format_2=dict(fmt=2), format_negative=dict(fmt=-1), utterance_beyond=dict(utterances=np.array([0, s.n], np.int64)),
        utterance_negative=dict(utterances=np.array([-1], np.int64)), negative_count=dict(n=-1), stride_short=dict(stride=most - 1),
        stride_negative=dict(stride=-1), host_memory=dict(ptr=host.ctypes.data), no_buffer=dict(ptr=None), misaligned_float=dict(ptr=out.data_ptr() + 2),
        misaligned_int16=dict(ptr=out.data_ptr() + 1, fmt=0), too_small=dict(stride=1 << 34), too_small_packed=dict(stride=0, ptr=one_short))
    for name, kw in cases.items():
        refused(name, **kw)
    # nothing to write needs no buffer
    assert export(L, bp, None, utt[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    # the batch is as usable as before
    assert call() == s.n * most
    torch.cuda.synchronize()
    got = out[:s.n * most].view(s.n, most).cpu().numpy()
    for u in range(s.n):
        w = eng.pcmResample(pcm[u], s.sr, 16000)
        assert same(got[u, :len(w)], w) and not bits(got[u, len(w):]).any(), u
    assert torch.equal(out[s.n * most:], sentinel[s.n * most:])
    # equal rates: speechPlayer_batch_exportPcm's output exactly
    for dtype in (torch.float32, torch.int16):
        a, la = bp.resampledTensor(s.sr, dtype=dtype)
        b, lb = bp.pcmTensor(dtype=dtype)
        assert torch.equal(la, lb) and torch.equal(a, b)
    bp.synthesize()
    assert all(np.array_equal(bp.read(u), pcm[u]) for u in range(s.n))
    bp.close()
