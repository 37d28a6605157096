"""A batch's PCM convolved with impulse responses (include/speechPlayer_batch.h: speechPlayer_batch_exportConvolved;
BatchPlayer.convolvedTensor; csrc/klatt_convolve.h) against the host's statement of the definition, speechPlayer_pcmConvolve applied to the
PCM the engine reads back -- bit for bit, float32 and int16 -- and, independently of the code the two share, against numpy's float64
convolution within the inner-product bound of tests/test_convolve_host.py.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_convolve_host import decaying, gamma, reference
from tests.test_gpu_resample import edge_batch, rows_of, same
from tests.test_gpu_spectrogram import bits, player
from tests.test_gpu_timeline import set_host
from tests.test_stems_host import Stemmed, compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64


def sizes():
    from nvspeechplayer_amd import speechPlayer as sp
    return sp.CONVOLVE_TILE, sp.CONVOLVE_BLOCK


def eight():
    """Eight seeded, exponentially decaying responses of 1, 2, 3, 5, B - 1, B, B + 1 and 2 B + 3 taps."""
    T, B = sizes()
    return [decaying(K, i) for i, K in enumerate((1, 2, 3, 5, B - 1, B, B + 1, 2 * B + 3))]


class Statement:
    """The host's statement per (utterance, response, dtype), computed once with its tail; tail = 0 is its first L values."""
    def __init__(self, pcm, irs):
        self.pcm, self.irs, self.done = pcm, irs, {}

    def __call__(self, u, j, npt, tail):
        import nvspeechplayer_amd as eng
        key = (u, j, npt)
        if key not in self.done:
            self.done[key] = eng.pcmConvolve(self.pcm[u], self.irs[j], tail=True, dtype=npt)
        return self.done[key] if tail else self.done[key][:len(self.pcm[u])]


def check_every_form(bp, want, irs, sel, irOf, tag):
    """float32 and int16, padded and packed, tail 0 and 1: every row's bits are the statement's, the padding is +0 on its bit pattern, the
    lengths and offsets are as defined."""
    import torch
    for dtype, npt in ((torch.float32, np.float32), (torch.int16, np.int16)):
        for tail in (True, False):
            rows_want = [want(u, j, npt, tail) for u, j in zip(sel, irOf)]
            lens = [len(want.pcm[u]) + (len(irs[j]) - 1 if tail else 0) for u, j in zip(sel, irOf)]
            assert [len(w) for w in rows_want] == lens
            for padded in (True, False):
                out, second = bp.convolvedTensor(irs, irOf=irOf, tail=tail, utterances=sel, dtype=dtype, padded=padded)
                assert list(second.numpy()) == (lens if padded else list(np.concatenate([[0], np.cumsum(lens)]))), tag
                assert out.dtype == dtype and out.shape == ((len(sel), max(lens)) if padded else (sum(lens),)), tag
                rows, past = rows_of(out, second, padded)
                for i, (g, w) in enumerate(zip(rows, rows_want)):
                    assert same(g, w), (tag, dtype, tail, padded, i, sel[i], irOf[i])
                for i, z in enumerate(past):
                    assert not z.view(np.uint32 if npt == np.float32 else np.uint16).any(), (tag, "padding", i)


def longest_to_shortest(pcm, n):
    """Response numbers for the utterances, cycled: the longest utterance takes response 0 (the shortest response), and so on."""
    order = np.argsort([-len(p) for p in pcm], kind="stable")
    of = np.zeros(len(pcm), np.int64)
    of[order] = np.arange(len(pcm)) % n
    return [int(j) for j in of]


@pytest.mark.parametrize("name", ["plain", "plain16k"])
def test_the_device_gives_the_statements_bits(name):
    """The ten-utterance batches at 22 050 and 16 000 Hz, the eight responses cycled over the rows (and cycled on by three, so that every
    utterance meets a short and a long one), every form; and a selection with repeats, a different response on each repeat."""
    s = compared(name)
    bp, pcm = player(s.b, s.sr)
    assert [len(p) for p in pcm] == [s.length(u) for u in range(s.n)] and any(p.any() for p in pcm)
    irs = eight()
    want = Statement(pcm, irs)
    irOf = longest_to_shortest(pcm, len(irs))
    check_every_form(bp, want, irs, list(range(s.n)), irOf, (name, "cycled"))
    check_every_form(bp, want, irs, list(range(s.n)), [(j + 3) % len(irs) for j in irOf], (name, "cycled on"))
    check_every_form(bp, want, irs, [9, 3, 3, 0, 9, 2], [7, 6, 1, 4, 0, 5], (name, "selection"))
    # one response for every row needs no irOf
    out, lens = bp.convolvedTensor(irs[4], padded=False)
    for u, g in enumerate(rows_of(out, lens, False)[0]):
        assert same(g, want(u, 4, np.float32, True)), u
    bp.close()


@pytest.mark.parametrize("name", ["plain", "plain16k"])
def test_independent_of_the_shared_code(name):
    """The device's float32 rows within gamma_K conv(|x|, |h|) of numpy's float64 convolution."""
    s = compared(name)
    bp, pcm = player(s.b, s.sr)
    irs = eight()
    for shift in (0, 3):
        irOf = [(j + shift) % len(irs) for j in longest_to_shortest(pcm, len(irs))]
        for tail in (True, False):
            out, offsets = bp.convolvedTensor(irs, irOf=irOf, tail=tail, padded=False)
            for u, g in enumerate(rows_of(out, offsets, False)[0]):
                w, mag = reference(pcm[u], irs[irOf[u]], tail)
                assert g.shape == w.shape and np.all(np.abs(g.astype(np.float64) - w) <= gamma(len(irs[irOf[u]])) * mag), (shift, tail, u)
    bp.close()


def export(L, bp, ptr, utterances, ir, start, irOf, tail=1, fmt=1, stride=0, n=None, nIr=None, batch=0, stream=None):
    p = lambda a: None if a is None else a.ctypes.data
    return L.speechPlayer_batch_exportConvolved(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, p(ir), p(start),
                                                len(start) - 1 if nIr is None else nIr, p(irOf), tail, ptr, fmt, stride, stream)


def test_edges():
    """Utterances of 3, 4, 5, T - 1, T, T + 1, 2 T - 1 and 2 T + 1 samples between loud neighbours, each against responses of 1, 4, 5 and
    B + 1 taps (K > L, and L + K - 1 landing on T and T + 1, among them), through the library's entry point into a buffer with guards either
    side, 16-byte aligned and one element past a 16-byte boundary, both tails, packed and two padded widths, both dtypes."""
    import torch
    from nvspeechplayer_amd import _native
    L = _native.load()
    T, B = sizes()
    lens = [3, 4, 5, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1]
    taps = [1, 4, 5, B + 1]
    assert any(n + k - 1 == T for n in lens for k in taps) and any(n + k - 1 == T + 1 for n in lens for k in taps) and any(k > n for n in lens for k in taps)
    batch, short, full = edge_batch(lens)
    assert [Stemmed(batch).length(u) for u in short] == lens
    bp, pcm = player(batch)
    assert [len(pcm[u]) for u in short] == lens
    for u in full:      # the neighbours' PCM is non-zero next to the short rows in the pool
        assert pcm[u][:200].any() and pcm[u][-200:].any(), u
    irs = [decaying(K, 30 + K) for K in taps]
    want = Statement(pcm, irs)
    flat, start = np.concatenate(irs), np.concatenate([[0], np.cumsum(taps)]).astype(np.int64)
    sel = np.array([u for u in short for _ in taps] + [full[0], short[0]], np.int64)
    irOf = np.array([j for _ in short for j in range(len(taps))] + [1, 3], np.int64)
    for fmt, dtype, npt in ((1, torch.float32, np.float32), (0, torch.int16, np.int16)):
        for tail in (1, 0):
            rows = [want(int(u), int(j), npt, tail) for u, j in zip(sel, irOf)]
            most = max(len(w) for w in rows)
            for stride in (0, most, most + 3):
                elements = sum(len(w) for w in rows) if stride == 0 else len(sel) * stride
                for shift in (0, 1):
                    buf = torch.full((elements + 2 * GUARD + 1,), -7, dtype=dtype, device="cuda:%d" % bp.device)
                    assert buf.data_ptr() % 16 == 0
                    assert export(L, bp, buf.data_ptr() + (GUARD + shift) * buf.element_size(), sel, flat, start, irOf, tail=tail, fmt=fmt, stride=stride) == elements
                    torch.cuda.synchronize()
                    got = buf.cpu().numpy()
                    tag = (fmt, tail, stride, shift)
                    assert np.all(got[:GUARD + shift] == -7) and np.all(got[GUARD + shift + elements:] == -7), tag
                    got = got[GUARD + shift:GUARD + shift + elements]
                    at = 0
                    for i, w in enumerate(rows):
                        span = len(w) if stride == 0 else stride
                        assert same(got[at:at + len(w)], w), tag + (i, int(sel[i]), int(irOf[i]))
                        assert not got[at + len(w):at + span].view(np.uint32 if fmt else np.uint16).any(), tag + (i, "padding")
                        at += span
    bp.close()


def test_identity_and_delay():
    """h = [1.0] is pcmTensor in both dtypes; a delay of B + 1 samples (and of 2 B + 1) is the shifted PCM: the later
    tap blocks lie wholly outside the signal at a row's start, the first at the end of its tail, so both ends of a row skip blocks."""
    import torch
    T, B = sizes()
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    assert min(len(p) for p in pcm) + B < 2 * T      # (the shortest rows' third tile lies past the first block's reach: skipped at 2 B + 1)
    for dtype in (torch.float32, torch.int16):
        for padded in (True, False):
            a, la = bp.pcmTensor(dtype=dtype, padded=padded)
            for tail in (True, False):
                b, lb = bp.convolvedTensor(np.ones(1, np.float32), tail=tail, dtype=dtype, padded=padded)
                assert torch.equal(la, lb) and torch.equal(a, b), (dtype, padded, tail)
        a, la = bp.pcmTensor(dtype=dtype)
        for d in (B + 1, 2 * B + 1):
            delay = np.zeros(d + 1, np.float32)
            delay[d] = 1.0
            b, lb = bp.convolvedTensor(delay, dtype=dtype)
            assert torch.equal(lb, la + d) and not b[:, :d].any() and torch.equal(b[:, d:], a), (dtype, d)
            c, lc = bp.convolvedTensor(delay, dtype=dtype, tail=False)
            assert torch.equal(lc, la)
            for u in range(s.n):
                assert torch.equal(c[u, :la[u]], b[u, :la[u]]) and not c[u, la[u]:].any(), (dtype, d, u)
    bp.close()


def test_subnormal_responses():
    """Responses scaled by 2^-130: every product is subnormal, and the device keeps them as the host does."""
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    irs = [h * np.float32(2.0 ** -130) for h in eight()[2:7]]
    irOf = longest_to_shortest(pcm, len(irs))
    out, offsets = bp.convolvedTensor(irs, irOf=irOf, padded=False)
    want = Statement(pcm, irs)
    rows = rows_of(out, offsets, False)[0]
    for u, g in enumerate(rows):
        assert same(g, want(u, irOf[u], np.float32, True)), u
    every = np.concatenate(rows)
    assert np.count_nonzero(every) > every.size // 2 and np.abs(every).max() < 2.0 ** -126      # subnormal, and not flushed
    bp.close()


def test_mode_fast():
    """A MODE_FAST player's export is the statement applied to that player's own PCM."""
    s = compared("plain")
    bp, pcm = player(s.b, s.sr, mode=1)
    irs = eight()
    check_every_form(bp, Statement(pcm, irs), irs, list(range(s.n)), longest_to_shortest(pcm, len(irs)), "fast")
    bp.close()


def test_ordering():
    """An export on a side stream right behind synthesize(wait=False); then, with no host wait, the batch is set to other content and
    synthesised again: the exported tensor still holds the first content.  Then sixteen exports in flight, and the refusal after a set
    call."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("plain")
    irs = eight()
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.convolvedTensor(irs[3])
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT
    batch, short, full = edge_batch([700, 50])
    side = torch.cuda.Stream(bp.device)
    bp.synthesize(wait=False)
    irOf = [u % len(irs) for u in range(s.n)]
    with torch.cuda.stream(side):
        a, la = bp.convolvedTensor(irs, irOf=irOf, padded=False)
    set_host(bp, batch)      # other content: the set call and the next launch wait for the export on the device
    bp.synthesize(wait=False)
    with torch.cuda.stream(side):
        b, lb = bp.convolvedTensor(irs[6], padded=False, dtype=torch.int16)
    torch.cuda.synchronize()
    second = [bp.read(u).copy() for u in range(bp.nUtterances)]
    for u, g in enumerate(rows_of(b, lb, False)[0]):
        assert same(g, eng.pcmConvolve(second[u], irs[6], dtype=np.int16)), u
    set_host(bp, s.b)
    bp.synthesize()
    first = [bp.read(u).copy() for u in range(s.n)]
    for u, g in enumerate(rows_of(a, la, False)[0]):
        assert same(g, eng.pcmConvolve(first[u], irs[irOf[u]])), u
    # sixteen exports in flight (every slot), and one more
    outs = [bp.convolvedTensor(irs[i % 8], tail=bool(i % 2), padded=False) for i in range(17)]
    torch.cuda.synchronize()
    for i, (out, offsets) in enumerate(outs):
        for u, g in enumerate(rows_of(out, offsets, False)[0]):
            assert same(g, eng.pcmConvolve(first[u], irs[i % 8], tail=bool(i % 2))), (i, u)
    set_host(bp, s.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.convolvedTensor(irs[3])
    bp.close()


def test_refusals_write_nothing_and_leave_the_batch_usable():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    s = compared("plain")
    utt = np.arange(s.n, dtype=np.int64)
    bp = eng.BatchPlayer(s.sr)
    set_host(bp, s.b)
    irs = [decaying(5, 1), decaying(40, 2)]
    flat, start = np.concatenate(irs), np.array([0, 5, 45], np.int64)
    irOf = (utt % 2).astype(np.int64)
    lens = [s.length(u) + len(irs[u % 2]) - 1 for u in range(s.n)]
    most, total = max(lens), sum(lens)
    out = torch.full((s.n * most + 8,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel = out.clone()
    host = np.zeros(s.n * most, np.float32)
    big = np.full(sp.CONVOLVE_MAX_TABLE + 1, 0.5, np.float32)
    steps = np.arange(0, sp.CONVOLVE_MAX_TABLE + 1, sp.CONVOLVE_MAX_TAPS).astype(np.int64)

    def call(**kw):
        a = dict(ptr=out.data_ptr(), utterances=utt, ir=flat, start=start, irOf=irOf, fmt=1, stride=most)
        a.update(kw)
        return export(L, bp, a.pop("ptr"), a.pop("utterances"), a.pop("ir"), a.pop("start"), a.pop("irOf"), **a)

    def refused(name, **kw):
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportConvolved" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), name

    def tap(value):
        h = flat.copy()
        h[5 + 17] = value
        return h

    refused("not synthesised since it was set")
    bp.synthesize()
    pcm = [bp.read(u).copy() for u in range(s.n)]
    seg = next(g for g in torch.cuda.memory_snapshot() if g["address"] <= out.data_ptr() < g["address"] + g["total_size"])
    one_short = seg["address"] + seg["total_size"] - 4 * (total - 1)
    assert one_short >= seg["address"]
    cases = dict(
        no_batch=dict(batch=None), format_2=dict(fmt=2), format_negative=dict(fmt=-1), stride_negative=dict(stride=-1), stride_short=dict(stride=most - 1),
        utterance_beyond=dict(utterances=np.array([0, s.n], np.int64), irOf=irOf[:2]), utterance_negative=dict(utterances=np.array([-1], np.int64), irOf=irOf[:1]),
        negative_count=dict(n=-1), host_memory=dict(ptr=host.ctypes.data), no_buffer=dict(ptr=None), misaligned_float=dict(ptr=out.data_ptr() + 2),
        misaligned_int16=dict(ptr=out.data_ptr() + 1, fmt=0), too_small=dict(stride=1 << 34), too_small_packed=dict(stride=0, ptr=one_short),
        tail_2=dict(tail=2), tail_negative=dict(tail=-1), nIr_zero=dict(nIr=0), nIr_negative=dict(nIr=-2), no_ir=dict(ir=None), no_start=dict(start=None, nIr=2),
        start_not_zero=dict(start=np.array([1, 5, 45], np.int64)), start_not_increasing=dict(start=np.array([0, 45, 5], np.int64)),
        response_of_no_taps=dict(start=np.array([0, 5, 5], np.int64)), response_too_long=dict(ir=big, start=np.array([0, 5, 5 + sp.CONVOLVE_MAX_TAPS + 1], np.int64)),
        table_too_long=dict(ir=big, start=np.concatenate([steps, [sp.CONVOLVE_MAX_TABLE + 1]]).astype(np.int64), irOf=np.zeros(s.n, np.int64)),
        irOf_beyond=dict(irOf=np.where(utt == 7, 2, irOf).astype(np.int64)), irOf_negative=dict(irOf=np.where(utt == 0, -1, irOf).astype(np.int64)),
        irOf_missing=dict(irOf=None), tap_nan=dict(ir=tap(np.nan)), tap_inf=dict(ir=tap(np.inf)), tap_minus_inf=dict(ir=tap(-np.inf)),
        tap_above_2_32=dict(ir=tap(np.float32(2.0 ** 32 * (1 + 2.0 ** -23)))), tap_below_minus_2_32=dict(ir=tap(-2.0 ** 33)))
    for name, kw in cases.items():
        refused(name, **kw)
    assert call(ir=tap(np.nan)) == -1 and b"tap 17 of response 1" in L.speechPlayer_lastError()
    # nothing to write needs no buffer
    assert export(L, bp, None, utt[:0], flat, start, irOf[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    # the limits themselves are admitted, and the batch is as usable as before
    assert call(ir=tap(-2.0 ** 32), utterances=utt[:1], irOf=np.zeros(1, np.int64), stride=0) == lens[0]
    assert call(ir=big, start=steps, irOf=np.zeros(1, np.int64), utterances=utt[9:], stride=0, tail=0) == s.length(9)      # 2^20 taps in all, 65 536 in one
    torch.cuda.synchronize()
    assert same(out[:s.length(9)].cpu().numpy(), eng.pcmConvolve(pcm[9], big[:sp.CONVOLVE_MAX_TAPS], tail=False))
    assert call() == s.n * most
    torch.cuda.synchronize()
    got = out[:s.n * most].view(s.n, most).cpu().numpy()
    for u in range(s.n):
        w = eng.pcmConvolve(pcm[u], irs[u % 2])
        assert same(got[u, :len(w)], w) and not bits(got[u, len(w):]).any(), u
    assert torch.equal(out[s.n * most:], sentinel[s.n * most:])
    bp.synthesize()
    assert all(np.array_equal(bp.read(u), pcm[u]) for u in range(s.n))
    bp.close()
