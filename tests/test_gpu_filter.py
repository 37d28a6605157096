"""A batch's PCM and a signal's rows through cascades of biquad sections (include/speechPlayer_batch.h: speechPlayer_batch_exportFiltered,
exportFilteredOf; BatchPlayer.filteredTensor; csrc/klatt_filter.h) against the host's statement of the definition, speechPlayer_pcmFilter /
signalFilter applied to what the engine read -- bit for bit, float32 and int16.  The statement itself is held to a transcription and to
a binary64 recursion by tests/test_filter_host.py.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_filter_host import impulse_rows, seven, stable, subnormal
from tests.test_convolve_host import decaying
from tests.test_gpu_resample import rows_of, same
from tests.test_gpu_signal import edge_rows, lay_out, poison, record
from tests.test_gpu_spectrogram import bits, player
from tests.test_gpu_timeline import set_host
from tests.test_stems_host import compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64


def tile():
    from nvspeechplayer_amd import speechPlayer as sp
    return sp.FILTER_TILE


class Statement:
    """The host's statement per (row, filter, dtype) with the longest tail asked for, computed once: a shorter tail is its head."""
    def __init__(self, rows, filters, most):
        self.rows, self.filters, self.most, self.done = rows, filters, most, {}

    def __call__(self, u, j, npt, tail):
        import nvspeechplayer_amd as eng
        key = (u, j, npt)
        if key not in self.done:
            self.done[key] = eng.signalFilter(self.rows[u], self.filters[j], tail=self.most, dtype=npt)
        return self.done[key][:len(self.rows[u]) + tail]


def check_every_form(bp, want, sel, of, tails, tag):
    """float32 and int16, padded and packed, every tail: every row's bits are the statement's, the padding is +0 on its bit pattern, the
    lengths and offsets are as defined."""
    import torch
    for dtype, npt in ((torch.float32, np.float32), (torch.int16, np.int16)):
        for tail in tails:
            rows_want = [want(u, j, npt, tail) for u, j in zip(sel, of)]
            lens = [len(want.rows[u]) + tail for u in sel]
            for padded in (True, False):
                out, second = bp.filteredTensor(want.filters, filterOf=of, tail=tail, utterances=sel, dtype=dtype, padded=padded)
                assert list(second.numpy()) == (lens if padded else list(np.concatenate([[0], np.cumsum(lens)]))), tag
                assert out.dtype == dtype and out.shape == ((len(sel), max(lens)) if padded else (sum(lens),)), tag
                rows, past = rows_of(out, second, padded)
                for i, (g, w) in enumerate(zip(rows, rows_want)):
                    assert same(g, w), (tag, dtype, tail, padded, i, sel[i], of[i])
                for i, z in enumerate(past):
                    assert not z.view(np.uint32 if npt == np.float32 else np.uint16).any(), (tag, "padding", i)


@pytest.mark.parametrize("name", ["plain", "plain16k"])
def test_the_device_gives_the_statements_bits(name):
    """The ten-utterance batches at 22 050 and 16 000 Hz, seven filters of 1, 2, 3, 5, 8, 9 and 16 sections cycled over the rows -- one
    call mixes every bucket and rows padded with identity sections --, every form, tails 0, 1 and T + 3; and a selection with repeats, a
    different filter on each repeat."""
    T = tile()
    s = compared(name)
    bp, pcm = player(s.b, s.sr)
    assert [len(p) for p in pcm] == [s.length(u) for u in range(s.n)] and any(p.any() for p in pcm)
    filters = seven()
    want = Statement(pcm, filters, T + 3)
    tails = (0, 1, T + 3)
    check_every_form(bp, want, list(range(s.n)), [u % 7 for u in range(s.n)], tails, (name, "cycled"))
    check_every_form(bp, want, [9, 3, 3, 0, 9, 2, 3], [6, 5, 1, 4, 0, 2, 3], tails, (name, "selection"))
    # one filter for every row needs no filterOf
    out, lens = bp.filteredTensor(filters[3], padded=False)
    for u, g in enumerate(rows_of(out, lens, False)[0]):
        assert same(g, want(u, 3, np.float32, 0)), u
    # the identity section is pcmTensor
    import torch
    for dtype in (torch.float32, torch.int16):
        a, la = bp.pcmTensor(dtype=dtype)
        b, lb = bp.filteredTensor([[1, 0, 0, 0, 0]], dtype=dtype)
        assert torch.equal(la, lb) and torch.equal(a, b), dtype
    bp.close()


def export_of(L, bp, sig, rows, sections, start, of, tail, ptr, fmt=1, stride=0, batch=0, stream=None):
    p = lambda a: None if a is None else a.ctypes.data
    return L.speechPlayer_batch_exportFilteredOf(bp._h if batch == 0 else batch, sig, p(rows), 0 if rows is None else len(rows), p(sections), p(start), len(start) - 1,
                                                 p(of), tail, ptr, fmt, stride, stream)


@pytest.fixture(scope="module")
def bare():
    """A player that was never set: the exports of a signal need no batch content."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    yield bp
    bp.close()


@pytest.mark.parametrize("npt", [np.float32, np.int16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_group_boundaries(bare, n, npt):
    """Signals made on the host of 1, 63, 64, 65 and 130 rows of 0, 1, T - 1, T, T + 1 and 2 T + 3 samples in an order that is not
    sorted, the seven filters cycled, through the library's entry point into a buffer with guards either side, 0, 1 and 3 elements past a
    16-byte boundary, packed and padded, both output formats, with and without a tail: the smallest shapes at which tile edges, the
    double buffer, the masks and the packing can go wrong.  What lies between and around the rows of the signal is poison."""
    import torch
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    T = tile()
    bp = bare
    dev = "cuda:%d" % bp.device
    kinds = [T + 1, 0, 2 * T + 3, 1, T, T - 1]
    lens = [kinds[(5 * i + i // 6) % 6] for i in range(n)]
    assert n < 6 or (set(lens) == set(kinds) and lens != sorted(lens) and lens != sorted(lens, reverse=True))
    rows = edge_rows(lens, npt, 300 + n)
    filters = seven()
    flat, start = np.concatenate(filters), np.concatenate([[0], np.cumsum([len(f) for f in filters])]).astype(np.int64)
    of = ((np.arange(n) * 3) % 7).astype(np.int64)
    most_tail = T + 3
    want = Statement(rows, filters, most_tail)
    sel = np.arange(n, dtype=np.int64)
    forms = [(1, "packed", 1, 0), (0, "packed", 3, most_tail), (1, "padded", 3, most_tail), (0, "padded", 1, 0), (1, "padded", 0, 1)]
    for k, (in_stride, in_shift) in enumerate(((0, 1), (2 * T + 5, 2))):
        host, first, extent = lay_out(rows, npt, in_stride, poison, in_shift)
        data = torch.from_numpy(host.view(np.int32 if npt == np.float32 else np.int16)).to(dev)
        rec = record(sp, data.data_ptr() + first * data.element_size(), 1 if npt == np.float32 else 0, n, in_stride, extent)
        for fmt, form, shift, tail in forms[k::2] if n not in (65, 130) else forms:
            out_np, dtype = (np.float32, torch.float32) if fmt else (np.int16, torch.int16)
            rows_want = [want(i, int(of[i]), out_np, tail) for i in range(n)]
            stride = 0 if form == "packed" else max(len(w) for w in rows_want) + 3
            elements = sum(len(w) for w in rows_want) if stride == 0 else n * stride
            buf = torch.full((elements + 2 * GUARD + shift,), -7, dtype=dtype, device=dev)
            assert buf.data_ptr() % 16 == 0
            got = export_of(L, bp, rec.ctypes.data, sel, flat, start, of, tail, buf.data_ptr() + (GUARD + shift) * buf.element_size(), fmt=fmt, stride=stride)
            assert got == elements, (got, elements, L.speechPlayer_lastError())
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            tag = (n, npt.__name__, in_stride, fmt, form, shift, tail)
            assert np.all(got[:GUARD + shift] == -7) and np.all(got[GUARD + shift + elements:] == -7), tag
            got = got[GUARD + shift:GUARD + shift + elements]
            at = 0
            for i, w in enumerate(rows_want):
                span = len(w) if stride == 0 else stride
                assert same(got[at:at + len(w)], w), tag + (i, lens[i], int(of[i]))
                assert not got[at + len(w):at + span].view(np.uint32 if fmt else np.uint16).any(), tag + (i, "padding")
                at += span


def test_subnormal_results_are_kept(bare):
    """The two impulse rows of the host test, each in a 64-row signal beside full-scale rows: the bits are the statement's, the halving
    section's 23 subnormal values and the resonator's subnormal limit cycle are there -- nothing is flushed to zero."""
    import torch
    import nvspeechplayer_amd as eng
    bp = bare
    rng = np.random.default_rng(23)
    for which, (impulse, sec) in enumerate(impulse_rows()):
        rows = [impulse if i % 2 == 0 else rng.integers(-32768, 32768, len(impulse)).astype(np.int16) for i in range(64)]
        signal = (torch.from_numpy(np.stack(rows)).to("cuda:%d" % bp.device), torch.full((64,), len(impulse), dtype=torch.int64))
        out, lens = bp.filteredTensor(sec, signal=signal)
        got = out.cpu().numpy()
        want = eng.pcmFilter(impulse, sec)
        for i in range(64):
            assert same(got[i], want if i % 2 == 0 else eng.pcmFilter(rows[i], sec)), (which, i)
        if which == 0:
            assert np.count_nonzero(subnormal(got[0])) == 23 and got[0][149] == 2.0 ** -149 and not bits(got[0][150:]).any()
        else:
            assert np.all(subnormal(got[62][-200:])), "the limit cycle"
        assert np.abs(rows[1]).max() > 30000 and np.abs(got[1]).max() > 1e-3      # (the neighbours are at full scale, and pass)


def test_the_chain_equals_the_composition_of_the_host_statements():
    """convolved -> filtered (the telephone band, from the designers) -> resampled to 16 kHz, each stage reading the one before as its
    signal=, against the host statements composed; float32 between the stages, and int16 at the end."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    rooms = [decaying(40, 1), decaying(300, 2)]
    of = [u % 2 for u in range(s.n)]
    band = np.concatenate([eng.biquad("highpass", s.sr, 300.0), eng.biquad("lowpass", s.sr, 3400.0), eng.preEmphasis(0.97)])
    wet = bp.convolvedTensor(rooms, irOf=of)
    phone = bp.filteredTensor(band, tail=5, signal=wet)
    x16k = bp.resampledTensor(16000, signal=phone)
    x16 = bp.resampledTensor(16000, signal=phone, dtype=torch.int16, padded=False)
    got, got16 = rows_of(*x16k, True)[0], rows_of(*x16, False)[0]
    mid = rows_of(*phone, True)[0]
    for u in range(s.n):
        a = eng.pcmConvolve(pcm[u], rooms[of[u]])
        b = eng.signalFilter(a, band, tail=5)
        assert same(mid[u], b), u
        assert same(got[u], eng.signalResample(b, s.sr, 16000)), u
        assert same(got16[u], eng.signalResample(b, s.sr, 16000, dtype=np.int16)), u
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
    filters = [stable(2, 1), stable(5, 2)]
    flat, start = np.concatenate(filters), np.array([0, 2, 7], np.int64)
    of = (utt % 2).astype(np.int64)
    lens = [s.length(u) + 4 for u in range(s.n)]
    most = max(lens)
    out = torch.full((s.n * most + 8,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel = out.clone()
    host = np.zeros(s.n * most, np.float32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(ptr=0, utterances=utt, sections=flat, starts=start, filterOf=of, tail=4, fmt=1, stride=most, n=None, nFilters=None, batch=0):
        return L.speechPlayer_batch_exportFiltered(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, p(sections), p(starts),
                                                   len(starts) - 1 if nFilters is None else nFilters, p(filterOf), tail, out.data_ptr() if ptr == 0 else ptr, fmt, stride, None)

    def refused(name, **kw):
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert b"exportFiltered" in L.speechPlayer_lastError(), name
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel), name

    def coefficient(section, q, value):
        f = flat.copy()
        f[section, q] = value
        return f

    refused("not synthesised since it was set")
    assert b"not been synthesised" in L.speechPlayer_lastError()
    bp.synthesize()
    pcm = [bp.read(u).copy() for u in range(s.n)]
    cases = dict(
        no_batch=dict(batch=None), format_2=dict(fmt=2), stride_negative=dict(stride=-1), stride_short=dict(stride=most - 1),
        utterance_beyond=dict(utterances=np.array([0, s.n], np.int64), filterOf=of[:2]), negative_count=dict(n=-1), host_memory=dict(ptr=host.ctypes.data), no_buffer=dict(ptr=None),
        misaligned_float=dict(ptr=out.data_ptr() + 2), misaligned_int16=dict(ptr=out.data_ptr() + 1, fmt=0), too_small=dict(stride=1 << 34),
        tail_negative=dict(tail=-1), tail_above=dict(tail=(1 << 20) + 1), no_filters=dict(nFilters=0), no_sections=dict(sections=None), no_starts=dict(starts=None, nFilters=2),
        start_not_zero=dict(starts=np.array([1, 2, 7], np.int64)), filter_of_no_sections=dict(starts=np.array([0, 2, 2], np.int64)),
        filter_of_17=dict(sections=np.tile(flat[:1], (20, 1)), starts=np.array([0, 2, 19], np.int64)),
        table=dict(sections=np.tile(flat[:1], ((1 << 16) + 16, 1)), starts=np.arange(0, (1 << 16) + 17, 16).astype(np.int64), filterOf=np.zeros(s.n, np.int64)),
        filterOf_beyond=dict(filterOf=np.where(utt == 7, 2, of).astype(np.int64)), filterOf_negative=dict(filterOf=np.where(utt == 0, -1, of).astype(np.int64)),
        filterOf_missing=dict(filterOf=None), b0_nan=dict(sections=coefficient(4, 0, np.nan)), a1_inf=dict(sections=coefficient(4, 3, np.inf)),
        on_the_circle=dict(sections=coefficient(4, 4, 1.0)), outside=dict(sections=coefficient(4, 4, 1.5)), a1_at_the_edge=dict(sections=coefficient(4, 3, 1.0 + np.float64(flat[4, 4]))),
        a1_beyond=dict(sections=coefficient(4, 3, -2.5)))
    if np.float32(1.0 + np.float64(flat[4, 4])) != 1.0 + np.float64(flat[4, 4]):      # (|a1| = 1 + a2 needs the sum to be a float32: make it one)
        f = coefficient(4, 4, 0.25)
        f[4, 3] = 1.25
        cases["a1_at_the_edge"] = dict(sections=f)
    for name, kw in cases.items():
        refused(name, **kw)
    assert call(sections=coefficient(4, 4, 1.0)) == -1 and b"section 2 of filter 1" in L.speechPlayer_lastError()
    assert call(sections=coefficient(1, 2, np.inf)) == -1 and b"b2 of section 1 of filter 0" in L.speechPlayer_lastError()
    assert call(filterOf=np.where(utt == 7, 2, of).astype(np.int64)) == -1 and b"filterOf[7] = 2" in L.speechPlayer_lastError()
    # nothing to write needs no buffer
    assert call(ptr=None, utterances=utt[:0], filterOf=of[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    # the limits themselves are admitted, and the batch is as usable as before
    assert call(sections=np.tile(flat[:1], (1 << 16, 1)), starts=np.arange(0, (1 << 16) + 1, 16).astype(np.int64), filterOf=np.full(1, 4095, np.int64), utterances=utt[9:], stride=0, tail=0) == s.length(9)
    torch.cuda.synchronize()
    assert same(out[:s.length(9)].cpu().numpy(), eng.pcmFilter(pcm[9], np.tile(flat[:1], (16, 1))))
    assert call() == s.n * most
    torch.cuda.synchronize()
    got = out[:s.n * most].view(s.n, most).cpu().numpy()
    for u in range(s.n):
        w = eng.pcmFilter(pcm[u], filters[u % 2], tail=4)
        assert same(got[u, :len(w)], w) and not bits(got[u, len(w):]).any(), u
    assert torch.equal(out[s.n * most:], sentinel[s.n * most:])
    bp.synthesize()
    assert all(np.array_equal(bp.read(u), pcm[u]) for u in range(s.n))
    # seventeen exports in flight: every slot, and one more
    first = [bp.read(u).copy() for u in range(s.n)]
    outs = [bp.filteredTensor(seven()[i % 7], tail=i % 3, padded=False) for i in range(17)]
    torch.cuda.synchronize()
    for i, (o, offsets) in enumerate(outs):
        for u, g in enumerate(rows_of(o, offsets, False)[0]):
            assert same(g, eng.pcmFilter(first[u], seven()[i % 7], tail=i % 3)), (i, u)
    set_host(bp, s.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.filteredTensor(filters[0])
    bp.close()
