"""A batch's PCM and a signal's rows through the G.711 laws and IMA ADPCM (include/speechPlayer_batch.h: speechPlayer_batch_exportCoded,
exportCodedOf; BatchPlayer.codedTensor; csrc/klatt_codec.h) against the host's statement of the definition, speechPlayer_pcmCode /
signalCode applied to what the engine read, and against what audioop answered (tests/golden/codec_golden.npz) -- bit for bit, codes and
decoded samples, int16 and float32.  The statement itself is held to audioop and to a transcription by tests/test_codec_host.py.
Needs a GPU."""
import numpy as np
import pytest

from tests.test_codec_host import EVERY, LAWS, adpcm_rows, golden, statement
from tests.test_convolve_host import x_of
from tests.test_gpu_resample import rows_of
from tests.test_gpu_signal import edge_rows, lay_out, poison, record
from tests.test_gpu_spectrogram import player
from tests.test_gpu_timeline import set_host
from tests.test_stems_host import compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64
CODECS = ("ulaw", "alaw", "adpcm")
# what an export puts out: (decoded, its format, codes)
OUTPUTS = (("int16", True, 0, False), ("float32", True, 1, False), ("codes", False, 0, True), ("both", True, 0, True), ("both32", True, 1, True))


def same(got, want):
    """Equality of type, shape and every bit."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def tiles():
    from nvspeechplayer_amd import speechPlayer as sp
    return sp.FILTER_TILE, sp.CODE_TILE


@pytest.fixture(scope="module")
def bare():
    """A player that was never set: the exports of a signal need no batch content."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    yield bp
    bp.close()


def as_signal(bp, rows):
    """Rows of one length as a padded signal on the batch's device."""
    import torch
    return torch.from_numpy(np.stack(rows)).to("cuda:%d" % bp.device), torch.full((len(rows),), len(rows[0]), dtype=torch.int64)


def test_the_exhaustive_row(bare):
    """One row of all 65 536 int16 values in a seeded shuffle, as int16 and as float32 (s / 32767): the mu-law and A-law codes and decoded
    samples are the fixture's tables, ADPCM is the host's statement."""
    import torch
    import nvspeechplayer_amd as eng
    bp = bare
    g = golden()
    order = np.random.default_rng(65536).permutation(65536)
    row = EVERY[order]
    assert sorted(row.tolist()) == list(range(-32768, 32768))
    for x in (row, x_of(row)):
        signal = as_signal(bp, [x])
        for law in LAWS:
            decoded, codes, lens = bp.codedTensor(law, codes=True, signal=signal)
            assert list(lens.numpy()) == [65536] and decoded.dtype == torch.int16 and codes.dtype == torch.uint8 and decoded.shape == codes.shape == (1, 65536)
            want = g[law + "_encode"][order]
            assert np.array_equal(codes.cpu().numpy()[0], want), (law, x.dtype)
            assert np.array_equal(decoded.cpu().numpy()[0], g[law + "_decode"][want]), (law, x.dtype)
            table = torch.from_numpy(eng.codecTable(law)).to(codes.device)
            assert torch.equal(table[codes.long()], decoded), law      # (the decode table, on the device)
        decoded, codes, lens = bp.codedTensor("adpcm", codes=True, signal=signal)
        wd, wc = eng.pcmCode(row, "adpcm", codes=True)
        assert np.array_equal(codes.cpu().numpy()[0], wc) and np.array_equal(decoded.cpu().numpy()[0], wd), x.dtype
        f32, _ = bp.codedTensor("adpcm", signal=signal, dtype=torch.float32)
        assert same(f32.cpu().numpy()[0], x_of(wd)), x.dtype


def test_the_fixtures_adpcm_rows(bare):
    """audioop's 24 ADPCM rows, each length's three rows as one signal: codes and decoded samples are the recorded ones."""
    bp = bare
    rows = list(adpcm_rows())
    for L in sorted({r[1] for r in rows} - {0}):
        three = [r for r in rows if r[1] == L]
        decoded, codes, lens = bp.codedTensor("adpcm", codes=True, signal=as_signal(bp, [r[2] for r in three]))
        for i, (kind, _, x, wc, wd, _) in enumerate(three):
            assert np.array_equal(codes.cpu().numpy()[i], wc) and np.array_equal(decoded.cpu().numpy()[i], wd), (kind, L)


def export_of(L, bp, sig, rows, codec, decoded, fmt, codes, stride, batch=0, stream=None):
    p = lambda a: None if a is None else a.ctypes.data
    return L.speechPlayer_batch_exportCodedOf(bp._h if batch == 0 else batch, sig, p(rows), 0 if rows is None else len(rows), codec, decoded, fmt, codes, stride, stream)


def check_guarded(call, want, lens, outputs, stride, shift, dev, tag):
    """call(decoded pointer, codes pointer) fills poisoned buffers between guards, `shift` elements past a 16-byte boundary: the guards stay,
    every row is the statement's (want[i] = (decoded, codes) in the output's format) and the padding is +0 / code 0."""
    import torch
    _, has_decoded, fmt, has_codes = outputs
    elements = sum(lens) if stride == 0 else len(lens) * stride
    dtype = torch.float32 if fmt else torch.int16
    d = torch.full((elements + 2 * GUARD + shift,), -7, dtype=dtype, device=dev)
    c = torch.full((elements + 2 * GUARD + shift,), 0xC9, dtype=torch.uint8, device=dev)
    assert d.data_ptr() % 16 == 0 and c.data_ptr() % 16 == 0
    got = call(d.data_ptr() + (GUARD + shift) * d.element_size() if has_decoded else None, c.data_ptr() + GUARD + shift if has_codes else None)
    assert got == elements, (tag, got, elements)
    torch.cuda.synchronize()
    for which, buf, has, fill in ((0, d, has_decoded, -7), (1, c, has_codes, 0xC9)):
        a = buf.cpu().numpy()
        if not has:
            assert np.all(a == fill), tag + ("an output not asked for",)
            continue
        assert np.all(a[:GUARD + shift] == fill) and np.all(a[GUARD + shift + elements:] == fill), tag + ("guards", which)
        a = a[GUARD + shift:GUARD + shift + elements]
        at = 0
        for i, L in enumerate(lens):
            span = L if stride == 0 else stride
            w = want[i][which]
            assert len(w) == L and same(a[at:at + L], w), tag + (which, i, L)
            assert not a[at + L:at + span].view(np.uint8).any(), tag + (which, i, "padding")
            at += span


@pytest.mark.parametrize("npt", [np.int16, np.float32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_boundaries(bare, n, npt):
    """Signals made on the host of 1, 63, 64, 65 and 130 rows of 0, 1, 2, T - 1, T, T + 1 and 3 T + 5 samples for both kernels' tiles (64 and
    1024) in an order that is not sorted, int16 and float32, through the library's entry point into poisoned buffers with guards either
    side, 0, 1 and 3 elements past a 16-byte boundary: packed and padded, the three codecs, decoded int16, decoded float32, codes only and
    both.  Packed rows of odd lengths start the uint8 rows on every byte offset.  What lies between and around the rows of the signal
    is poison."""
    import torch
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    bp = bare
    dev = "cuda:%d" % bp.device
    kinds = sorted({v for T in tiles() for v in (0, 1, 2, T - 1, T, T + 1, 3 * T + 5)})
    assert len(kinds) == 11
    lens = [kinds[(7 * i + i // 11) % 11] for i in range(n)] if n > 1 else [3 * 64 + 5]
    assert n < 11 or (set(lens) == set(kinds) and lens != sorted(lens) and lens != sorted(lens, reverse=True))
    rows = edge_rows(lens, npt, 700 + n)
    want = {(codec, fmt): [statement(r, codec, np.float32 if fmt else np.int16) for r in rows] for codec in CODECS for fmt in (0, 1)}
    sel = np.arange(n, dtype=np.int64)
    offsets = set()
    k = 0
    for in_stride, in_shift in ((0, 1), (max(lens) + 5, 2)):
        host, first, extent = lay_out(rows, npt, in_stride, poison, in_shift)
        data = torch.from_numpy(host.view(np.int32 if npt == np.float32 else np.int16)).to(dev)
        rec = record(sp, data.data_ptr() + first * data.element_size(), 1 if npt == np.float32 else 0, n, in_stride, extent)
        for ci, codec in enumerate(CODECS):
            for outputs in OUTPUTS:
                for form in ("packed", "padded"):
                    k += 1
                    if (k + in_shift) % 2 and n not in (65, 130):      # (the small row counts take every other combination of each layout of the input)
                        continue
                    shift = (0, 1, 3)[k % 3]
                    stride = 0 if form == "packed" else max(lens) + 3
                    if stride == 0 and outputs[3]:
                        offsets |= {int(v + shift) % 16 for v in np.cumsum(lens)[:-1]}
                    call = lambda d, c: export_of(L, bp, rec.ctypes.data, sel, ci, d, outputs[2], c, stride)
                    check_guarded(call, want[(codec, outputs[2])], lens, outputs, stride, shift, dev, (n, npt.__name__, in_stride, codec, outputs[0], form, shift))
    if n == 130:
        assert offsets == set(range(16)), "packed uint8 rows start on every byte offset"


def test_the_pool():
    """The ten-utterance batch: codedTensor equals pcmCode of what the engine reads back, every codec and output, padded and packed, all the
    utterances and a selection with repeats; through the entry point into guarded buffers as well."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    assert any(p.any() for p in pcm)
    p = lambda a: None if a is None else a.ctypes.data
    for sel in (None, [9, 3, 3, 0, 9, 2, 3]):
        idx = list(range(s.n)) if sel is None else sel
        lens = [len(pcm[u]) for u in idx]
        for codec in CODECS:
            wd, wc = zip(*[eng.pcmCode(pcm[u], codec, codes=True) for u in idx])
            for padded in (True, False):
                second = lens if padded else list(np.concatenate([[0], np.cumsum(lens)]))
                for dtype in (None, torch.int16, torch.float32):
                    d, c, got = bp.codedTensor(codec, codes=True, utterances=sel, dtype=dtype, padded=padded)
                    assert list(got.numpy()) == second and d.dtype == (torch.float32 if dtype == torch.float32 else torch.int16) and c.dtype == torch.uint8
                    assert d.shape == c.shape == ((len(idx), max(lens)) if padded else (sum(lens),))
                    (rd, pd), (rc, pc) = rows_of(d, got, padded), rows_of(c, got, padded)
                    for i in range(len(idx)):
                        assert same(rd[i], x_of(wd[i]) if dtype == torch.float32 else wd[i]) and same(rc[i], wc[i]), (codec, padded, dtype, i)
                    assert not any(z.view(np.uint8).any() for z in pd + pc), (codec, "padding")
                d, got = bp.codedTensor(codec, utterances=sel, padded=padded)
                c, got2 = bp.codedTensor(codec, codes=True, decoded=False, utterances=sel, padded=padded)
                assert torch.equal(got, got2) and all(same(a, w) for a, w in zip(rows_of(d, got, padded)[0], wd)) and all(same(a, w) for a, w in zip(rows_of(c, got, padded)[0], wc))
            utt = None if sel is None else np.array(sel, np.int64)
            for k, outputs in enumerate(OUTPUTS):
                want = [(x_of(a) if outputs[2] else a, b) for a, b in zip(wd, wc)]
                stride = 0 if k % 2 else max(lens) + 1
                call = lambda dp, cp: L.speechPlayer_batch_exportCoded(bp._h, p(utt), len(idx), CODECS.index(codec), dp, outputs[2], cp, stride, None)
                check_guarded(call, want, lens, outputs, stride, (1, 3, 0)[k % 3], "cuda:%d" % bp.device, ("pool", codec, outputs[0], stride))
    bp.close()


def test_the_chain_equals_the_composition_of_the_host_statements():
    """filtered (the telephone band, from the designers) -> resampled to 8 kHz -> coded (mu-law), each stage reading the one before as
    its signal=, against the host statements composed; the decoded pair feeds a further stage."""
    import torch
    import nvspeechplayer_amd as eng
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    band = np.concatenate([eng.biquad("highpass", s.sr, 300.0), eng.biquad("lowpass", s.sr, 3400.0)])
    phone = bp.filteredTensor(band)
    narrow = bp.resampledTensor(8000, signal=phone)
    decoded, codes, lens = bp.codedTensor("ulaw", codes=True, signal=narrow)
    handset = bp.codedTensor("adpcm", signal=narrow, dtype=torch.float32, padded=False)
    again = bp.resampledTensor(16000, signal=(decoded, lens), signalRate=8000)
    gd, gc, gh, ga = rows_of(decoded, lens, True)[0], rows_of(codes, lens, True)[0], rows_of(*handset, False)[0], rows_of(*again, True)[0]
    for u in range(s.n):
        a = eng.signalFilter(pcm[u], band)
        b = eng.signalResample(a, s.sr, 8000)
        wd, wc = eng.signalCode(b, "ulaw", codes=True)
        assert same(gd[u], wd) and same(gc[u], wc), u
        assert same(gh[u], eng.signalCode(b, "adpcm", dtype=np.float32)), u
        assert same(ga[u], eng.signalResample(wd, 8000, 16000)), u
    assert any(len(set(c.tolist())) > 64 for c in gc), "the chain carries speech"
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
    lens = [s.length(u) for u in range(s.n)]
    most = max(lens)
    dev = "cuda:%d" % bp.device
    out = torch.full((s.n * most + 8,), -7, dtype=torch.int16, device=dev)
    codes = torch.full((s.n * most + 8,), 0xC9, dtype=torch.uint8, device=dev)
    sentinel, sentinel_codes = out.clone(), codes.clone()
    host = np.zeros(s.n * most, np.int16)
    p = lambda a: None if a is None else a.ctypes.data

    def call(ptr=0, cptr=0, utterances=utt, codec=2, fmt=0, stride=most, n=None, batch=0):
        return L.speechPlayer_batch_exportCoded(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, codec,
                                                out.data_ptr() if ptr == 0 else ptr, fmt, codes.data_ptr() if cptr == 0 else cptr, stride, None)

    def refused(name, words=b"", entry=b"exportCoded", fn=call, **kw):
        assert fn(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert entry in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel) and torch.equal(codes, sentinel_codes), name

    refused("not synthesised since it was set", b"not been synthesised")
    bp.synthesize()
    pcm = [bp.read(u).copy() for u in range(s.n)]
    cases = dict(
        no_batch=(dict(batch=None), b"no batch"), codec_3=(dict(codec=3), b"codec 3"), codec_negative=(dict(codec=-1), b"codec -1"),
        both_null=(dict(ptr=None, cptr=None), b"no output"), format_2=(dict(fmt=2), b"format 2"), format_negative=(dict(fmt=-1), b"format -1"),
        stride_negative=(dict(stride=-1), b"rowStride -1"), stride_short=(dict(stride=most - 1), b""), utterance_beyond=(dict(utterances=np.array([0, s.n], np.int64)), b"utterances[1]"),
        negative_count=(dict(n=-1), b""), host_memory=(dict(ptr=host.ctypes.data), b""), host_codes=(dict(cptr=host.ctypes.data), b""),
        misaligned_int16=(dict(ptr=out.data_ptr() + 1), b""), misaligned_float=(dict(ptr=out.data_ptr() + 2, fmt=1), b""), too_small=(dict(stride=1 << 34), b""),
        codes_too_small=(dict(ptr=None, stride=1 << 34), b""), overlap=(dict(cptr=out.data_ptr() + 64), b"overlap"))
    for name, (kw, words) in cases.items():
        refused(name, words, **kw)
        refused(name + " (ulaw)", words, **dict(kw, codec=kw.get("codec", 0)))
    # a signal's table
    x = torch.zeros((4, 100), dtype=torch.int16, device=dev)
    extent = np.full(4, 100, np.int64)

    def of(rec=None, rows=None, **fields):
        if rec is None:
            rec = record(sp, x.data_ptr(), 0, 4, 100, extent)
            for key, v in fields.items():
                rec[key] = v
            rec = rec.ctypes.data
        return L.speechPlayer_batch_exportCodedOf(bp._h, rec, p(rows), 0 if rows is None else len(rows), 0, out.data_ptr(), 0, codes.data_ptr(), 100, None)

    bad_extent = np.array([100, 101, 0, 0], np.int64)
    for name, kw, words in (("no signal", dict(rec=0), b"no signal"), ("signal format", dict(format=2), b"signal format 2"), ("signal rows", dict(nRows=-1), b"nRows"),
                            ("signal stride", dict(rowStride=-1), b"rowStride"), ("no extent", dict(extent=0), b"extent"), ("extent beyond the stride", dict(extent=bad_extent.ctypes.data), b"extent[1]"),
                            ("no data", dict(data=0), b"without data"), ("host data", dict(data=host.ctypes.data), b""), ("row beyond", dict(rows=np.array([4], np.int64)), b"rows[0] = 4"),
                            ("the output is the signal", dict(data=out.data_ptr()), b"overlaps")):
        refused(name, words, entry=b"exportCodedOf", fn=of, **kw)
    assert of() == 400
    torch.cuda.synchronize()
    assert not out[:400].any() and torch.all(codes[:400] == 0xFF) and torch.equal(out[400:], sentinel[400:])      # (mu-law of silence)
    out.copy_(sentinel); codes.copy_(sentinel_codes)
    # nothing to write needs no buffer
    assert call(ptr=None, cptr=None, utterances=utt[:0]) == -1      # (both outputs NULL is refused before anything is counted)
    assert call(cptr=None, utterances=utt[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    # and the batch is as usable as before
    for codec in (0, 2):
        assert call(codec=codec) == s.n * most
        torch.cuda.synchronize()
        got, got_codes = out[:s.n * most].view(s.n, most).cpu().numpy(), codes[:s.n * most].view(s.n, most).cpu().numpy()
        for u in range(s.n):
            wd, wc = eng.pcmCode(pcm[u], codec, codes=True)
            assert same(got[u, :len(wd)], wd) and same(got_codes[u, :len(wc)], wc) and not got[u, len(wd):].any() and not got_codes[u, len(wc):].any(), (codec, u)
        assert torch.equal(out[s.n * most:], sentinel[s.n * most:]) and torch.equal(codes[s.n * most:], sentinel_codes[s.n * most:])
    bp.synthesize()
    assert all(np.array_equal(bp.read(u), pcm[u]) for u in range(s.n))
    # seventeen exports in flight: every slot, and one more
    outs = [bp.codedTensor(CODECS[i % 3], codes=True, padded=False) for i in range(17)]
    torch.cuda.synchronize()
    for i, (d, c, offsets) in enumerate(outs):
        for u, (gd, gc) in enumerate(zip(rows_of(d, offsets, False)[0], rows_of(c, offsets, False)[0])):
            wd, wc = eng.pcmCode(pcm[u], CODECS[i % 3], codes=True)
            assert same(gd, wd) and same(gc, wc), (i, u)
    set_host(bp, s.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.codedTensor("alaw")
    with pytest.raises(KeyError):
        bp.codedTensor("g722")
    with pytest.raises(ValueError):
        bp.codedTensor("ulaw", codes=False, decoded=False)
    bp.close()
