"""The spectrogram, resampled and convolved exports on a caller's device signal (include/speechPlayer_batch.h:
speechPlayer_batch_exportSpectrogramOf / exportResampledOf / exportConvolvedOf; BatchPlayer.spectrogramTensor / resampledTensor /
convolvedTensor with signal=; csrc/klatt_tiles.h: the reader): the pool handed back as a signal gives the pool exports' bits; the chain
mix -> room -> 16 kHz -> log-mel equals the composition of the host statements; what lies beside a row is never read as signal; the
float64 numpy references of tests/test_signal_host.py; players never set; selections; every refusal.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_convolve_host import decaying, gamma
from tests.test_gpu_mix import single_frames
from tests.test_gpu_resample import rows_of, same
from tests.test_gpu_spectrogram import player
from tests.test_gpu_timeline import set_host
from tests.test_mix_host import bank
from tests.test_resample_host import FILTERS
from tests.test_resample_host import gamma as res_gamma
from tests.test_signal_host import check_spectrum, conv_reference, res_reference, x_signals
from tests.test_spectrogram_host import ulps
from tests.test_stems_host import compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64
T = 1024
EDGES = [0, 1, 3, T - 1, T, T + 1, 2 * T + 1]
PACKED_EDGES = [0, 1, 1, 1, 1, 1, 1, 1, 3, T - 1, T, T + 1, 2 * T + 1]      # packed: the rows start at every residue of 16 bytes
RATES = [(22050, 16000), (16000, 22050), (32000, 16000)]
TAPS = [1, 5, T + 1]


def test_sizes_are_the_kernels():
    from nvspeechplayer_amd import speechPlayer as sp
    assert sp.RESAMPLE_TILE == sp.CONVOLVE_TILE == T and sp.CONVOLVE_BLOCK == T
    starts = np.concatenate([[0], np.cumsum(PACKED_EDGES)])[:-1]
    assert set(starts % 8) == set(range(8)) and len(PACKED_EDGES) <= 16


# ---- through the signal or through the pool, the same bits ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    yield bp, pcm, s
    bp.close()


def signals_of(bp):
    """pcmTensor in both dtypes, padded and packed: what is handed back as signal=."""
    import torch
    return [(bp.pcmTensor(dtype=dtype, padded=padded), (dtype, padded)) for dtype in (torch.int16, torch.float32) for padded in (True, False)]


def test_the_pool_as_a_signal_gives_the_pool_exports_bits(plain):
    """Every element of the three exports, padding included, in both output dtypes and both output forms."""
    import torch
    import nvspeechplayer_amd as eng
    bp, pcm, s = plain
    irs = [decaying(K, K) for K in TAPS]
    irOf = [u % 3 for u in range(s.n)]
    for signal, tag in signals_of(bp):
        for padded in (True, False):
            for dtype in (torch.float32, torch.int16):
                for rate in (16000, 44100, s.sr):
                    a, la = bp.resampledTensor(rate, dtype=dtype, padded=padded)
                    b, lb = bp.resampledTensor(rate, dtype=dtype, padded=padded, signal=signal)
                    assert torch.equal(la, lb) and a.dtype == b.dtype and torch.equal(a.view(torch.int32 if dtype == torch.float32 else torch.int16),
                                                                                      b.view(torch.int32 if dtype == torch.float32 else torch.int16)), (tag, padded, dtype, rate)
                for tail in (True, False):
                    a, la = bp.convolvedTensor(irs, irOf=irOf, tail=tail, dtype=dtype, padded=padded)
                    b, lb = bp.convolvedTensor(irs, irOf=irOf, tail=tail, dtype=dtype, padded=padded, signal=signal)
                    assert torch.equal(la, lb) and torch.equal(a.view(torch.int32 if dtype == torch.float32 else torch.int16),
                                                               b.view(torch.int32 if dtype == torch.float32 else torch.int16)), (tag, padded, dtype, tail)
            for dtype, as_int in ((torch.float32, torch.int32), (torch.float64, torch.int64)):
                for kw in (dict(nFft=64, hop=16, power=1), dict(nFft=256, hop=100, phase=37, bank=eng.melFilterbank(s.sr, 256, 20)),
                           dict(nFft=256, hop=261, log="db", floor=1e-10)):
                    a, la = bp.spectrogramTensor(dtype=dtype, padded=padded, **kw)
                    b, lb = bp.spectrogramTensor(dtype=dtype, padded=padded, signal=signal, **kw)
                    assert torch.equal(la, lb) and a.shape == b.shape and torch.equal(a.view(as_int), b.view(as_int)), (tag, padded, dtype, sorted(kw))


def test_selection_with_repeats_and_a_response_per_repeat(plain):
    import torch
    import nvspeechplayer_amd as eng
    bp, pcm, s = plain
    irs = [decaying(K, 10 + K) for K in TAPS]
    sel, irOf = [9, 3, 3, 0, 9, 3], [2, 0, 1, 2, 0, 2]
    for signal, tag in signals_of(bp):
        npt = np.int16 if tag[0] == torch.int16 else np.float32
        rows = [p if npt == np.int16 else p.astype(np.float32) / np.float32(32767.0) for p in pcm]
        for padded in (True, False):
            out, second = bp.convolvedTensor(irs, irOf=irOf, utterances=sel, padded=padded, signal=signal)
            for i, g in enumerate(rows_of(out, second, padded)[0]):
                assert same(g, eng.signalConvolve(rows[sel[i]], irs[irOf[i]])), (tag, padded, i)
            out, second = bp.resampledTensor(16000, utterances=sel, padded=padded, dtype=torch.int16, signal=signal)
            for i, g in enumerate(rows_of(out, second, padded)[0]):
                assert same(g, eng.signalResample(rows[sel[i]], s.sr, 16000, dtype=np.int16)), (tag, padded, i)
            out, second = bp.spectrogramTensor(nFft=64, hop=50, utterances=sel, padded=padded, dtype=torch.float64, signal=signal)
            for i, g in enumerate(rows_of(out, second, padded)[0]):
                assert np.array_equal(g.view(np.uint64), eng.signalSpectrogram(rows[sel[i]], nFft=64, hop=50).view(np.uint64)), (tag, padded, i)
    with pytest.raises(ValueError, match="row numbers"):
        bp.convolvedTensor(irs[0], utterances=[0, s.n], signal=signals_of(bp)[0][0])


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
def test_the_chain_equals_the_composition_of_the_host_statements():
    """mixedTensor -> convolvedTensor -> resampledTensor -> spectrogramTensor, each on the one before: every linear value bit for bit,
    the int16 forms, the log-mel within the bar of tests/test_gpu_spectrogram.py (4 ulp in float64), the steps of the 16 kHz lengths."""
    import torch
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    lens = [3, T - 1, T + 1, 2 * T + 1]
    bp, pcm = player(single_frames(lens))
    assert [len(p) for p in pcm] == lens
    clips = bank()
    bp.setNoiseBank(clips)
    sources = clips + pcm
    big = [k for k, c in enumerate(clips) if len(c) > 100 and c.any()]
    assert len(big) >= 2
    terms = [[M(noise=0, gain=0.5)]] + [[M(noise=big[u % len(big)], snr=10.0 - u, offset=7 * u)] for u in range(1, len(lens))]      # (utterance 0 is three samples of silence: no SNR)
    rooms, of = [decaying(K, 60 + K) for K in TAPS], [2, 0, 1, 2]
    mel_bank = eng.melFilterbank(16000, 256, 20)
    spec = dict(nFft=256, hop=160, bank=mel_bank)

    noisy = bp.mixedTensor(terms)
    wet = bp.convolvedTensor(rooms, irOf=of, signal=noisy)
    x16k = bp.resampledTensor(16000, signal=wet)
    mel, steps = bp.spectrogramTensor(log="ln", floor=1e-5, dtype=torch.float64, signal=x16k, **spec)
    lin, steps_lin = bp.spectrogramTensor(dtype=torch.float64, signal=x16k, **spec)
    wet16 = bp.convolvedTensor(rooms, irOf=of, dtype=torch.int16, signal=noisy)
    x16 = bp.resampledTensor(16000, dtype=torch.int16, signal=wet)
    mel16, _ = bp.spectrogramTensor(dtype=torch.float64, signal=x16, **spec)      # an int16 signal that no pool holds

    for u in range(len(lens)):
        h_noisy = eng.pcmMix(pcm[u], sources, terms[u])
        h_wet = eng.signalConvolve(h_noisy, rooms[of[u]])
        h_x = eng.signalResample(h_wet, 22050, 16000)
        n16 = -(-(lens[u] + len(rooms[of[u]]) - 1) * 320 // 441)
        assert len(h_x) == n16 == int(x16k[1][u]) and int(steps[u]) == int(steps_lin[u]) == -(-n16 // 160), u
        assert same(rows_of(*noisy, True)[0][u], h_noisy) and same(rows_of(*wet, True)[0][u], h_wet) and same(rows_of(*x16k, True)[0][u], h_x), u
        assert same(rows_of(*wet16, True)[0][u], eng.signalConvolve(h_noisy, rooms[of[u]], dtype=np.int16)), u
        h_x16 = eng.signalResample(h_wet, 22050, 16000, dtype=np.int16)
        assert same(rows_of(*x16, True)[0][u], h_x16), u
        g = rows_of(lin, steps_lin, True)[0][u]
        assert np.array_equal(g.view(np.uint64), eng.signalSpectrogram(h_x, **spec).view(np.uint64)), u
        assert np.array_equal(rows_of(mel16, steps_lin, True)[0][u].view(np.uint64), eng.signalSpectrogram(h_x16, **spec).view(np.uint64)), u
        g, w = rows_of(mel, steps, True)[0][u], eng.signalSpectrogram(h_x, log="ln", floor=1e-5, **spec)
        assert g.shape == w.shape and g.size > 0 and ulps(g, w).max() <= 4, u
    for out, second in (wet, x16k, wet16, x16):      # the padding of every stage is +0 on its bits
        for z in rows_of(out, second, True)[1]:
            assert not z.view(np.uint32 if z.dtype == np.float32 else np.uint16).any()
    bp.close()


# ---- padding is never signal ---------------------------------------------------------------------------------------------------------------
def poison(n, npt):
    """n elements of NaN and 1e30 bit patterns."""
    raw = np.empty(-(-n * np.dtype(npt).itemsize // 8) * 2 + 2, np.float32)
    raw[0::2], raw[1::2] = np.nan, 1e30
    return raw.view(npt)[:n].copy()


def edge_rows(lens, npt, seed):
    rng = np.random.default_rng(seed)
    if npt == np.int16:
        return [rng.integers(-32768, 32768, L).astype(np.int16) for L in lens]
    return [rng.uniform(-2.0, 2.0, L).astype(np.float32) for L in lens]


def lay_out(rows, npt, stride, fill, shift):
    """The rows in one host array as a signal lays them out, between guards, `shift` elements past a 16-byte boundary: -> (array, first element,
    extent).  Padded (stride > 0): the rows' remainders hold `fill`; packed: back to back.  The guards hold `fill` too."""
    lens = [len(r) for r in rows]
    body = len(rows) * stride if stride else sum(lens)
    a = fill(GUARD + shift + body + GUARD, npt)
    at = GUARD + shift
    for i, r in enumerate(rows):
        a[at:at + len(r)] = r
        at += stride if stride else len(r)
    return a, GUARD + shift, np.array(lens if stride else np.concatenate([[0], np.cumsum(lens)]), np.int64)


def record(sp, ptr, fmt, n, stride, extent):
    rec = np.zeros(1, sp._signalDtype)
    rec["data"], rec["format"], rec["nRows"], rec["rowStride"], rec["extent"] = ptr, fmt, n, stride, 0 if extent is None else extent.ctypes.data
    return rec


class Exports:
    """The three C entry points with one set of arguments each: call(kind, signal record pointer, rows, output pointer, output format,
    output stride) -> elements; lengths(kind, lens) -> the rows' output lengths."""
    def __init__(self, L, bp):
        import nvspeechplayer_amd as eng
        self.L, self.bp = L, bp
        self.irs = [decaying(K, 80 + K) for K in TAPS]
        self.flat, self.start = np.concatenate(self.irs), np.concatenate([[0], np.cumsum(TAPS)]).astype(np.int64)
        self.bank = eng.melFilterbank(16000, 64, 8)

    def irOf(self, n):
        return (np.arange(n) % len(TAPS)).astype(np.int64)

    def lengths(self, kind, lens):
        lens = np.asarray(lens, np.int64)
        if kind == "convolved":
            return lens + np.array(TAPS)[self.irOf(len(lens))] - 1
        if kind == "spectrogram":
            return -(-lens // 48) * 8
        up, down = {"resampled": (320, 441), "up": (441, 320), "half": (1, 2), "same": (1, 1)}[kind]
        return -(-lens * up // down)

    def call(self, kind, sig, rows, out, fmt=1, stride=0, n=None, batch=0, stream=None, src=None):
        p = lambda a: None if a is None else a.ctypes.data
        h = self.bp._h if batch == 0 else batch
        n = (0 if rows is None else len(rows)) if n is None else n
        if kind == "convolved":
            of = self.irOf(n if rows is not None or n else 16)
            return self.L.speechPlayer_batch_exportConvolvedOf(h, sig, p(rows), n, p(self.flat), p(self.start), len(TAPS), p(of), 1, out, fmt, stride, stream)
        if kind == "spectrogram":
            return self.L.speechPlayer_batch_exportSpectrogramOf(h, sig, p(rows), n, 64, 48, 0, None, p(self.bank), 8, 2, 0.0, 0.0, out, fmt, stride, stream)
        a, b = {"resampled": (22050, 16000), "up": (16000, 22050), "half": (32000, 16000), "same": (16000, 16000)}[kind]
        return self.L.speechPlayer_batch_exportResampledOf(h, sig, p(rows), n, a if src is None else src, b, 6, 0.99, 0, 0.0, out, fmt, stride, stream)


KINDS = ["convolved", "resampled", "up", "half", "same", "spectrogram"]


@pytest.fixture(scope="module")
def bare():
    """A player that was never set."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    bp = eng.BatchPlayer(22050)
    yield Exports(_native.load(), bp)
    bp.close()


def run(ex, kind, host, first, fmt_in, n, stride, extent, rows, out_fmt, out_shift=0):
    """One export of a laid-out signal into a buffer with guards either side: -> the whole buffer, guards included."""
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    dev = "cuda:%d" % ex.bp.device
    data = torch.from_numpy(host.view(np.int32 if host.dtype == np.float32 else np.int16)).to(dev)
    assert data.data_ptr() % 16 == 0
    lens = np.asarray(extent if stride else np.diff(extent))[rows]
    elements = int(ex.lengths(kind, lens).sum())
    np_out = {("spectrogram", 0): np.float64, ("spectrogram", 1): np.float32}.get((kind, out_fmt), np.float32 if out_fmt else np.int16)
    dtype = {np.float64: torch.float64, np.float32: torch.float32, np.int16: torch.int16}[np_out]
    buf = torch.full((GUARD + out_shift + elements + GUARD,), -7, dtype=dtype, device=dev)
    rec = record(sp, data.data_ptr() + first * data.element_size(), fmt_in, n, stride, extent)
    got = ex.call(kind, rec.ctypes.data, rows, buf.data_ptr() + (GUARD + out_shift) * buf.element_size(), fmt=out_fmt)
    assert got == elements, (kind, got, elements, ex.L.speechPlayer_lastError())
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.all(out[:GUARD + out_shift] == -7) and np.all(out[GUARD + out_shift + elements:] == -7), kind
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("npt", [np.int16, np.float32])
def test_padding_is_never_signal(bare, kind, npt):
    """The edge rows in a padded signal whose remainder, and in a packed one whose guards, hold NaN and 1e30 bit patterns give what the
    same rows beside zeros give -- and what the host statement gives; the signal 16-byte aligned and one element past a boundary."""
    import nvspeechplayer_amd as eng
    zeros = lambda n, t: np.zeros(n, t)
    fmt_in = 0 if npt == np.int16 else 1
    for lens, stride in ((EDGES, 2 * T + 5), (PACKED_EDGES, 0)):
        rows = edge_rows(lens, npt, len(lens))
        sel = np.arange(len(lens), dtype=np.int64)[::-1].copy()
        for shift in (0, 1):
            for out_fmt in (1, 0):
                host, first, extent = lay_out(rows, npt, stride, poison, shift)
                dirty = run(bare, kind, host, first, fmt_in, len(lens), stride, extent, sel, out_fmt, out_shift=shift)
                host, first, extent = lay_out(rows, npt, stride, zeros, shift)
                clean = run(bare, kind, host, first, fmt_in, len(lens), stride, extent, sel, out_fmt, out_shift=shift)
                assert dirty.dtype == clean.dtype and np.array_equal(dirty.view(np.uint8), clean.view(np.uint8)), (kind, stride, shift, out_fmt)
                assert np.all(np.isfinite(dirty.astype(np.float64)))
                # ... and the statement's bits, row by row (packed output)
                at = GUARD + shift
                for at_row, i in enumerate(sel):      # (irOf is per OUTPUT row)
                    if kind == "convolved":
                        w = eng.signalConvolve(rows[i], bare.irs[int(bare.irOf(len(sel))[at_row])], dtype=np.float32 if out_fmt else np.int16)
                    elif kind == "spectrogram":
                        w = eng.signalSpectrogram(rows[i], nFft=64, hop=48, bank=bare.bank).reshape(-1)
                        w = w.astype(np.float32) if out_fmt else w
                    else:
                        a, b = {"resampled": (22050, 16000), "up": (16000, 22050), "half": (32000, 16000), "same": (16000, 16000)}[kind]
                        w = eng.signalResample(rows[i], a, b, dtype=np.float32 if out_fmt else np.int16)
                    g = dirty[at:at + len(w)]
                    assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (kind, stride, shift, out_fmt, int(i))
                    at += len(w)


# ---- independent of the shared code, on players that were never synthesised -----------------------------------------------------------------
@pytest.mark.parametrize("state", ["never set", "set, not synthesised"])
def test_float_signals_against_numpy_float64(state):
    """The Python interface on a player that was never set, and on one that is set but not synthesised: float32 signals no PCM gives, within
    the bounds of the three host test modules."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    if state != "never set":
        set_host(bp, compared("plain").b)
    dev = "cuda:%d" % bp.device
    xs = list(x_signals(2 * T + 1, 3).values()) + [x_signals(T - 1, 4)["noise"], np.zeros(0, np.float32)]
    lens = [len(x) for x in xs]
    padded = torch.zeros((len(xs), max(lens)), dtype=torch.float32)
    for i, x in enumerate(xs):
        padded[i, :len(x)] = torch.from_numpy(x)
    signal = (padded.to(dev), torch.tensor(lens))
    for K in TAPS:
        h = decaying(K, 90 + K)
        out, second = bp.convolvedTensor(h, signal=signal, padded=False)
        for x, g in zip(xs, rows_of(out, second, False)[0]):
            want, mag = conv_reference(x, h) if len(x) else (np.zeros(K - 1), np.zeros(K - 1))      # (a row of nothing has its tail: K - 1 zeros)
            assert g.shape == want.shape and np.all(np.abs(g.astype(np.float64) - want) <= gamma(K) * mag), K
    for src, dst in RATES:
        table, up, down = eng.resampleKernel(src, dst, **FILTERS[0])
        out, second = bp.resampledTensor(dst, signal=signal, signalRate=src, padded=False, **FILTERS[0])
        for x, g in zip(xs, rows_of(out, second, False)[0]):
            want, mag = res_reference(x, table, up, down)
            assert g.shape == want.shape and np.all(np.abs(g.astype(np.float64) - want) <= res_gamma(table.shape[1]) * mag), (src, dst)
    for n in (64, 256):
        out, second = bp.spectrogramTensor(nFft=n, hop=n // 4, phase=3, power=1, dtype=torch.float64, signal=signal, padded=False)
        for x, g in zip(xs, rows_of(out, second, False)[0]):
            check_spectrum(g, x, n, n // 4, 3)
    # equal rates: the samples, -0.0 included; the batch's rate is the default
    y = padded.clone()
    y[0, 5] = -0.0
    out, second = bp.resampledTensor(22050, signal=(y.to(dev), torch.tensor(lens)))
    assert torch.equal(out.cpu().view(torch.int32)[0, :lens[0]], y.view(torch.int32)[0, :lens[0]]) and list(second.numpy()) == lens
    if state != "never set":      # the pool exports still need their synthesis, and the player is as usable as before
        with pytest.raises(RuntimeError, match="not been synthesised"):
            bp.convolvedTensor(decaying(5, 1))
        bp.synthesize()
        a, la = bp.pcmTensor()
        b, lb = bp.convolvedTensor(np.ones(1, np.float32), tail=False, signal=(a, la))
        assert torch.equal(a, b) and torch.equal(la, lb)
    bp.close()


def test_seventeen_in_flight(bare):
    """More exports than slots, no host wait between them."""
    import torch
    import nvspeechplayer_amd as eng
    bp = bare.bp
    x = x_signals(T + 1, 9)["noise"]
    signal = (torch.from_numpy(x).to("cuda:%d" % bp.device), torch.tensor([0, len(x)]))
    outs = [bp.convolvedTensor(decaying(5, i), signal=signal)[0] if i % 2 else bp.resampledTensor(16000, signal=signal)[0] for i in range(17)]
    torch.cuda.synchronize()
    for i, out in enumerate(outs):
        assert same(out.cpu().numpy()[0], eng.signalConvolve(x, decaying(5, i)) if i % 2 else eng.signalResample(x, 22050, 16000)), i


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["convolved", "resampled", "same", "spectrogram"])
def test_refusals_write_nothing_and_name_the_row(bare, kind):
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    L, bp = bare.L, bare.bp
    dev = "cuda:%d" % bp.device
    n, stride = 4, 300
    lens = np.array([300, 0, 7, 120], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    whole = torch.full((8192,), -7.0, dtype=torch.float32, device=dev)      # the signal at its head, the output behind it
    data, out = whole[:n * stride], whole[4096:]
    sentinel = whole.clone()
    host = np.zeros(n * stride, np.float32)
    rows = np.arange(n, dtype=np.int64)
    seg = next(g for g in torch.cuda.memory_snapshot() if g["address"] <= whole.data_ptr() < g["address"] + g["total_size"])
    near_end = seg["address"] + seg["total_size"] - 4 * (3 * stride + 120) + 16      # four elements short of the rows' need
    assert near_end >= seg["address"] and near_end % 4 == 0

    def call(data=data.data_ptr(), fmt=1, nRows=n, rowStride=stride, extent=lens, sig=True, rows=rows, out=out.data_ptr(), **kw):
        rec = record(sp, data, fmt, nRows, rowStride, extent)
        return bare.call(kind, rec.ctypes.data if sig else None, rows, out, stride=0, **kw)

    name = {"convolved": b"exportConvolvedOf", "resampled": b"exportResampledOf", "same": b"exportResampledOf", "spectrogram": b"exportSpectrogramOf"}[kind]
    cases = dict(
        no_signal=(dict(sig=False), b"no signal"), format_2=(dict(fmt=2), b"format 2"), format_negative=(dict(fmt=-1), b"format -1"),
        nRows_negative=(dict(nRows=-1), b"nRows -1"), rowStride_negative=(dict(rowStride=-1), b"rowStride -1"), no_extent=(dict(extent=None), b"extent"),
        length_negative=(dict(extent=np.array([300, 0, -1, 120], np.int64)), b"row 2"), length_above_stride=(dict(extent=np.array([300, 301, 7, 120], np.int64)), b"row 1"),
        offsets_late=(dict(rowStride=0, extent=offsets + 1), b"extent[0] = 1"), offsets_down=(dict(rowStride=0, extent=np.array([0, 300, 299, 307, 427], np.int64)), b"row 1"),
        length_huge=(dict(rowStride=1 << 45, extent=np.array([1, 1, 1, (1 << 44) + 1], np.int64)), b"row 3"),
        offset_huge=(dict(rowStride=0, extent=np.array([0, 1, 2, 3, (1 << 44) + 4], np.int64)), b"row 3"),
        packed_total=(dict(rowStride=0, nRows=(1 << 16) + 1, extent=np.arange((1 << 16) + 2, dtype=np.int64) << 44), b"past 2^60 elements"),
        host_memory=(dict(data=host.ctypes.data), b"signal"), no_data=(dict(data=0), b"signal without data"), misaligned=(dict(data=data.data_ptr() + 2), b"aligned"),
        misaligned_int16=(dict(data=data.data_ptr() + 1, fmt=0), b"aligned"), too_small=(dict(data=near_end), b"allocation"),
        row_beyond=(dict(rows=np.array([0, 4], np.int64)), b"rows[1] = 4"), row_negative=(dict(rows=np.array([3, 2, -1], np.int64)), b"rows[2] = -1"),
        rows_negative_count=(dict(n=-1), b"rows"), overlap_head=(dict(out=data.data_ptr()), b"overlaps"), overlap_tail=(dict(out=data.data_ptr() + 4 * (3 * stride + 116)), b"overlaps"),
        no_batch=(dict(batch=None), b"no batch"), no_output=(dict(out=None), b"no output"))
    if kind in ("resampled", "same"):
        cases.update(src_zero=(dict(src=0), b"sample rates"), src_negative=(dict(src=-16000), b"sample rates"))
    for tag, (kw, word) in cases.items():
        assert call(**kw) == -1, (kind, tag)
        text = L.speechPlayer_lastError()
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and name in text and word in text, (kind, tag, text)
        torch.cuda.synchronize()
        assert torch.equal(whole.view(torch.int32), sentinel.view(torch.int32)), (kind, tag)
    # nothing to write needs neither data nor output; rows of nothing are not read; and the player is as usable as before
    assert call(rows=rows[:0], out=None) == 0 and L.speechPlayer_lastErrorCode() == 0
    if kind != "convolved":
        assert call(data=0, extent=np.zeros(n, np.int64), out=None) == 0 and L.speechPlayer_lastErrorCode() == 0
    whole[:n * stride] = torch.from_numpy(x_signals(n * stride, 7)["noise"]).to(dev)
    want = int(bare.lengths(kind, lens).sum())
    assert call() == want and call(rowStride=0, extent=offsets[:3], nRows=2, rows=rows[:2]) == int(bare.lengths(kind, lens[:2]).sum())
    torch.cuda.synchronize()
    assert torch.equal(whole[:4096].view(torch.int32), torch.cat([whole[:n * stride], sentinel[n * stride:4096]]).view(torch.int32))
