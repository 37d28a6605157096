"""The mix onto a caller's device signal and the power of its rows (include/speechPlayer_batch.h: speechPlayer_batch_exportMixedOf /
exportPowerOf; BatchPlayer.mixedTensor / powerTensor with signal=; csrc/klatt_sigpower.h, klatt_mix.h): the pool handed back as a signal
gives the pool export's bits; float32 and int16 signals equal the host statements (signalMix, signalPower) bit for bit in every layout;
what lies beside a row is never read; the chain in the standard order -- room, then noise at an SNR against the wet speech, 16 kHz, log-mel --
equals the composition of the host statements; players never set; seventeen in flight; every refusal.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_convolve_host import decaying
from tests.test_gpu_mix import single_frames
from tests.test_gpu_resample import rows_of, same
from tests.test_gpu_signal import lay_out, poison, record
from tests.test_gpu_spectrogram import player
from tests.test_mix_host import bank, clip_power, gain_of
from tests.test_signal_mix_host import bits64, seeded_row
from tests.test_spectrogram_host import ulps

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
B = 2048
LENS = [0, 1, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4100, 8 * B + 1, 500]      # the last row is all zeros
ZERO_ROW, LONG_ROW = 11, 9
SEL = list(range(len(LENS)))[::-1] + [3, 3, 10, ZERO_ROW]      # out of order, with repeats: each repeat has its own terms


def make_rows(npt):
    """The rows of the test signals: values up to 2^16 (float32) or the whole int16 range, and one all-zero row."""
    if npt == np.float32:
        rows = [seeded_row(L, k) for k, L in enumerate(LENS)]
    else:
        rng = np.random.default_rng(31)
        rows = [rng.integers(-32768, 32768, L).astype(np.int16) for L in LENS]
    rows[ZERO_ROW] = np.zeros(LENS[ZERO_ROW], npt)
    return rows


def term_pairs(i, r, nClips):
    """The terms of output row i, made from row r of the signal: -> (the device's terms, the host statement's, the speech gain).  The host's
    sources are the clips followed by the rows, so utterance=u is source nClips + u there."""
    from nvspeechplayer_amd import MixTerm as M
    pairs = []

    def clip(k, **kw):
        pairs.append((M(noise=k, **kw), M(noise=k, **kw)))

    def row(u, **kw):
        pairs.append((M(utterance=u, **kw), M(utterance=nClips + u, **kw)))
    kind = i % 4
    if kind == 0:      # looped clips shorter and longer than a tile, at an SNR and at a gain
        clip(1, snr=10.0, offset=2); clip(2, gain=0.25, offset=1022); clip(5, snr=3.0, offset=7000)
    elif kind == 1:    # a row placed once at positive and negative offsets
        row(LONG_ROW, snr=5.0, offset=5, loop=False); row(LONG_ROW, gain=-0.5, offset=-37, loop=False); row(7, snr=0.0, offset=1024, loop=False)
    elif kind == 2:    # the row itself, once and (where it has samples) looped; a silent source
        row(r, snr=0.0, offset=0, loop=False); row(ZERO_ROW, snr=10.0, offset=3)
        if LENS[r]:
            row(r, snr=6.0, offset=LENS[r] // 2)
    else:              # everything at once; a row looped from its last sample
        clip(3, snr=15.0, offset=100); row(LONG_ROW, snr=-3.0, offset=LENS[LONG_ROW] - 1); clip(0, gain=-0.125); row(5, snr=20.0, offset=-1000, loop=False)
    return [p[0] for p in pairs], [p[1] for p in pairs], (1.0, 0.5, -1.0, 0.75)[i % 4]


def as_signal(rows, padded, shift, dev, fill=0):
    """The rows as a device signal, `shift` elements past the start of their allocation: -> ((tensor, lengths or offsets), the base tensor)."""
    import torch
    npt = rows[0].dtype
    lens = [len(r) for r in rows]
    stride = max(lens) + 3 if padded else 0
    body = len(rows) * stride if padded else sum(lens)
    host = np.full(shift + body, fill, npt)
    at = shift
    for r in rows:
        host[at:at + len(r)] = r
        at += stride if padded else len(r)
    base = torch.from_numpy(host).to(dev)
    view = base[shift:]
    if padded:
        return (view.view(len(rows), stride), torch.tensor(lens)), base
    return (view, torch.tensor(np.concatenate([[0], np.cumsum(lens)]))), base


@pytest.fixture(scope="module")
def bare():
    """A player that was never set, with the shared noise bank."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    clips = bank()
    bp.setNoiseBank(clips)
    yield bp, clips
    bp.close()


@pytest.fixture(scope="module")
def statements(bare):
    """The host statements of every output row of SEL, once: {(input dtype, output dtype): [(mixed, gains)]} and the rows themselves."""
    import nvspeechplayer_amd as eng
    _, clips = bare
    want, rows = {}, {}
    for npt in (np.float32, np.int16):
        rows[npt] = make_rows(npt)
        sources = clips + rows[npt]
        for out in (np.float32, np.int16):
            want[npt, out] = []
            for i, r in enumerate(SEL):
                _, host, sg = term_pairs(i, r, len(clips))
                want[npt, out].append(eng.signalMix(rows[npt][r], sources, host, speechGain=sg, dtype=out, gains=True))
    return want, rows


# ---- the pool as a signal ---------------------------------------------------------------------------------------------------------------------
def test_the_pool_as_a_signal_gives_the_pool_exports_bits():
    import torch
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    lens = [3, 1023, 1025, 2 * B + 1, 700]
    bp, pcm = player(single_frames(lens))
    bp.setNoiseBank(bank())
    terms = [[M(noise=5, snr=10.0, offset=7 * u), M(utterance=(u + 1) % len(lens), snr=3.0, offset=-5, loop=False), M(utterance=u, snr=0.0, loop=False),
              M(utterance=3, gain=0.25, offset=11)] for u in range(len(lens))]
    sg = [1.0, 0.5, -1.0, 0.0, 2.0]
    for in_padded in (True, False):
        signal = bp.pcmTensor(dtype=torch.int16, padded=in_padded)
        for padded in (True, False):
            for dtype, it in ((torch.float32, torch.int32), (torch.int16, torch.int16)):
                a, la, ga, sa = bp.mixedTensor(terms, speechGain=sg, dtype=dtype, padded=padded, gains=True)
                b, lb, gb, sb = bp.mixedTensor(terms, speechGain=sg, dtype=dtype, padded=padded, gains=True, signal=signal)
                assert torch.equal(la, lb) and torch.equal(sa, sb) and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it)), (in_padded, padded, dtype)
                assert torch.equal(ga.view(torch.int32), gb.view(torch.int32)) and bool((ga != 0).any()), (in_padded, padded, dtype)
                c, lc = bp.mixedTensor(terms, speechGain=sg, dtype=dtype, padded=padded, signal=signal)
                assert torch.equal(c.view(it), a.view(it)) and torch.equal(lc, la)
        # the powers: P of the int16 signal is mix_power of the pool's exact sum
        sums, _ = bp.powerTensor()
        powers, plens = bp.powerTensor(signal=signal)
        want = [float(int(s)) / float(L) / 1073676289.0 for s, L in zip(sums.cpu().numpy(), lens)]
        assert [bits64(p) for p in powers.cpu().numpy()] == [bits64(w) for w in want] and list(plens.cpu().numpy()) == lens
    bp.close()


# ---- float32 and int16 signals against the host statement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("npt", [np.float32, np.int16])
@pytest.mark.parametrize("in_padded", [True, False])
def test_signals_against_the_host_statement(bare, statements, npt, in_padded):
    """Every row's mixture and gains are signalMix's bits: both output formats, padded and packed, the data 0 .. 3 elements past an aligned
    address, rows chosen out of order and with repeats."""
    import torch
    bp, clips = bare
    want, rows = statements
    dev = "cuda:%d" % bp.device
    terms = [term_pairs(i, r, len(clips))[0] for i, r in enumerate(SEL)]
    sg = [term_pairs(i, r, len(clips))[2] for i, r in enumerate(SEL)]
    for shift in range(4):
        signal, base = as_signal(rows[npt], in_padded, shift, dev, fill=7)
        assert (signal[0].data_ptr() - base.data_ptr()) == shift * base.element_size()
        for out_np, dtype in ((np.float32, torch.float32), (np.int16, torch.int16)):
            for padded in (True, False):
                out, second, g, start = bp.mixedTensor(terms, speechGain=sg, utterances=SEL, dtype=dtype, padded=padded, gains=True, signal=signal)
                got, pad = rows_of(out, second, padded)
                g, start = g.cpu().numpy(), start.numpy()
                for i, r in enumerate(SEL):
                    w, wg = want[npt, out_np][i]
                    assert same(got[i], w), (shift, out_np, padded, i, r)
                    assert np.array_equal(g[start[i]:start[i + 1]].view(np.uint32), wg.view(np.uint32)), (shift, out_np, padded, i, r, g[start[i]:start[i + 1]], wg)
                for z in pad:
                    assert not z.view(np.uint32 if z.dtype == np.float32 else np.uint16).any()
    # a silent row or a silent source gives gain +0, and the case list did hold SNR gains that are not
    flat = np.concatenate([wg for _, wg in want[npt, np.float32]])
    assert (flat == 0).any() and (flat > 0).any()


@pytest.mark.parametrize("npt", [np.float32, np.int16])
def test_power_tensor_of_a_signal(bare, statements, npt):
    """powerTensor(signal=) equals signalPower bit for bit, repeats included, whichever rows a call chooses."""
    import nvspeechplayer_amd as eng
    bp, _ = bare
    _, rows = statements
    dev = "cuda:%d" % bp.device
    want = [bits64(eng.signalPower(r)) for r in rows[npt]]
    assert want[ZERO_ROW] == 0 and want[0] == 0 and len(set(want)) > 8
    for padded in (True, False):
        for shift in (0, 1, 3):
            signal, _ = as_signal(rows[npt], padded, shift, dev, fill=9)
            p, lens = bp.powerTensor(signal=signal)
            assert [bits64(v) for v in p.cpu().numpy()] == want and list(lens.cpu().numpy()) == LENS, (padded, shift)
            for sel in (SEL, [10, 10, 0, 4], [2]):
                p, lens = bp.powerTensor(utterances=sel, signal=signal)
                assert [bits64(v) for v in p.cpu().numpy()] == [want[r] for r in sel] and list(lens.cpu().numpy()) == [LENS[r] for r in sel], (padded, shift, sel)


# ---- padding is never signal ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npt", [np.float32, np.int16])
def test_padding_is_never_signal(bare, statements, npt):
    """NaN, inf and 1e30 bit patterns in a padded signal's remainders, in the guards and in unchosen neighbouring rows change no bit of the
    powers, the gains or the output."""
    import torch
    bp, clips = bare
    want, rows = statements
    dev = "cuda:%d" % bp.device
    named = {LONG_ROW, 7, 5, ZERO_ROW}                       # the rows a term of term_pairs may name
    chosen = [r for r in SEL if r not in (6, 8)]             # rows 6 and 8 are neither chosen nor named: they hold poison
    index = [i for i, r in enumerate(SEL) if r not in (6, 8)]
    assert not named & {6, 8}

    def nasty(n, t):
        a = poison(n, t)
        if t == np.float32:
            a[2::5] = np.inf
        return a
    results = []
    for fill in (nasty, lambda n, t: np.zeros(n, t)):
        per = []
        for stride, shift in ((max(LENS) + 5, 1), (0, 2)):
            laid = [r if k not in (6, 8) else fill(len(r), npt) for k, r in enumerate(rows[npt])]
            host, first, extent = lay_out(laid, npt, stride, fill, shift)
            base = torch.from_numpy(host.view(np.int32 if npt == np.float32 else np.int16)).to(dev).view(torch.float32 if npt == np.float32 else torch.int16)
            body = base[first:first + (len(LENS) * stride if stride else sum(LENS))]
            signal = (body.view(len(LENS), stride), torch.tensor(LENS)) if stride else (body, torch.from_numpy(extent))
            terms = [term_pairs(i, SEL[i], len(clips))[0] for i in index]
            sg = [term_pairs(i, SEL[i], len(clips))[2] for i in index]
            out, second, g, start = bp.mixedTensor(terms, speechGain=sg, utterances=chosen, padded=False, gains=True, signal=signal)
            p, _ = bp.powerTensor(utterances=chosen, signal=signal)
            got = rows_of(out, second, False)[0]
            for at, i in enumerate(index):
                assert same(got[at], want[npt, np.float32][i][0]), (stride, i)
            per.append((out.cpu().numpy().tobytes(), g.cpu().numpy().tobytes(), p.cpu().numpy().tobytes()))
            assert np.isfinite(out.cpu().numpy()).all() and np.isfinite(p.cpu().numpy()).all()
        results.append(per)
    assert results[0] == results[1]


# ---- the chain in the standard order ---------------------------------------------------------------------------------------------------------
def test_the_chain_in_the_standard_order():
    """convolvedTensor -> mixedTensor(signal=wet, noise at 5 dB) -> resampledTensor(16000, signal=) -> spectrogramTensor(signal=): every
    linear value bit for bit, the log-mel within the bar of the existing chain test (4 ulp in float64), and the gain label is mix_gain of
    the wet row's signalPower."""
    import torch
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    lens = [3, 1023, 1025, 2 * B + 1]
    bp, pcm = player(single_frames(lens))
    clips = bank()
    bp.setNoiseBank(clips)
    big = [k for k, c in enumerate(clips) if len(c) > 100 and c.any()]
    rooms, of = [decaying(K, 60 + K) for K in (1, 5, 1025)], [2, 0, 1, 2]
    terms = [[M(noise=big[u % len(big)], snr=5.0, offset=7 * u)] for u in range(len(lens))]
    spec = dict(nFft=256, hop=160, bank=eng.melFilterbank(16000, 256, 20))

    wet = bp.convolvedTensor(rooms, irOf=of)
    noisy, nlens, gains, _ = bp.mixedTensor(terms, gains=True, signal=wet)
    x16k = bp.resampledTensor(16000, signal=(noisy, nlens))
    mel, steps = bp.spectrogramTensor(log="ln", floor=1e-5, dtype=torch.float64, signal=x16k, **spec)
    lin, steps_lin = bp.spectrogramTensor(dtype=torch.float64, signal=x16k, **spec)
    wet_powers, _ = bp.powerTensor(signal=wet)
    gains = gains.cpu().numpy()
    for u in range(len(lens)):
        h_wet = eng.signalConvolve(pcm[u], rooms[of[u]])
        h_noisy, h_g = eng.signalMix(h_wet, clips, terms[u], gains=True)
        h_x = eng.signalResample(h_noisy, 22050, 16000)
        assert same(rows_of(*wet, True)[0][u], h_wet) and same(rows_of(noisy, nlens, True)[0][u], h_noisy) and same(rows_of(*x16k, True)[0][u], h_x), u
        assert int(nlens[u]) == lens[u] + len(rooms[of[u]]) - 1
        label = gain_of(eng.signalPower(h_wet), clip_power(clips[terms[u][0].source]), 5.0)
        assert gains[u:u + 1].view(np.uint32)[0] == h_g.view(np.uint32)[0] == np.array([label], np.float32).view(np.uint32)[0] and (label > 0) == (u > 0), u      # (utterance 0 is three samples of silence: no SNR)
        assert bits64(wet_powers.cpu().numpy()[u]) == bits64(eng.signalPower(h_wet)), u
        g = rows_of(lin, steps_lin, True)[0][u]
        assert np.array_equal(g.view(np.uint64), eng.signalSpectrogram(h_x, **spec).view(np.uint64)), u
        g, w = rows_of(mel, steps, True)[0][u], eng.signalSpectrogram(h_x, log="ln", floor=1e-5, **spec)
        assert g.shape == w.shape and g.size > 0 and ulps(g, w).max() <= 4, u
    bp.close()


# ---- a batch never set; seventeen in flight ------------------------------------------------------------------------------------------------------
def test_a_batch_never_set_and_seventeen_in_flight(bare, statements):
    """The exports above ran on a player that was never set: no synthesis.  More calls than slots, no host wait between them."""
    import torch
    import nvspeechplayer_amd as eng
    bp, clips = bare
    want, rows = statements
    assert bp.nUtterances == 0
    dev = "cuda:%d" % bp.device
    signal, _ = as_signal(rows[np.float32], False, 1, dev)
    M = eng.MixTerm
    outs = []
    for k in range(17):
        if k % 2:
            outs.append(bp.powerTensor(utterances=[10, k % 12], signal=signal)[0])
        else:
            outs.append(bp.mixedTensor([[M(noise=5, snr=float(k), offset=k), M(utterance=10, snr=0.0, offset=3)]], utterances=[LONG_ROW], signal=signal)[0])
    torch.cuda.synchronize()
    sources = clips + rows[np.float32]
    for k, out in enumerate(outs):
        if k % 2:
            assert [bits64(v) for v in out.cpu().numpy()] == [bits64(eng.signalPower(rows[np.float32][r])) for r in (10, k % 12)], k
        else:
            w = eng.signalMix(rows[np.float32][LONG_ROW], sources, [M(noise=5, snr=float(k), offset=k), M(utterance=len(clips) + 10, snr=0.0, offset=3)])
            assert same(out.cpu().numpy()[0], w), k


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_name_the_row_or_term(bare):
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    from nvspeechplayer_amd import speechPlayer as sp
    L = _native.load()
    bp, clips = bare
    nobank = eng.BatchPlayer(22050)
    dev = "cuda:%d" % bp.device
    n, stride = 4, 300
    lens = np.array([300, 0, 7, 120], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    whole = torch.full((8192,), -7.0, dtype=torch.float32, device=dev)      # the signal at its head, the output and the gains behind it
    data, out, gains = whole[:n * stride], whole[4096:6144], whole[6144:]
    sentinel = whole.clone()
    host_gains = np.zeros(16, np.float32)
    rows = np.arange(n, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data

    def term(kind=1, levelKind=0, source=0, offset=0, level=10.0, loop=0):
        return (kind, levelKind, source, offset, level, loop, 0)

    def call(terms=(term(),), start=None, data=data.data_ptr(), fmt=1, nRows=n, rowStride=stride, extent=lens, rows=rows, out=out.data_ptr(), gains=gains.data_ptr(),
             batch=bp, speech=None, outFmt=1, outStride=0, power=False):
        rec = record(sp, data, fmt, nRows, rowStride, extent)
        flat = np.array(list(terms), sp.mixTermDtype).reshape(-1)
        start = np.array([0] + [len(flat)] * len(rows) if start is None else start, np.int64)
        if power:
            return L.speechPlayer_batch_exportPowerOf(batch._h, rec.ctypes.data, p(rows), len(rows), out, None)
        return L.speechPlayer_batch_exportMixedOf(batch._h, rec.ctypes.data, p(rows), len(rows), p(flat) if len(flat) else None, p(start), p(speech), gains, out, outFmt,
                                                  outStride, None)

    cases = dict(
        overlap_head=(dict(out=data.data_ptr()), b"overlaps"), overlap_tail=(dict(out=data.data_ptr() + 4 * (3 * stride + 116)), b"overlaps"),
        gains_overlap=(dict(gains=data.data_ptr() + 8), b"overlaps"), power_overlap=(dict(power=True, out=data.data_ptr() + 64), b"overlaps"),
        source_beyond=(dict(terms=(term(source=0), term(source=4))), b"row 0, term 1: source 4 is not a row of the signal (4)"),
        source_negative=(dict(terms=(term(source=-1),)), b"row 0, term 0: source -1 is not a row of the signal"),
        source_later_row=(dict(terms=(term(), term(source=9)), start=[0, 1, 1, 1, 2]), b"row 3, term 0: source 9 is not a row of the signal"),
        no_bank=(dict(terms=(term(kind=0),), batch=nobank), b"row 0, term 0: clip 0, and no noise bank is set"),
        clip_beyond=(dict(terms=(term(kind=0, source=len(clips)),)), b"is not in the bank"),
        offsets_late=(dict(rowStride=0, extent=offsets + 1), b"extent[0] = 1"), offsets_down=(dict(rowStride=0, extent=np.array([0, 300, 299, 307, 427], np.int64)), b"row 1"),
        gains_host=(dict(gains=host_gains.ctypes.data), b"exportMixedOf"), gains_misaligned=(dict(gains=gains.data_ptr() + 2), b"aligned"),
        looped_empty=(dict(terms=(term(source=1, loop=1),)), b"row 0, term 0: a looped source of length 0"), snr_nan=(dict(terms=(term(level=np.nan),)), b"an SNR of nan dB"),
        speech_gain=(dict(speech=np.array([1, 1, np.inf, 1], np.float32)), b"row 2: speechGain inf"), terms_start=(dict(start=[0, 1, 0, 1, 1]), b"termStart"),
        row_beyond=(dict(rows=np.array([0, 4], np.int64)), b"rows[1] = 4"), format_2=(dict(outFmt=2), b"format 2"), signal_format=(dict(fmt=2), b"signal format 2"),
        partials_cap=(dict(rowStride=1 << 40, extent=np.array([1 << 36, 0, 0, 0], np.int64)), b"33554432 blocks of 2048 samples (at most 2^24 in one call)"),
        power_cap=(dict(power=True, rowStride=1 << 40, extent=np.array([0, 0, (1 << 35) + 1, 0], np.int64)), b"16777217 blocks of 2048 samples"),
        stride_short=(dict(outStride=299), b"rowStride 299"), no_output=(dict(out=None), b"no output"), misaligned=(dict(data=data.data_ptr() + 2), b"aligned"))
    for tag, (kw, word) in cases.items():
        assert call(**kw) == -1, tag
        text = L.speechPlayer_lastError()
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and (b"exportPowerOf" if kw.get("power") else b"exportMixedOf") in text and word in text, (tag, text)
        torch.cuda.synchronize()
        assert torch.equal(whole.view(torch.int32), sentinel.view(torch.int32)), tag
    # nothing to write needs neither data nor output; and the player is as usable as before
    assert call(rows=rows[:0], out=None, gains=None) == 0 and L.speechPlayer_lastErrorCode() == 0
    x = seeded_row(n * stride, 3)
    whole[:n * stride] = torch.from_numpy(x).to(dev)
    assert call() == int(lens.sum()) and L.speechPlayer_lastErrorCode() == 0
    torch.cuda.synchronize()
    w, wg = eng.signalMix(x[:300], [x[:300]], [eng.MixTerm(utterance=0, snr=10.0, loop=False)], gains=True)
    assert same(out.cpu().numpy()[:300], w) and gains.cpu().numpy()[:1].view(np.uint32)[0] == wg.view(np.uint32)[0] and abs(float(wg[0]) - 10.0 ** -0.5) < 1e-6
    nobank.close()
