"""A batch's PCM mixed with noise clips and other utterances (include/speechPlayer_batch.h: speechPlayer_batch_exportMixed,
speechPlayer_batch_exportPower, speechPlayer_batch_setNoiseBank; BatchPlayer.mixedTensor, powerTensor, setNoiseBank; csrc/klatt_mix.h) against
the host's statement of the definition, speechPlayer_pcmMix applied to the PCM the engine reads back -- bit for bit, float32 and int16,
the gains included -- and, independently of the code the two share, against a numpy float64 sum within the bound of a chain of fused
multiply-adds.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_gpu_resample import rows_of, same
from tests.test_gpu_spectrogram import bits, player
from tests.test_gpu_timeline import set_host
from tests.test_mix_host import bank, case_terms, many_terms
from tests.test_stems_host import Stemmed, compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64
U = 2.0 ** -24
LENGTHS = [3, 1023, 1024, 1025, 2049, 5000]      # one request each: L = max(M, F + 1) + 1
SILENT, SPEECH = 6, 7


def eight():
    """The fixture: single-frame voiced utterances of 3, T - 1, T, T + 1, 2 T + 1 and 5000 samples, one silent utterance (a NULL frame) and
    one speech utterance of the plain batch (utterance 3: six frames, a few thousand samples)."""
    b = compared("plain").b
    voiced = [k for k in range(len(b["frames"])) if not b["isnull"][k]]
    frames = [np.asarray(b["frames"][voiced[i % len(voiced)]])[None, :] for i in range(len(LENGTHS))] + [np.asarray(b["frames"][voiced[0]])[None, :]]
    mins, fade, isnull = [L - 1 for L in LENGTHS] + [799], [1] * (len(LENGTHS) + 1), [0] * len(LENGTHS) + [1]
    k0, k1 = int(b["frame_start"][3]), int(b["frame_start"][4])
    frames.append(np.asarray(b["frames"][k0:k1]))
    mins += list(b["min"][k0:k1]); fade += list(b["fade"][k0:k1]); isnull += list(b["isnull"][k0:k1])
    start = list(range(len(LENGTHS) + 2)) + [len(LENGTHS) + 1 + k1 - k0]
    return dict(frame_start=np.array(start, np.int64), frames=np.ascontiguousarray(np.concatenate(frames)), min=np.array(mins, np.uint32),
                fade=np.array(fade, np.uint32), index=np.full(len(mins), -1, np.int32), isnull=np.array(isnull, np.uint8),
                seeds=np.arange(1, 9, dtype=np.uint32))


def single_frames(lens):
    """Single-frame voiced utterances of lens[i] samples."""
    b = compared("plain").b
    voiced = [k for k in range(len(b["frames"])) if not b["isnull"][k]]
    n = len(lens)
    return dict(frame_start=np.arange(n + 1, dtype=np.int64), frames=np.ascontiguousarray(np.stack([np.asarray(b["frames"][voiced[i % len(voiced)]]) for i in range(n)])),
                min=np.array([L - 1 for L in lens], np.uint32), fade=np.ones(n, np.uint32), index=np.full(n, -1, np.int32), isnull=np.zeros(n, np.uint8),
                seeds=np.arange(1, n + 1, dtype=np.uint32))


class Fixture:
    def __init__(self, mode=0, clips=True, batch=None):
        self.batch = eight() if batch is None else batch
        self.bp, self.pcm = player(self.batch, mode=mode)
        self.clips = bank()
        if clips:
            self.bp.setNoiseBank(self.clips)
        self.sources = self.clips + self.pcm      # the host statement's sources: utterance u is source len(clips) + u
        self.done = {}

    def host(self, u):
        return len(self.clips) + u

    def statement(self, key, u, terms, sg, npt):
        """speechPlayer_pcmMix of utterance u, computed once per key: -> (mixed, gains)."""
        import nvspeechplayer_amd as eng
        if (key, npt) not in self.done:
            self.done[(key, npt)] = eng.pcmMix(self.pcm[u], self.sources, terms, speechGain=sg, dtype=npt, gains=True)
        return self.done[(key, npt)]


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    lens = [len(p) for p in f.pcm]
    assert lens[:6] == LENGTHS and lens[SILENT] == 800 and 2000 < lens[SPEECH] < 9000 and lens == [Stemmed(f.batch).length(u) for u in range(8)]
    assert not f.pcm[SILENT].any() and not f.pcm[0].any() and all(f.pcm[u].any() for u in (1, 2, 3, 4, 5, SPEECH))      # (three samples into a fade from silence are 0 too)
    yield f
    f.bp.close()


def case_rows(f, names=None, many=True):
    """Rows (u, device terms, host terms, speechGain, key) for every utterance and case; the other utterance of row u is u + 3 (mod 8)."""
    rows = []
    for u in range(8):
        L, other = len(f.pcm[u]), (u + 3) % 8
        dev = case_terms(L, u, other, len(f.pcm[other]))
        hst = case_terms(L, f.host(u), f.host(other), len(f.pcm[other]))
        for name in dev:
            if names is None or name in names:
                rows.append((u, dev[name][0], hst[name][0], dev[name][1], (name, u)))
        if many:
            rows.append((u, many_terms(L, u, other, len(f.pcm[other])), many_terms(L, f.host(u), f.host(other), len(f.pcm[other])), 0.9, ("many", u)))
    return rows


def check_rows(f, rows, tag, forms=None):
    """float32 and int16, padded and packed: every row's bits are the statement's, the gains the host's, the padding +0."""
    import torch
    sel = [r[0] for r in rows]
    terms, sg = [r[1] for r in rows], [r[3] for r in rows]
    lens = [len(f.pcm[u]) for u in sel]
    for dtype, npt in ((torch.float32, np.float32), (torch.int16, np.int16)):
        want = [f.statement(r[4], r[0], r[2], r[3], npt) for r in rows]
        for padded in (True, False):
            if forms is not None and (dtype, padded) not in forms:
                continue
            out, second, gains, start = f.bp.mixedTensor(terms, speechGain=sg, utterances=sel, dtype=dtype, padded=padded, gains=True)
            assert list(second.numpy()) == (lens if padded else list(np.concatenate([[0], np.cumsum(lens)]))), tag
            assert out.dtype == dtype and out.shape == ((len(sel), max(lens)) if padded else (sum(lens),)), tag
            assert list(start.numpy()) == list(np.concatenate([[0], np.cumsum([len(t) for t in terms])])), tag
            got_rows, past = rows_of(out, second, padded)
            gains, start = gains.cpu().numpy(), start.numpy()
            for i, (g, (w, wg)) in enumerate(zip(got_rows, want)):
                assert np.array_equal(bits(gains[start[i]:start[i + 1]]), bits(wg)), (tag, "gains", dtype, padded, i, rows[i][4], gains[start[i]:start[i + 1]], wg)
                assert same(g, w), (tag, dtype, padded, i, rows[i][4])
            for i, z in enumerate(past):
                assert not z.view(np.uint32 if npt == np.float32 else np.uint16).any(), (tag, "padding", i)
            plain, _ = f.bp.mixedTensor(terms, speechGain=sg, utterances=sel, dtype=dtype, padded=padded)      # without the gains: the same values
            assert torch.equal(plain, out), tag


def test_the_device_gives_the_statements_bits(fx):
    """Every utterance of the fixture against the whole case list of tests/test_mix_host.py and a row of 64 terms, in one call of some 300
    rows (every utterance repeated, a different mixture on each repeat), every form; then reversed."""
    rows = case_rows(fx)
    assert len(rows) > 250 and max(len(r[1]) for r in rows) == 64
    check_rows(fx, rows, "given")
    import torch
    check_rows(fx, rows[::-1], "reversed", forms=[(torch.float32, False), (torch.int16, True)])
    # the speech gain's default and a scalar; utterances None
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    terms = [[M(noise=5, snr=10.0, offset=u)] for u in range(8)]
    a, la = fx.bp.mixedTensor(terms, padded=False)
    b, lb = fx.bp.mixedTensor(terms, speechGain=1.0, utterances=np.arange(8), padded=False)
    assert torch.equal(a, b) and torch.equal(la, lb)
    for u, g in enumerate(rows_of(a, la, False)[0]):
        assert same(g, eng.pcmMix(fx.pcm[u], fx.sources, terms[u])), u
    # the large-batch form: a structured array and termStart
    flat = np.array([t[0].record() for t in terms], eng.mixTermDtype)
    c, lc = fx.bp.mixedTensor((flat, np.arange(9)), padded=False)
    assert torch.equal(a, c)
    # speech gain 0 and no speech terms: the noise bed alone, and the identity
    bed, _ = fx.bp.mixedTensor([[M(noise=4, gain=1.0)]], speechGain=0.0, utterances=[5])
    assert torch.equal(bed[0].cpu(), torch.from_numpy(np.resize(fx.clips[4], 5000) + np.float32(0)))
    for dtype in (torch.float32, torch.int16):
        ident, _ = fx.bp.mixedTensor([[]] * 8, dtype=dtype)
        assert torch.equal(ident, fx.bp.pcmTensor(dtype=dtype)[0]), dtype


def test_without_a_bank():
    """A player with no bank mixes utterances; a term that names a clip is refused; so it is after the bank has been freed."""
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    f = Fixture(clips=False)
    assert len(f.bp.noiseBankPowers()) == 0
    rows = case_rows(f, names=("own_utterance", "other_utterance_looped", "once_utterance_negative", "once_utterance_tile", "no_terms"), many=False)
    check_rows(f, rows, "no bank")
    with pytest.raises(RuntimeError, match="row 2, term 1: clip 0, and no noise bank is set"):
        f.bp.mixedTensor([[], [], [M(utterance=1, gain=1.0), M(noise=0, snr=3.0)]], utterances=[0, 1, 2])
    f.bp.setNoiseBank(f.clips)
    check_rows(f, rows, "a bank, and no clip named")
    f.bp.setNoiseBank(None)
    assert len(f.bp.noiseBankPowers()) == 0
    with pytest.raises(RuntimeError, match="no noise bank is set"):
        f.bp.mixedTensor([[M(noise=0, snr=3.0)]], utterances=[0])
    check_rows(f, rows, "the bank freed")
    f.bp.close()


def test_empty_utterances():
    """Utterances of no samples (no frames) beside voiced ones: their power is 0 and every SNR against or within them gives gain +0; a row
    of no samples writes nothing (packed) or padding alone (padded); a term placed once on an empty source is accepted and contributes
    nothing; a LOOPED term on one is refused, writes nothing and sets the error code."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    M = eng.MixTerm
    batch = single_frames([1500, 2049])
    batch["frame_start"] = np.array([0, 0, 1, 1, 2], np.int64)      # utterances 0 and 2 are empty
    batch["seeds"] = np.arange(1, 5, dtype=np.uint32)
    f = Fixture(batch=batch)
    bp = f.bp
    assert [len(p) for p in f.pcm] == [0, 1500, 0, 2049] and f.pcm[1].any() and f.pcm[3].any()
    sums, lens = bp.powerTensor()
    assert sums.cpu().tolist() == exact_sums(f.pcm) and sums.cpu().tolist()[0] == 0 and sums.cpu().tolist()[2] == 0 and lens.cpu().tolist() == [0, 1500, 0, 2049]
    assert bp.powerTensor(utterances=[2, 0, 2])[0].cpu().tolist() == [0, 0, 0]      # jobs of no tiles alone: no power launch
    assert bp.powerTensor(utterances=[2, 3, 0, 1, 2])[0].cpu().tolist() == [exact_sums(f.pcm)[u] for u in (2, 3, 0, 1, 2)]

    def both(u, make):
        return (u, make(lambda v: v), make(f.host))

    rows = [both(0, lambda h: [M(noise=5, snr=10.0), M(utterance=h(1), snr=0.0)]) + (1.0, "empty row, SNR terms"),
            both(1, lambda h: [M(utterance=h(0), snr=0.0, loop=False), M(utterance=h(2), gain=0.5, loop=False, offset=5), M(noise=5, snr=10.0)]) + (1.0, "empty sources once"),
            both(2, lambda h: []) + (0.5, "empty row, no terms"),
            both(3, lambda h: [M(utterance=h(3), snr=6.0, offset=7), M(utterance=h(0), snr=3.0, loop=False, offset=-3), M(utterance=h(1), snr=0.0, offset=1499)]) + (1.0, "own, empty, other"),
            both(2, lambda h: [M(utterance=h(2), gain=1.0, loop=False), M(utterance=h(3), snr=-5.0, loop=False, offset=100)]) + (1.0, "empty row, its own utterance once"),
            both(1, lambda h: [M(noise=2, snr=20.0, offset=1022)]) + (0.75, "between empty rows")]
    check_rows(f, rows, "empty utterances")
    check_rows(f, rows[::-1], "empty utterances, reversed")
    _, g = eng.pcmMix(f.pcm[1], f.sources, rows[1][2], gains=True)
    assert bits(g[:1])[0] == 0 and g[1] == 0.5 and g[2] > 0      # an SNR against an empty source is gain +0
    _, g = eng.pcmMix(f.pcm[0], f.sources, rows[0][2], gains=True)
    assert not bits(g).any()                                     # ... and so is every SNR within an empty row
    # rows of no samples alone: nothing to write, no buffer needed
    out, lens, g, start = bp.mixedTensor([[M(noise=0, snr=1.0)], []], utterances=[0, 2], gains=True)
    assert out.shape == (2, 0) and lens.tolist() == [0, 0] and start.tolist() == [0, 1, 1]
    # the looped term on an empty source
    out = torch.full((4 * 2049 + 8,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    gains = torch.full((8,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    utt = np.arange(4, dtype=np.int64)
    start = np.array([0, 0, 2, 2, 3], np.int64)
    for name, empty in (("first", 0), ("second", 2)):
        terms = np.array([M(noise=1, snr=3.0).record(), M(utterance=empty, snr=0.0, offset=0).record(), M(utterance=1, gain=1.0).record()], eng.mixTermDtype)
        for stride in (2049, 0):
            assert export(L, bp, out.data_ptr(), utt, terms, start, gains=gains.data_ptr(), stride=stride) == -1, name
            assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
            assert L.speechPlayer_lastError().decode() == "exportMixed: row 1, term 1: a looped source of length 0", name
    with pytest.raises(RuntimeError, match="row 0, term 0: a looped source of length 0"):
        bp.mixedTensor([[M(utterance=0, gain=1.0)]], utterances=[0])      # (refused although the row itself has no samples)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((gains == -7.0).all())
    terms = np.array([M(noise=1, snr=3.0).record(), M(utterance=0, snr=0.0, offset=0, loop=False).record(), M(utterance=1, gain=1.0).record()], eng.mixTermDtype)
    assert export(L, bp, out.data_ptr(), utt, terms, start, gains=gains.data_ptr(), stride=0) == 1500 + 2049 and L.speechPlayer_lastErrorCode() == 0
    torch.cuda.synchronize()
    w, wg = eng.pcmMix(f.pcm[1], f.sources, [M(noise=1, snr=3.0), M(utterance=f.host(0), snr=0.0, loop=False)], gains=True)
    assert same(out[:1500].cpu().numpy(), w) and np.array_equal(bits(gains[:2].cpu().numpy()), bits(wg)) and float(gains[2]) == 1.0 and bool((gains[3:] == -7.0).all())
    assert same(out[1500:1500 + 2049].cpu().numpy(), eng.pcmMix(f.pcm[3], f.sources, [M(utterance=f.host(1), gain=1.0)])) and bool((out[1500 + 2049:] == -7.0).all())
    bp.close()


def exact_sums(pcm):
    return [int(np.sum(p.astype(np.int64) ** 2)) for p in pcm]


def test_powers(fx):
    """powerTensor equals the exact integer sums: every utterance, a selection with repeats in reverse, after a second synthesize(), in
    MODE_FAST against that mode's own PCM; the bank's powers equal the ascending binary64 sums."""
    from tests.test_mix_host import clip_power
    want = exact_sums(fx.pcm)
    sums, lens = fx.bp.powerTensor()
    assert sums.dtype.is_floating_point is False and sums.is_cuda and lens.is_cuda
    assert sums.cpu().tolist() == want and lens.cpu().tolist() == [len(p) for p in fx.pcm] and want[SILENT] == 0 and min(want[1:6]) > 0
    sel = [7, 5, 5, 0, 6, 7, 1]
    sums, lens = fx.bp.powerTensor(utterances=sel)
    assert sums.cpu().tolist() == [want[u] for u in sel] and lens.cpu().tolist() == [len(fx.pcm[u]) for u in sel]
    fx.bp.synthesize()
    assert fx.bp.powerTensor()[0].cpu().tolist() == want
    assert len(fx.bp.powerTensor(utterances=[])[0]) == 0
    powers = fx.bp.noiseBankPowers()
    assert powers.dtype == np.float64 and powers.tolist() == [clip_power(c) for c in fx.clips] and powers[-1] == 0.0
    fast = Fixture(mode=1)
    assert fast.bp.powerTensor()[0].cpu().tolist() == exact_sums(fast.pcm)
    check_rows(fast, case_rows(fast, names=("loop_N1025_from_0", "own_utterance", "two_talkers_and_noise", "once_negative"), many=False), "fast")
    fast.bp.close()
    # utterances of P - 1, P, P + 1 and 2 P + 3616 samples (P = kPowerTile = 8192): one, two and three tiles, whole and ragged 16-byte loads
    lens = [8191, 8192, 8193, 20000]
    bp, pcm = player(single_frames(lens))
    assert [len(p) for p in pcm] == lens and all(p.any() for p in pcm)
    assert bp.powerTensor()[0].cpu().tolist() == exact_sums(pcm) and bp.powerTensor(utterances=[3, 3, 0])[0].cpu().tolist() == [exact_sums(pcm)[u] for u in (3, 3, 0)]
    bp.close()


def test_independent_of_the_shared_code(fx):
    """numpy float64: y64 = sg s / 32767 + sum g_j v_j with the gains the export returned; |y - y64| <= gamma_(T + 2) (|sg x| + sum |g_j v_j|),
    T the row's terms: the two extra roundings are the input conversion and the first product."""
    rows = case_rows(fx, names=("loop_N3_from_last", "loop_N1025_from_0", "once_negative", "once_utterance_positive", "own_utterance", "two_talkers_and_noise", "clamp"))
    sel, terms, sg = [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows]
    out, offsets, gains, start = fx.bp.mixedTensor(terms, speechGain=sg, utterances=sel, padded=False, gains=True)
    gains, start = gains.cpu().numpy().astype(np.float64), start.numpy()
    worst = 0.0
    for i, g in enumerate(rows_of(out, offsets, False)[0]):
        u = sel[i]
        L, m = len(fx.pcm[u]), np.arange(len(fx.pcm[u]), dtype=np.int64)
        y = float(np.float32(sg[i])) * fx.pcm[u].astype(np.float64) / 32767.0
        mag = np.abs(y)
        for t, gj in zip(terms[i], gains[start[i]:start[i + 1]]):
            src = fx.clips[t.source].astype(np.float64) if t.kind == 0 else fx.pcm[t.source].astype(np.float64) / 32767.0
            v = np.zeros(L)
            if t.loop:
                v = src[(t.offset + m) % len(src)]
            else:
                k = m - t.offset
                ok = (k >= 0) & (k < len(src))
                v[ok] = src[k[ok]]
            y, mag = y + gj * v, mag + np.abs(gj * v)
        n = len(terms[i]) + 2
        bound = n * U / (1 - n * U) * mag
        err = np.abs(g.astype(np.float64) - y)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))) if L else 0.0)
        assert np.all(err <= bound), (rows[i][4], float(np.max(err - bound)))
    print("largest error over its bound: %.3g" % worst)


def export(L, bp, ptr, utterances, terms, start, sg=None, gains=None, fmt=1, stride=0, n=None, batch=0, stream=None):
    p = lambda a: None if a is None else a.ctypes.data
    return L.speechPlayer_batch_exportMixed(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, p(terms), p(start), p(sg), gains, ptr,
                                            fmt, stride, stream)


def flat_terms(rows):
    import nvspeechplayer_amd as eng
    flat = np.array([t.record() for r in rows for t in r[1]], eng.mixTermDtype).reshape(-1)
    return flat, np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])]).astype(np.int64)


def test_edges(fx):
    """Through the library's entry point into a buffer with guards either side, 16-byte aligned and one element past a 16-byte boundary,
    packed and two padded widths, both dtypes: the values are the statement's, the padding is +0, the guards are untouched."""
    import torch
    from nvspeechplayer_amd import _native
    L = _native.load()
    rows = case_rows(fx, names=("loop_N3_from_last", "loop_N1024_from_0", "once_tile", "once_utterance_negative", "no_terms_half"), many=False)
    rows = [r for r in rows if r[0] != SPEECH] + [r for r in rows if r[0] == 0]
    sel = np.array([r[0] for r in rows], np.int64)
    sg = np.array([r[3] for r in rows], np.float32)
    flat, start = flat_terms(rows)
    for fmt, dtype, npt in ((1, torch.float32, np.float32), (0, torch.int16, np.int16)):
        want = [fx.statement(r[4], r[0], r[2], r[3], npt)[0] for r in rows]
        most = max(len(w) for w in want)
        for stride in (0, most, most + 3):
            elements = sum(len(w) for w in want) if stride == 0 else len(sel) * stride
            for shift in (0, 1):
                buf = torch.full((elements + 2 * GUARD + 1,), -7, dtype=dtype, device="cuda:%d" % fx.bp.device)
                assert buf.data_ptr() % 16 == 0
                assert export(L, fx.bp, buf.data_ptr() + (GUARD + shift) * buf.element_size(), sel, flat, start, sg=sg, fmt=fmt, stride=stride) == elements
                torch.cuda.synchronize()
                got = buf.cpu().numpy()
                tag = (fmt, stride, shift)
                assert np.all(got[:GUARD + shift] == -7) and np.all(got[GUARD + shift + elements:] == -7), tag
                got = got[GUARD + shift:GUARD + shift + elements]
                at = 0
                for i, w in enumerate(want):
                    span = len(w) if stride == 0 else stride
                    assert same(got[at:at + len(w)], w), tag + (i, rows[i][4])
                    assert not got[at + len(w):at + span].view(np.uint32 if fmt else np.uint16).any(), tag + (i, "padding")
                    at += span


def test_ordering():
    """An export on a side stream right behind synthesize(wait=False), then -- no host wait -- other content is set and synthesised: the
    exported tensor still holds the first content.  setNoiseBank between two exports changes only the second.  A set call keeps the
    bank.  Seventeen exports in flight."""
    import torch
    import nvspeechplayer_amd as eng
    from tests.test_mix_host import clip_power
    M = eng.MixTerm
    f = Fixture()
    bp, clips = f.bp, f.clips
    other = compared("plain")
    side = torch.cuda.Stream(bp.device)
    terms = [[M(noise=5, snr=10.0, offset=3), M(utterance=(u + 1) % 8, snr=0.0, loop=False, offset=-2)] for u in range(8)]
    host_terms = [[M(noise=5, snr=10.0, offset=3), M(utterance=f.host((u + 1) % 8), snr=0.0, loop=False, offset=-2)] for u in range(8)]
    set_host(bp, f.batch)
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.mixedTensor(terms)
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.powerTensor()
    bp.synthesize(wait=False)
    with torch.cuda.stream(side):
        a, la, ga, _ = bp.mixedTensor(terms, padded=False, gains=True)
        pa, _ = bp.powerTensor()
    set_host(bp, other.b)      # other content: the set call and the next launch wait for the exports on the device
    bp.synthesize(wait=False)
    second_terms = [[M(noise=2, snr=5.0)] for _ in range(other.n)]
    with torch.cuda.stream(side):
        b, lb = bp.mixedTensor(second_terms, padded=False, dtype=torch.int16)
    torch.cuda.synchronize()
    second = [bp.read(u).copy() for u in range(other.n)]
    assert len(bp.noiseBankPowers()) == len(clips)      # the set calls kept the bank
    for u, g in enumerate(rows_of(b, lb, False)[0]):
        assert same(g, eng.pcmMix(second[u], clips, [M(noise=2, snr=5.0)], dtype=np.int16)), u
    got_gains = ga.cpu().numpy()
    for u, g in enumerate(rows_of(a, la, False)[0]):
        w, wg = eng.pcmMix(f.pcm[u], f.sources, host_terms[u], gains=True)
        assert same(g, w) and np.array_equal(bits(got_gains[2 * u:2 * u + 2]), bits(wg)), u
    assert pa.cpu().tolist() == exact_sums(f.pcm)
    # the bank is replaced between two exports, with no wait in between: the first keeps the old clips
    louder = [c * np.float32(2.0) for c in clips]
    with torch.cuda.stream(side):
        c1, l1 = bp.mixedTensor(second_terms, padded=False)
    bp.setNoiseBank(louder)
    with torch.cuda.stream(side):
        c2, l2 = bp.mixedTensor([[M(noise=2, gain=0.5)] for _ in range(other.n)], padded=False)
    torch.cuda.synchronize()
    for u, (g1, g2) in enumerate(zip(rows_of(c1, l1, False)[0], rows_of(c2, l2, False)[0])):
        assert same(g1, eng.pcmMix(second[u], clips, [M(noise=2, snr=5.0)])), u
        assert same(g2, eng.pcmMix(second[u], louder, [M(noise=2, gain=0.5)])), u
    assert np.array_equal(bp.noiseBankPowers(), 4.0 * np.array([clip_power(c) for c in clips]))
    # seventeen exports in flight (every slot, and one more)
    outs = [bp.mixedTensor([[M(noise=i % 6, snr=float(i))] for _ in range(other.n)], padded=False) for i in range(17)]
    torch.cuda.synchronize()
    for i, (out, offsets) in enumerate(outs):
        for u, g in enumerate(rows_of(out, offsets, False)[0]):
            assert same(g, eng.pcmMix(second[u], louder, [M(noise=i % 6, snr=float(i))])), (i, u)
    set_host(bp, other.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.mixedTensor(second_terms)
    bp.close()


def test_refusals_write_nothing_and_leave_the_batch_usable(fx):
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    bp = fx.bp
    utt = np.arange(8, dtype=np.int64)
    lens = [len(p) for p in fx.pcm]
    most, total = max(lens), sum(lens)
    out = torch.full((8 * most + 8,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    gains = torch.full((32,), -7.0, dtype=torch.float32, device="cuda:%d" % bp.device)
    sentinel, gsentinel = out.clone(), gains.clone()
    host = np.zeros(8 * most, np.float32)

    def term(kind=0, levelKind=0, source=0, offset=0, level=10.0, loop=1):
        return (kind, levelKind, source, offset, level, loop, 0)

    good = np.array([term(source=u % 6) for u in range(8)] + [term(kind=1, source=3, loop=0, offset=-4)], eng.mixTermDtype)
    start = np.array([0, 1, 2, 3, 4, 5, 6, 7, 9], np.int64)

    def with_term(**kw):      # row 6, term 0
        t = good.copy()
        t[6] = term(**kw)
        return t

    def call(**kw):
        a = dict(ptr=out.data_ptr(), utterances=utt, terms=good, start=start, gains=gains.data_ptr(), fmt=1, stride=most)
        a.update(kw)
        return export(L, bp, a.pop("ptr"), a.pop("utterances"), a.pop("terms"), a.pop("start"), **a)

    def refused(name, message=None, **kw):
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        text = L.speechPlayer_lastError().decode()
        assert text.startswith("exportMixed: ") and (message is None or message in text), (name, text)
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel) and torch.equal(gains, gsentinel), name

    seg = next(g for g in torch.cuda.memory_snapshot() if g["address"] <= out.data_ptr() < g["address"] + g["total_size"])
    one_short = seg["address"] + seg["total_size"] - 4 * (total - 1)
    assert one_short >= seg["address"]
    sg = np.ones(8, np.float32)

    def speech(v):
        g = sg.copy()
        g[4] = v
        return g

    many_start = (np.arange(65538, dtype=np.int64) * 64)
    cases = dict(
        no_batch=(dict(batch=None), "no batch"), format_2=(dict(fmt=2), "format 2"), format_negative=(dict(fmt=-1), None), stride_negative=(dict(stride=-1), "rowStride -1"),
        stride_short=(dict(stride=most - 1), "rowStride"), utterance_beyond=(dict(utterances=np.array([0, 8], np.int64), start=start[:3]), "utterances[1] = 8"),
        utterance_negative=(dict(utterances=np.array([-1], np.int64), start=start[:2]), None), negative_count=(dict(n=-1), None),
        host_memory=(dict(ptr=host.ctypes.data), None), no_buffer=(dict(ptr=None), "no output buffer"), misaligned_float=(dict(ptr=out.data_ptr() + 2), None),
        misaligned_int16=(dict(ptr=out.data_ptr() + 1, fmt=0), None), too_small=(dict(stride=1 << 34), None), too_small_packed=(dict(stride=0, ptr=one_short), None),
        gains_host_memory=(dict(gains=host.ctypes.data), None), gains_misaligned=(dict(gains=gains.data_ptr() + 2), None),
        no_term_start=(dict(start=None), "no termStart"), start_not_zero=(dict(start=start + 1), "termStart[0] = 1"),
        start_decreasing=(dict(start=np.array([0, 1, 2, 3, 2, 5, 6, 7, 9], np.int64)), "termStart[4] = 2 is below termStart[3] = 3"),
        terms_65=(dict(terms=np.repeat(good[:1], 65), start=np.array([0, 65], np.int64), utterances=utt[:1]), "row 0 has 65 terms"),
        terms_in_all=(dict(terms=np.zeros(1 << 22, eng.mixTermDtype), start=many_start, utterances=np.zeros(65537, np.int64), stride=0), "more than 4194304 terms in all"),
        no_terms=(dict(terms=None), "row 0 has 1 terms and there are none"),
        kind_2=(dict(terms=with_term(kind=2)), "row 6, term 0: kind 2"), kind_negative=(dict(terms=with_term(kind=-1)), "row 6, term 0: kind -1"),
        level_kind_2=(dict(terms=with_term(levelKind=2)), "row 6, term 0: levelKind 2"), loop_2=(dict(terms=with_term(loop=2)), "row 6, term 0: loop 2"),
        clip_beyond=(dict(terms=with_term(source=len(fx.clips))), "row 6, term 0: clip %d is not in the bank (%d clips)" % (len(fx.clips), len(fx.clips))),
        clip_negative=(dict(terms=with_term(source=-1)), "row 6, term 0: clip -1"),
        source_beyond=(dict(terms=with_term(kind=1, source=8)), "row 6, term 0: source 8 is not an utterance of the batch (8)"),
        source_negative=(dict(terms=with_term(kind=1, source=-1)), "row 6, term 0: source -1"),
        loop_offset_N=(dict(terms=with_term(source=1, offset=3)), "row 6, term 0: offset 3 of a looped source of 3 samples"),
        loop_offset_utterance=(dict(terms=with_term(kind=1, source=0, offset=3)), "row 6, term 0: offset 3 of a looped source of 3 samples"),
        loop_offset_negative=(dict(terms=with_term(offset=-1)), "row 6, term 0: offset -1"),
        offset_above=(dict(terms=with_term(loop=0, offset=2 ** 44 + 1)), "row 6, term 0: offset"), offset_below=(dict(terms=with_term(loop=0, offset=-2 ** 44 - 1)), "row 6, term 0: offset"),
        snr_nan=(dict(terms=with_term(level=np.nan)), "row 6, term 0: an SNR of nan dB"), snr_above=(dict(terms=with_term(level=200.5)), "row 6, term 0: an SNR of 200.5 dB"),
        snr_minus_inf=(dict(terms=with_term(level=-np.inf)), "row 6, term 0: an SNR of -inf dB"),
        gain_nan=(dict(terms=with_term(levelKind=1, level=np.nan)), "row 6, term 0: gain nan"), gain_above=(dict(terms=with_term(levelKind=1, level=2.0 ** 33)), "row 6, term 0: gain"),
        speech_gain_nan=(dict(sg=speech(np.nan)), "row 4: speechGain nan"), speech_gain_inf=(dict(sg=speech(np.inf)), "row 4: speechGain inf"),
        speech_gain_above=(dict(sg=speech(2.0 ** 33)), "row 4: speechGain"))
    for name, (kw, message) in cases.items():
        refused(name, message, **kw)
    second = good.copy()
    second[8] = term(kind=1, source=9, loop=0)
    assert call(terms=second) == -1 and b"row 7, term 1: source 9" in L.speechPlayer_lastError()
    # the power export's refusals
    sums = torch.full((16,), -7, dtype=torch.int64, device="cuda:%d" % bp.device)
    for name, args in dict(no_batch=(None, utt.ctypes.data, 8, sums.data_ptr()), beyond=(bp._h, np.array([8], np.int64).ctypes.data, 1, sums.data_ptr()),
                           negative=(bp._h, utt.ctypes.data, -1, sums.data_ptr()), host_memory=(bp._h, utt.ctypes.data, 8, host.ctypes.data),
                           no_buffer=(bp._h, utt.ctypes.data, 8, None), misaligned=(bp._h, utt.ctypes.data, 8, sums.data_ptr() + 4)).items():
        assert L.speechPlayer_batch_exportPower(*args, None) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert L.speechPlayer_lastError().decode().startswith("exportPower: "), name
    torch.cuda.synchronize()
    assert torch.all(sums == -7)
    # the bank's refusals leave the bank as it was
    noise, nstart = np.concatenate(fx.clips), np.concatenate([[0], np.cumsum([len(c) for c in fx.clips])]).astype(np.int64)
    p = lambda a: None if a is None else a.ctypes.data

    def spoiled(v):
        c = noise.copy()
        c[nstart[2] + 11] = v
        return c

    powers = bp.noiseBankPowers()
    for name, (args, message) in dict(negative=((noise, nstart, -1), "-1 clips"), too_many=((noise, nstart, (1 << 20) + 1), "clips"), no_noise=((None, nstart, 7), "no clips"),
                                      no_start=((noise, None, 7), "no clips"), start_not_zero=((noise, nstart + 1, 7), "noiseStart[0] = 1"),
                                      empty_clip=((noise, np.array([0, 5, 5], np.int64), 2), "a clip has at least 1 sample"),
                                      too_long=((noise, np.array([0, (1 << 28) + 1], np.int64), 1), "in all"),
                                      nan=((spoiled(np.nan), nstart, 7), "sample 11 of clip 2 is nan"), inf=((spoiled(-np.inf), nstart, 7), "sample 11 of clip 2 is -inf"),
                                      above=((spoiled(np.float32(65536.0 * (1 + 2.0 ** -23))), nstart, 7), "sample 11 of clip 2")).items():
        assert L.speechPlayer_batch_setNoiseBank(bp._h, p(args[0]), p(args[1]), args[2]) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        text = L.speechPlayer_lastError().decode()
        assert text.startswith("setNoiseBank: ") and message in text, (name, text)
    assert np.array_equal(bp.noiseBankPowers(), powers)
    # nothing to write needs no buffer
    assert export(L, bp, None, utt[:0], good, start[:1]) == 0 and L.speechPlayer_lastErrorCode() == 0
    # the limits themselves are admitted, and the batch is as usable as before
    assert call(terms=with_term(loop=0, offset=2 ** 44), sg=speech(-2.0 ** 32)) == 8 * most
    assert call(terms=with_term(levelKind=1, level=2.0 ** 32, loop=0, offset=-2 ** 44)) == 8 * most
    assert call(terms=with_term(level=-200.0)) == 8 * most and call(terms=with_term(level=200.0)) == 8 * most
    assert call() == 8 * most
    torch.cuda.synchronize()
    got = out[:8 * most].view(8, most).cpu().numpy()
    got_gains = gains.cpu().numpy()
    M = eng.MixTerm
    for u in range(8):
        terms = [M(noise=u % 6, snr=10.0)] if u < 7 else [M(noise=1, snr=10.0), M(utterance=fx.host(3), snr=10.0, loop=False, offset=-4)]
        w, wg = eng.pcmMix(fx.pcm[u], fx.sources, terms, gains=True)
        assert same(got[u, :len(w)], w) and not bits(got[u, len(w):]).any(), u
        assert np.array_equal(bits(got_gains[start[u]:start[u + 1]]), bits(wg)), u
    assert torch.equal(out[8 * most:], sentinel[8 * most:]) and torch.equal(gains[9:], gsentinel[9:])
    bp.synthesize()
    assert all(np.array_equal(bp.read(u), fx.pcm[u]) for u in range(8))
