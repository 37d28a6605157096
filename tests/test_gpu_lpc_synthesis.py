"""LPC synthesis of a batch's PCM and of a signal's rows (include/speechPlayer_batch.h: speechPlayer_batch_exportLpcSynthesis,
exportLpcSynthesisOf; BatchPlayer.lpcSynthesisTensor; csrc/klatt_lpcsynth.h) against the host's statements of the definition --
speechPlayer_pcmLpcSynthesis / signalLpcSynthesis applied to what the engine read -- bit for bit.  The statements themselves are held to a
transcription by tests/test_lpc_synthesis_host.py.  Needs a GPU."""
import numpy as np
import pytest

from tests.far_offsets import B31, plan_cycles
from tests.test_gpu_lpc import NULL, SHORT, SILENT, same, the_batch
from tests.test_gpu_signal import lay_out, poison, record
from tests.test_gpu_spectrogram import player, rows_of
from tests.test_gpu_timeline import set_host
from tests.test_lpc_host import float_row, golden_pcm
from tests.test_stems_host import compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64
SIX = list(range(13)) * 6      # 78 rows: one full group of the kernel, and one of 14 rows and 50 fillers, sorted by length across utterances


@pytest.fixture(scope="module")
def batch():
    bp, pcm = player(the_batch())
    assert len(pcm) == 13 and len(pcm[NULL]) == 0 and len(pcm[SHORT]) == 3 and len(pcm[SILENT]) > 7000
    yield bp, pcm
    bp.close()


@pytest.fixture(scope="module")
def bare():
    """A player that was never set: the exports of a signal need no batch content."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    yield bp
    bp.close()


def statement_of(row):
    import nvspeechplayer_amd as eng
    return eng.pcmLpcSynthesis if row.dtype == np.int16 else eng.signalLpcSynthesis


def every_form():
    import torch
    return [(torch.float32, True), (torch.int16, False), (torch.float32, False), (torch.int16, True)]


def check_synthesis(bp, rows, coeff_rows, lpc, kw, column, forms, tag, sel=None, signal=None, finite=True):
    """lpcSynthesisTensor in each of `forms` (dtype, padded): the chosen rows' bits are the statement's on coeff_rows[i] (float64
    [steps, order], one per CHOSEN row), the lengths are the rows', the padding is +0.  The host's output is asserted finite first."""
    import torch
    idx = list(range(len(rows))) if sel is None else list(sel)
    lens = [len(rows[u]) for u in idx]
    results = []
    for dtype, padded in forms:
        npt = np.float32 if dtype == torch.float32 else np.int16
        want = [statement_of(rows[u])(rows[u], coeff_rows[i], hop=kw["hop"], phase=kw["phase"], dtype=npt) for i, u in enumerate(idx)]
        if finite and npt == np.float32:
            assert all(np.all(np.isfinite(w)) for w in want), tag + ("the host's output is finite",)
        out, second = bp.lpcSynthesisTensor(lpc, column=column, utterances=sel, dtype=dtype, padded=padded, signal=signal, **kw)
        assert out.dtype == dtype and list(second.numpy()) == (lens if padded else list(np.concatenate([[0], np.cumsum(lens)]))), tag
        assert tuple(out.shape) == ((len(idx), max(lens, default=0)) if padded else (sum(lens),)), tag
        got, past = rows_of(out, second, padded)
        for i, (g, w) in enumerate(zip(got, want)):
            assert same(g, w), tag + (dtype, padded, i, idx[i], len(w))
        for z in past:
            assert not z.view(np.uint8).any(), tag + ("padding",)
        results.append((out, second, want))
    return results


def analysed(bp, order, hop, phase, dtype, padded, nWin, times):
    """The coefficients lpcTensor gives the thirteen utterances, inside a tensor of three fields, `times` times over on the device (the
    analysis runs once): -> (the tensor, the column of a_1, each utterance's [steps, order] as float64)."""
    import torch
    import nvspeechplayer_amd as eng
    lag = eng.lagWindow(order, 22050.0, whiteNoise=2.0 ** -12)
    lpc, second = bp.lpcTensor(order=order, nWin=nWin, hop=hop, phase=phase, lagWindow=lag, fields=("autocorr", "lpc", "error"), dtype=dtype, padded=padded)
    rows = [np.ascontiguousarray(r[:, order + 1:2 * order + 1]).astype(np.float64) for r in rows_of(lpc, second, padded)[0]]
    many = lpc.repeat(times, 1, 1) if padded else torch.cat([lpc] * times)
    return many.contiguous(), order + 1, rows


# ---- 1. the main grid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 8, 9, 16, 17, 32])
def test_synthesis_is_the_statements_bits(batch, order):
    """Every ring at both edges of its orders.  78 rows (the thirteen utterances six times over).  hop 1 (a load per sample), 64 with
    phase 32 (frame changes on tile edges) and phase 0 (inside tiles), 160 with phase 7 and 0, 8192 (one step); the coefficients from
    lpcTensor, float64 and float32, padded and packed, at a column inside a tensor of three fields; the excitation lpcResidualTensor's
    output as signal= (float32 and int16) and the pool's own PCM; the four output forms ROTATED over the combinations, two a
    combination, not crossed."""
    import torch
    bp, pcm = batch
    forms = every_form()
    for k, (hop, phase) in enumerate(((1, 0), (64, 32), (64, 0), (160, 7), (8192, 0), (160, 0))):
        cdtype, cpadded = (torch.float64, torch.float32)[(k + order) % 2], bool((k // 2 + order) % 2)
        lpc, column, coeff = analysed(bp, order, hop, phase, cdtype, cpadded, 64 if hop == 1 else 400, 6)
        kw = dict(order=order, hop=hop, phase=phase)
        two = [forms[(k + j) % 4] for j in range(2)]
        tag = (order, hop, phase, cdtype, cpadded)
        if k % 3 != 2:      # the residual, a signal of 78 rows, back through 1 / A(z)
            rdtype, rnpt = ((torch.float32, np.float32), (torch.int16, np.int16))[k % 2]
            res = bp.lpcResidualTensor(lpc, column=column, utterances=SIX, dtype=rdtype, padded=bool(k % 4 < 2), **kw)
            e_rows = rows_of(res[0], res[1], bool(k % 4 < 2))[0]
            check_synthesis(bp, [np.ascontiguousarray(r) for r in e_rows], [coeff[u] for u in SIX], lpc, kw, column, two, tag + ("residual", rdtype), signal=res)
        else:               # the pool's own PCM as the excitation
            check_synthesis(bp, pcm, [coeff[u] for u in SIX], lpc, kw, column, two, tag + ("pool",), sel=SIX)


# ---- 2. the caller's own coefficients ---------------------------------------------------------------------------------------------------------------
def test_the_callers_own_coefficients(batch):
    """Zeros: the output is the float32 of the input exactly; random reflection coefficients in (-0.9, 0.9) through lpcFromReflection,
    order 1 and 32, float64 and float32, at a column of their own."""
    import torch
    import nvspeechplayer_amd as eng
    bp, pcm = batch
    dev = "cuda:%d" % bp.device
    sel = [2, 11, 10, 12, 2]
    lens = [len(pcm[u]) for u in sel]
    forms = every_form()
    for order, hop, phase in ((1, 40, 0), (32, 160, 7)):
        steps = [-(-(L - phase) // hop) if L > phase else 0 for L in lens]
        zeros = torch.zeros((len(sel), max(steps), order + 2), dtype=torch.float32, device=dev)
        out, second = bp.lpcSynthesisTensor(zeros, order=order, hop=hop, phase=phase, column=2, utterances=sel)
        for g, u in zip(rows_of(out, second, True)[0], sel):
            assert same(g, pcm[u].astype(np.float32) / np.float32(32767.0)), (order, u)
        rng = np.random.default_rng(order)
        for k, dtype in enumerate((torch.float64, torch.float32)):
            host = rng.uniform(-1, 1, (sum(steps), order + 3))
            host[:, 3:] = np.concatenate([stable_frames(1, n, order, rng)[0] for n in steps])
            host = host.astype(np.float32 if dtype == torch.float32 else np.float64)
            own = torch.from_numpy(host).to(dev)
            ends = np.cumsum(steps)
            coeff_rows = [host[e - s:e, 3:].astype(np.float64) for s, e in zip(steps, ends)]
            check_synthesis(bp, pcm, coeff_rows, own, dict(order=order, hop=hop, phase=phase), 3, forms[2 * k:2 * k + 2], ("own", order, dtype), sel=sel)


# ---- 3. cross-synthesis ------------------------------------------------------------------------------------------------------------------------------
def made_rows(lens, npt):
    src = golden_pcm("ipa_l15_s10_c0_p100_i05")
    rows = [src[700 + 13 * i:700 + 13 * i + L].copy() for i, L in enumerate(lens)]
    return rows if npt == np.int16 else [float_row(r) for r in rows]


def made_signal(rows, npt, stride, shift, dev):
    """The rows as a device signal with poison either side of every row: -> (the whole buffer, the (tensor, extent) pair)."""
    import torch
    lens = [len(r) for r in rows]
    host, first, extent = lay_out(rows, npt, stride, poison, shift)
    data = torch.from_numpy(host.view(np.int32 if npt == np.float32 else np.int16)).to(dev)
    body = data.view(torch.float32 if npt == np.float32 else torch.int16)[first:first + (len(rows) * stride if stride else sum(lens))]
    return data, ((body.view(len(rows), stride), torch.from_numpy(extent)) if stride else (body, torch.from_numpy(extent)))


def stable_frames(n, steps, order, rng):
    """[n, steps, order] float64: per row one draw of reflection coefficients in (-0.9, 0.9), each step's shrunk by its own factors in
    (0.8, 1) -- filters that vary slowly along a row, as a time-varying recursion needs to stay bounded -- through lpcFromReflection."""
    import nvspeechplayer_amd as eng
    out = np.zeros((n, steps, order))
    for i in range(n):
        k0 = rng.uniform(-0.9, 0.9, order)
        for j in range(steps):
            out[i, j] = eng.lpcFromReflection(k0 * rng.uniform(0.8, 1.0, order))
    return out


def test_cross_synthesis_rows_out_of_order_with_repeats(bare):
    """Row i's excitation through row j's envelope: the coefficient tensor is permuted, the rows are chosen out of order with repeats, and
    their lengths straddle 64, 65 and 128 samples."""
    import torch
    dev = "cuda:%d" % bare.device
    lens = [63, 64, 65, 127, 128, 129, 200, 3, 0, 1]
    sel = [5, 0, 9, 4, 4, 8, 2, 6, 1, 3, 7, 5]
    rng = np.random.default_rng(7)
    for npt, order, hop, phase in ((np.float32, 10, 16, 0), (np.int16, 20, 50, 7)):
        rows = made_rows(lens, npt)
        most = -(-(max(lens) - phase) // hop)
        frames = stable_frames(len(sel), most, order, rng)
        perm = rng.permutation(len(sel))
        for k, dtype in enumerate((torch.float64, torch.float32)):
            host = frames.astype(np.float32 if dtype == torch.float32 else np.float64)[perm]
            steps = [-(-(lens[u] - phase) // hop) if lens[u] > phase else 0 for u in sel]
            coeff_rows = [host[i, :steps[i]].astype(np.float64) for i in range(len(sel))]
            _, signal = made_signal(rows, npt, max(lens) + 3 if k else 0, 1, dev)
            check_synthesis(bare, rows, coeff_rows, torch.from_numpy(np.ascontiguousarray(host)).to(dev), dict(order=order, hop=hop, phase=phase), 0, every_form()[2 * k:2 * k + 2],
                            ("cross", npt.__name__, dtype), sel=sel, signal=signal)


# ---- 4. the raw entry point ----------------------------------------------------------------------------------------------------------------------------
def test_the_raw_entry_point_on_a_side_stream_into_a_misaligned_buffer(bare):
    """speechPlayer_batch_exportLpcSynthesisOf on a non-default stream, the output one element past a 16-byte boundary, between guards:
    int16 and float32, padded and packed; the guards and the signal are as they were."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    dev = "cuda:%d" % bare.device
    lens = [300, 64, 0, 129, 65, 1000, 7]
    rows = made_rows(lens, np.float32)
    data, signal = made_signal(rows, np.float32, 0, 3, dev)
    before = data.clone()
    sel = np.array([5, 2, 0, 6, 3, 1, 4, 5], np.int64)
    order, hop, phase = 12, 80, 7
    steps = [-(-(lens[u] - phase) // hop) if lens[u] > phase else 0 for u in sel]
    host = stable_frames(1, sum(steps), order, np.random.default_rng(4))[0]
    coeff = torch.from_numpy(host).to(dev)
    ends = np.cumsum(steps)
    side = torch.cuda.Stream(device=dev)
    rec = record(sp, signal[0].data_ptr(), 1, len(lens), 0, signal[1].numpy())
    for fmt, dtype, npt in ((0, torch.int16, np.int16), (1, torch.float32, np.float32)):
        want = [eng.signalLpcSynthesis(rows[u], host[e - s:e], hop=hop, phase=phase, dtype=npt) for u, s, e in zip(sel, steps, ends)]
        for stride in (0, max(lens) + 2):
            elements = sum(len(w) for w in want) if stride == 0 else len(sel) * stride
            buf = torch.full((elements + 2 * GUARD + 1,), -7, dtype=dtype, device=dev)
            torch.cuda.synchronize()
            out = buf.data_ptr() + (GUARD + 1) * buf.element_size()
            assert buf.data_ptr() % 16 == 0 and out % 16 != 0
            got = L.speechPlayer_batch_exportLpcSynthesisOf(bare._h, rec.ctypes.data, sel.ctypes.data, len(sel), order, hop, phase, coeff.data_ptr(), 0, order, 0, 0, out, fmt, stride,
                                                            side.cuda_stream)
            assert got == elements, (fmt, stride, L.speechPlayer_lastError())
            side.synchronize()
            a = buf.cpu().numpy()
            assert np.all(a[:GUARD + 1] == -7) and np.all(a[GUARD + 1 + elements:] == -7), (fmt, stride, "guards")
            a, at = a[GUARD + 1:GUARD + 1 + elements], 0
            for i, w in enumerate(want):
                span = len(w) if stride == 0 else stride
                assert same(a[at:at + len(w)], w), (fmt, stride, i)
                assert not a[at + len(w):at + span].view(np.uint8).any(), (fmt, stride, i, "padding")
                at += span
    torch.cuda.synchronize()
    assert torch.equal(data, before), "the signal and its guards are as they were"


# ---- 5. hand-made signals ------------------------------------------------------------------------------------------------------------------------------
def test_hand_made_signals_between_poison(bare):
    """int16 and float32 signals with poison (NaN for float32) either side of every row, padded and packed, on odd first elements: nothing
    outside a row is read -- the output is the statement's and finite --, and the signal is unchanged afterwards."""
    import torch
    dev = "cuda:%d" % bare.device
    lens = [64 * 3, 64 * 3 + 1, 0, 3, 1500, 199, 63]
    sel = [6, 1, 0, 4, 2, 3, 1, 5]
    rng = np.random.default_rng(11)
    for npt in (np.int16, np.float32):
        rows = made_rows(lens, npt)
        for k, (stride, shift) in enumerate(((max(lens) + 5, 1), (0, 3))):
            order, hop, phase = (9, 64, 32) if k else (16, 100, 0)
            data, signal = made_signal(rows, npt, stride, shift, dev)
            before = data.clone()
            steps = [-(-(lens[u] - phase) // hop) if lens[u] > phase else 0 for u in sel]
            host = stable_frames(len(sel), max(steps), order, rng)
            coeff_rows = [host[i, :steps[i]] for i in range(len(sel))]
            check_synthesis(bare, rows, coeff_rows, torch.from_numpy(host).to(dev), dict(order=order, hop=hop, phase=phase), 0, every_form()[2 * k:2 * k + 2],
                            ("made", npt.__name__, stride), sel=sel, signal=signal)
            torch.cuda.synchronize()
            assert torch.equal(data, before), "the signal and its guards are as they were"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------
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
    hop, order = 100, 8
    steps = [-(-n // hop) for n in lens]
    most, mostSteps, cols = max(lens), max(steps), order + 1
    dev = "cuda:%d" % bp.device
    res = torch.full((s.n * most + 8,), -7, dtype=torch.int16, device=dev)
    coeff = torch.full((s.n * mostSteps * cols,), 0.0625, dtype=torch.float64, device=dev)
    canary_res, canary_coeff = res.clone(), coeff.clone()
    host = np.zeros(s.n * most * 8, np.float64)
    p = lambda a: None if a is None else a.ctypes.data

    def synth(ptr=0, cptr=0, utterances=utt, n=None, order=order, hop=hop, phase=0, cfmt=0, ccols=cols, col0=0, cstride=mostSteps, fmt=0, stride=most, batch=0):
        return L.speechPlayer_batch_exportLpcSynthesis(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, order, hop, phase,
                                                       coeff.data_ptr() if cptr == 0 else cptr, cfmt, ccols, col0, cstride, res.data_ptr() if ptr == 0 else ptr, fmt, stride, None)

    def refused(name, fn, entry, words=b"", **kw):
        assert fn(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert entry in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert torch.equal(res, canary_res) and torch.equal(coeff, canary_coeff), name

    refused("not synthesised since it was set", synth, b"exportLpcSynthesis", b"not been synthesised")
    bp.synthesize()
    pcm = [bp.read(u).copy() for u in range(s.n)]
    cases = dict(no_batch=(dict(batch=None), b"no batch"), order_0=(dict(order=0), b"order 0"), order_33=(dict(order=33), b"order 33"), hop_0=(dict(hop=0), b"hop 0"),
                 phase_negative=(dict(phase=-1), b"phase -1"), format_2=(dict(fmt=2), b"format 2"), stride_negative=(dict(stride=-1), b"rowStride -1"),
                 utterance_beyond=(dict(utterances=np.array([0, s.n], np.int64)), b"utterances[1]"), negative_count=(dict(n=-1), b""), no_output=(dict(ptr=None), b"no output"),
                 host_memory=(dict(ptr=host.ctypes.data), b""), too_small=(dict(stride=1 << 34), b""),
                 coeff_format=(dict(cfmt=2), b"coefficient format 2"), col0_negative=(dict(col0=-1), b"columns -1"),
                 col0_beyond=(dict(col0=2), b"columns 2 .. 9 of 9"), coeff_stride_short=(dict(cstride=mostSteps - 1), b"coeffStride %d is below the largest step count" % (mostSteps - 1)),
                 coeff_stride_negative=(dict(cstride=-1), b"coeffStride -1"), coeff_host=(dict(cptr=host.ctypes.data), b"coefficients"), no_coeff=(dict(cptr=None), b"no coefficients"),
                 coeff_misaligned=(dict(cptr=coeff.data_ptr() + 4), b"aligned"), coeff_too_small=(dict(cstride=1 << 34), b"coefficients"),
                 coeff_stride_wraps=(dict(cstride=1 << 62, utterances=utt[:4]), b"coeffStride 4611686018427387904"),
                 stride_short=(dict(stride=most - 1), b""), misaligned=(dict(ptr=res.data_ptr() + 1), b"aligned"),
                 overlap=(dict(ptr=coeff.data_ptr() + 64), b"overlaps the coefficients"))
    for name, (kw, words) in cases.items():
        refused(name, synth, b"exportLpcSynthesis", words, **kw)
    # a signal's table, and the output on the signal
    x = torch.zeros((4, 1000), dtype=torch.int16, device=dev)
    extent = np.full(4, 1000, np.int64)

    def of(rec=None, rows=None, **fields):
        if rec is None:
            rec = record(sp, x.data_ptr(), 0, 4, 1000, extent)
            for key, v in fields.items():
                rec[key] = v
            rec = rec.ctypes.data
        return L.speechPlayer_batch_exportLpcSynthesisOf(bp._h, rec, p(rows), 0 if rows is None else len(rows), order, hop, 0, coeff.data_ptr(), 0, cols, 0, 10, res.data_ptr(), 0, 1000, None)

    bad_extent = np.array([1000, 1001, 0, 0], np.int64)
    for name, kw, words in (("no signal", dict(rec=0), b"no signal"), ("signal format", dict(format=2), b"signal format 2"), ("signal rows", dict(nRows=-1), b"nRows"),
                            ("no extent", dict(extent=0), b"extent"), ("extent beyond the stride", dict(extent=bad_extent.ctypes.data), b"extent[1]"),
                            ("no data", dict(data=0), b"without data"), ("host data", dict(data=host.ctypes.data), b""), ("row beyond", dict(rows=np.array([4], np.int64)), b"rows[0] = 4"),
                            ("the output is the signal", dict(data=res.data_ptr()), b"overlaps the signal")):
        refused(name, of, b"exportLpcSynthesisOf", words, **kw)
    # nothing to write needs no buffer; and the batch is as usable as before
    assert synth(ptr=None, cptr=None, utterances=utt[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert of() == 4000
    torch.cuda.synchronize()
    assert not res[:4000].any()      # silence: +0 everywhere
    res.copy_(canary_res)
    assert synth() == s.n * most
    torch.cuda.synchronize()
    got = res[:s.n * most].view(s.n, most).cpu().numpy()
    sixteenth = np.full((mostSteps, order), 0.0625)
    for u in range(s.n):
        w = eng.pcmLpcSynthesis(pcm[u], sixteenth[:steps[u]], hop=hop, dtype=np.int16)
        assert same(got[u, :len(w)], w) and not got[u, len(w):].any(), u
    assert torch.equal(res[s.n * most:], canary_res[s.n * most:]) and torch.equal(coeff, canary_coeff)
    # seventeen exports in flight: every slot, and one more
    lpc = coeff.view(s.n, mostSteps, cols)
    outs = [bp.lpcSynthesisTensor(lpc, order=order, hop=hop, column=i % 2, padded=False) for i in range(17)]
    torch.cuda.synchronize()
    want = [eng.pcmLpcSynthesis(pcm[u], sixteenth[:steps[u]], hop=hop) for u in range(s.n)]
    for i, (o, offsets) in enumerate(outs):
        for u, g in enumerate(rows_of(o, offsets, False)[0]):
            assert same(g, want[u]), (i, u)
    set_host(bp, s.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.lpcSynthesisTensor(lpc, order=order, hop=hop)
    with pytest.raises(ValueError, match="cuda"):
        bp.lpcSynthesisTensor(torch.zeros((s.n, mostSteps, cols)), order=order, hop=hop)
    with pytest.raises(ValueError, match="columns"):
        bp.lpcSynthesisTensor(lpc, order=order, hop=hop, column=2)
    with pytest.raises(ValueError, match="steps"):
        bp.lpcSynthesisTensor(lpc[:, :5].contiguous(), order=order, hop=hop)
    with pytest.raises(TypeError, match="contiguous"):
        bp.lpcSynthesisTensor(lpc.to(torch.float16), order=order, hop=hop)
    bp.close()


# ---- 7. past element 2^31 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
def test_far_outputs(padded):
    """exportLpcSynthesis (order 8, hop 160, int16) past element 2^31 with the periodic selection of tests/far_offsets.py, the coefficients
    of the same selection read from a tensor of the analysis' own: every later cycle is the first on the device, the first, the
    straddling and the last are the host's."""
    import torch
    import nvspeechplayer_amd as eng
    from tests.test_gpu_far_offsets import ORDER, check_cycles, into_guarded, want_cycle
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    lens = np.array([len(p) for p in pcm], np.int64)
    kw = dict(order=8, hop=160, phase=0)
    plan = plan_cycles(lens, 1, (B31,), padded, ORDER)
    lag = eng.lagWindow(8, 22050.0, whiteNoise=2.0 ** -12)
    lpc, _ = bp.lpcTensor(nWin=256, fields="lpc", lagWindow=lag, utterances=plan.selection(), dtype=torch.float32, padded=padded, **kw)
    rows = [eng.pcmLpcSynthesis(p, eng.pcmLpc(p, nWin=256, fields="lpc", lagWindow=lag, **kw).astype(np.float32), dtype=np.int16, hop=160, phase=0) for p in pcm]
    kept = {}
    with into_guarded(bp, kept, plan.repeats * len(plan.cycle), plan.rowStride, plan.per, plan.total):
        bp.lpcSynthesisTensor(lpc, utterances=plan.selection(), dtype=torch.int16, padded=padded, **kw)
    check_cycles(kept["buf"], kept["body"], plan, want_cycle(plan, rows, 0, np.int16), kept["got"], ("synthesis", padded))
    bp.close()
    del kept, lpc
    torch.cuda.empty_cache()
