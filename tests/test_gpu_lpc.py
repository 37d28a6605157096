"""Linear prediction of a batch's PCM and of a signal's rows (include/speechPlayer_batch.h: speechPlayer_batch_exportLpc, exportLpcOf,
exportLpcResidual, exportLpcResidualOf; BatchPlayer.lpcTensor, lpcResidualTensor; csrc/klatt_lpc.h) against the host's statements of the
definition -- speechPlayer_pcmLpc / signalLpc and pcmLpcResidual / signalLpcResidual applied to what the engine read -- bit for bit, on
integer views.  The statements themselves are held to a transcription and to scipy by tests/test_lpc_host.py.  Needs a GPU."""
import numpy as np
import pytest

from tests.far_offsets import B31, B32, plan_cycles
from tests.test_gpu_signal import lay_out, poison, record
from tests.test_gpu_spectrogram import player, rows_of
from tests.test_gpu_timeline import set_host
from tests.test_lpc_host import bits, float_row, golden_pcm
from tests.test_stems_host import compared

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64
ALL = 31
NULL, SHORT, SILENT = 10, 11, 12      # the utterances added to the ten of the plain batch


def same(got, want):
    """Equality of type, shape and every bit."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def the_batch():
    """The ten utterances of the plain batch (840 .. 5860 samples) and three more: one of no frames (length 0), one of 3 samples (shorter
    than half of any window here but the smallest), and one with a null frame of 6000 samples (the resonators ring out, then exact zeros) between two voiced frames."""
    b = dict(compared("plain").b)
    voiced = [k for k in range(len(b["frames"])) if not b["isnull"][k]][:3]
    n = len(b["min"])
    extra_min, extra_fade, extra_null = [0, 400, 6000, 600], [1, 100, 100, 100], [0, 0, 1, 0]
    b["frames"] = np.concatenate([b["frames"], b["frames"][[voiced[0], voiced[1], voiced[1], voiced[2]]]])
    b["min"] = np.concatenate([b["min"], np.array(extra_min, np.uint32)])
    b["fade"] = np.concatenate([b["fade"], np.array(extra_fade, np.uint32)])
    b["index"] = np.concatenate([b["index"], np.full(4, -1, np.int32)])
    b["isnull"] = np.concatenate([b["isnull"], np.array(extra_null, np.uint8)])
    b["frame_start"] = np.concatenate([b["frame_start"], [n, n + 1, n + 4]]).astype(np.int64)
    b["seeds"] = np.concatenate([b["seeds"], np.array([11, 12, 13], np.uint32)])
    return b


@pytest.fixture(scope="module")
def batch():
    bp, pcm = player(the_batch())
    assert len(pcm) == 13 and len(pcm[NULL]) == 0 and len(pcm[SHORT]) == 3 and len(pcm[SILENT]) > 7000
    quiet = np.flatnonzero(pcm[SILENT] == 0)
    assert len(quiet) > 3000 and pcm[SILENT][:300].any() and pcm[SILENT][-300:].any()      # a long silence inside
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
    return (eng.pcmLpc, eng.pcmLpcResidual) if row.dtype == np.int16 else (eng.signalLpc, eng.signalLpcResidual)


def check_analysis(bp, rows, kw, forms, tag, sel=None, signal=None):
    """lpcTensor in each of `forms` (dtype, padded) against the statement of every chosen row: shapes, step counts, bits, +0 padding."""
    import torch
    idx = list(range(len(rows))) if sel is None else list(sel)
    want = [statement_of(rows[u])[0](rows[u], **kw) for u in idx]
    steps = [len(w) for w in want]
    for dtype, padded in forms:
        npt = np.float32 if dtype == torch.float32 else np.float64
        out, second = bp.lpcTensor(dtype=dtype, padded=padded, utterances=sel, signal=signal, **kw)
        assert out.dtype == dtype and list(second.numpy()) == (steps if padded else list(np.concatenate([[0], np.cumsum(steps)]))), tag
        assert tuple(out.shape) == ((len(idx), max(steps, default=0), want[0].shape[1]) if padded else (sum(steps), want[0].shape[1])), tag
        got, past = rows_of(out, second, padded)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(bits(g), bits(w.astype(npt))), tag + (dtype, padded, i, idx[i])
        for i, z in enumerate(past):
            assert not bits(z).any(), tag + ("padding", i)
    return want


def every_form():
    import torch
    return [(torch.float64, True), (torch.float32, False), (torch.float64, False), (torch.float32, True)]


# ---- 1. the analysis against the host statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 16, 32])
@pytest.mark.parametrize("win", ["order+1", 64, 65, 400, 4096])
def test_analysis_is_the_statements_bits(batch, win, order):
    """The thirteen utterances: hop 160 and 8192 on all of them and hop 1 on the three shortest, phase 0 and 7, every field at once, float64
    and float32, padded and packed; a lag window with the default window, none with a window of the caller's.  The four output forms
    are ROTATED over the twelve combinations of hop, phase and window, two forms a combination, not crossed with them: every form meets
    every (order, nWin) and every hop, not every hop with every phase and window."""
    import nvspeechplayer_amd as eng
    bp, pcm = batch
    nWin = order + 1 if win == "order+1" else win
    lag = eng.lagWindow(order, 22050.0, whiteNoise=2.0 ** -12)
    window = np.hamming(nWin) - 0.15
    forms = every_form()
    k = 0
    for hop in (160, 8192, 1):
        sel = None if hop > 1 else [SHORT, 9, NULL, 8]      # (hop 1 on the shortest rows only: 3, 840, 0 and 876 steps)
        for phase in (0, 7):
            for lw, w in ((lag, None), (None, window)):
                kw = dict(order=order, nWin=nWin, hop=hop, phase=phase, window=w, lagWindow=lw, fields=ALL)
                want = check_analysis(bp, pcm, kw, forms[k % 4:k % 4 + 2] if k % 4 < 3 else [forms[3], forms[0]], (win, order, hop, phase, lw is not None), sel=sel)
                k += 1
    if nWin >= 400:      # the batch holds silent frames and frames that run the whole recursion
        stages = eng.pcmLpc(pcm[SILENT], order=order, nWin=nWin, hop=160, lagWindow=lag, fields="stages")
        assert (stages == 0).any() and (stages == order).any()


def test_every_field_alone_a_selection_with_repeats_and_step_counts_around_64(batch):
    """Each field alone and some pairs; a selection with repeats in reverse order; hops that give the longest utterance 64, 65 and 128
    steps (whole groups of the kernel, and one step more), twice over, with the 3-sample utterance behind."""
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    bp, pcm = batch
    forms = every_form()
    for k, fields in enumerate([(f,) for f in sp.LPC_FIELDS] + [("lpc", "error"), ("stages", "autocorr"), ("reflection", "lpc", "error")]):
        check_analysis(bp, pcm, dict(order=10, nWin=300, hop=160, phase=3, fields=fields), [forms[k % 4]], ("fields", fields))
    sel = [12, 11, 10, 9, 9, 5, 2, 2, 0]
    check_analysis(bp, pcm, dict(order=12, nWin=256, hop=100, phase=0, fields=("lpc", "error")), forms, ("selection",), sel=sel)
    L = len(pcm[2])
    for steps in (64, 65, 128):
        hop = next(h for h in range(1, L) if -(-L // h) == steps)
        want = check_analysis(bp, pcm, dict(order=8, nWin=128, hop=hop, phase=0, fields=ALL), forms[:2], ("steps", steps), sel=[2, 2, 11])
        assert len(want[0]) == steps
    bp2 = bp.lpcTensor(order=4, nWin=64, hop=160, utterances=[NULL, NULL], dtype=torch.float64)      # rows of nothing: nothing to launch
    assert tuple(bp2[0].shape) == (2, 0, 5) and list(bp2[1].numpy()) == [0, 0]


def test_the_raw_entry_point_on_a_side_stream_into_a_misaligned_buffer(batch):
    """speechPlayer_batch_exportLpc on a non-default stream, the output one element past a 16-byte boundary, between guards: float64 and
    float32, padded and packed."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    bp, pcm = batch
    dev = "cuda:%d" % bp.device
    sel = np.array([7, 12, 0, 11, 10, 3], np.int64)
    kw = dict(order=16, nWin=400, hop=160, phase=7)
    lag = eng.lagWindow(16, 22050.0)
    want = [eng.pcmLpc(pcm[u], lagWindow=lag, fields=ALL, **kw) for u in sel]
    steps, cols = [len(w) for w in want], want[0].shape[1]
    side = torch.cuda.Stream(device=dev)
    for fmt, dtype, npt in ((0, torch.float64, np.float64), (1, torch.float32, np.float32)):
        for stride in (0, max(steps) + 2):
            elements = (sum(steps) if stride == 0 else len(sel) * stride) * cols
            buf = torch.full((elements + 2 * GUARD + 1,), -7.0, dtype=dtype, device=dev)
            torch.cuda.synchronize()
            out = buf.data_ptr() + (GUARD + 1) * buf.element_size()
            assert buf.data_ptr() % 16 == 0 and out % 16 != 0
            got = L.speechPlayer_batch_exportLpc(bp._h, sel.ctypes.data, len(sel), 16, 400, 160, 7, None, lag.ctypes.data, ALL, out, fmt, stride, side.cuda_stream)
            assert got == elements, (fmt, stride, L.speechPlayer_lastError())
            side.synchronize()
            a = buf.cpu().numpy()
            assert np.all(a[:GUARD + 1] == -7.0) and np.all(a[GUARD + 1 + elements:] == -7.0), (fmt, stride, "guards")
            a, at = a[GUARD + 1:GUARD + 1 + elements], 0
            for i, w in enumerate(want):
                span = (len(w) if stride == 0 else stride) * cols
                assert np.array_equal(bits(a[at:at + w.size]), bits(w.astype(npt).reshape(-1))), (fmt, stride, i)
                assert not bits(a[at + w.size:at + span]).any(), (fmt, stride, i, "padding")
                at += span


# ---- 2. signal= ---------------------------------------------------------------------------------------------------------------------------------
def test_the_signal_forms(batch, bare):
    """The analysis of convolvedTensor's output, float32 and int16, and of hand-made int16 and float32 signals with poison either side of
    every row (padded: in the rows' remainders; packed: before the first and behind the last), rows chosen out of order with a repeat:
    the statement's bits, and the signal unchanged afterwards.  Row lengths give 64 and 65 steps among others."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer as sp
    bp, pcm = batch
    forms = every_form()
    ir = (0.6 * np.exp(-np.arange(40) / 9.0) * np.cos(np.arange(40))).astype(np.float32)
    for k, (dtype, npt) in enumerate(((torch.float32, np.float32), (torch.int16, np.int16))):
        wet = bp.convolvedTensor(ir, dtype=dtype, padded=bool(k))
        rows = [eng.pcmConvolve(p, ir, dtype=npt) for p in pcm]
        check_analysis(bp, rows, dict(order=16, nWin=400, hop=160, phase=0, fields=("lpc", "error")), forms[2 * k:2 * k + 2], ("wet", dtype), sel=[12, 0, 11, 10, 5, 0], signal=wet)
    dev = "cuda:%d" % bare.device
    hop = 40
    lens = [64 * hop, 64 * hop + 1, 0, 3, 1500, 199, 128 * hop]
    for npt in (np.int16, np.float32):
        src = golden_pcm("ipa_l15_s10_c0_p100_i05")
        rows = [src[700 + 13 * i:700 + 13 * i + L].copy() for i, L in enumerate(lens)]
        rows = rows if npt == np.int16 else [float_row(r) for r in rows]
        for stride, shift in ((max(lens) + 5, 1), (0, 3)):
            host, first, extent = lay_out(rows, npt, stride, poison, shift)
            data = torch.from_numpy(host.view(np.int32 if npt == np.float32 else np.int16)).to(dev)
            before = data.clone()
            body = data.view(torch.float32 if npt == np.float32 else torch.int16)[first:first + (len(rows) * stride if stride else sum(lens))]
            signal = (body.view(len(rows), stride), torch.from_numpy(extent)) if stride else (body, torch.from_numpy(extent))
            sel = [6, 1, 0, 4, 2, 3, 1, 5]
            want = check_analysis(bare, rows, dict(order=32, nWin=65, hop=hop, phase=0, fields=ALL), forms[:2] if stride else forms[2:], ("made", npt.__name__, stride), sel=sel, signal=signal)
            assert [len(w) for w in want[:3]] == [128, 65, 64]
            res = bare.lpcResidualTensor(torch.zeros((len(sel), 128, 4), dtype=torch.float64, device=dev), order=4, hop=hop, utterances=sel, signal=signal)[0]
            zero = [np.zeros((-(-len(rows[u]) // hop), 4)) for u in sel]
            for g, u, z in zip(rows_of(res, torch.tensor([lens[u] for u in sel]), True)[0], sel, zero):      # (zero coefficients: x itself, but for the sign of a zero)
                assert same(g, statement_of(rows[u])[1](rows[u], z, hop=hop)) and np.array_equal(g, rows[u] if npt == np.float32 else rows[u].astype(np.float32) / np.float32(32767.0)), u
            torch.cuda.synchronize()
            assert torch.equal(data, before), "the signal and its guards are as they were"


# ---- 3. residual and prediction -------------------------------------------------------------------------------------------------------------
def check_inverse(bp, rows, coeff_rows, lpc, kw, column, tag, sel=None, signal=None):
    """lpcResidualTensor, both outputs, int16 and float32, padded and packed where the coefficients' layout allows: rows' bits are the
    statement's on coeff_rows[i] (float64 [steps, order])."""
    import torch
    idx = list(range(len(rows))) if sel is None else list(sel)
    lens = [len(rows[u]) for u in idx]
    got_rows = {}
    for what in ("residual", "prediction"):
        for dtype, npt in ((torch.float32, np.float32), (torch.int16, np.int16)):
            want = [statement_of(rows[u])[1](rows[u], coeff_rows[i], hop=kw["hop"], phase=kw["phase"], what=what, dtype=npt) for i, u in enumerate(idx)]
            for padded in (True, False):
                out, second = bp.lpcResidualTensor(lpc, column=column, what=what, utterances=sel, dtype=dtype, padded=padded, signal=signal, **kw)
                assert out.dtype == dtype and list(second.numpy()) == (lens if padded else list(np.concatenate([[0], np.cumsum(lens)]))), tag
                got, past = rows_of(out, second, padded)
                for i, (g, w) in enumerate(zip(got, want)):
                    assert same(g, w), tag + (what, dtype, padded, i, idx[i])
                for z in past:
                    assert not z.view(np.uint8).any(), tag + ("padding",)
                got_rows[what, npt, padded] = (out, second, want)
    return got_rows


@pytest.mark.parametrize("hop", [1, 160, 8192])
def test_residual_and_prediction_are_the_statements_bits(batch, hop):
    """Coefficients straight from lpcTensor, float64 and float32, padded and packed, `column` pointing into a tensor of several fields;
    hop 1 (every sample its own row of coefficients, read per lane), 160 (rows staged) and 8192 (longer than every row: one step).  The
    utterances are longer than a tile of 1024, so tiles start inside rows, and every row's first tile starts within its first `order`
    samples.  Then codedTensor("ulaw", signal=(residual, lengths)) equals the host's chain."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer as sp
    bp, pcm = batch
    order = 16
    sel = [SHORT, 9, NULL, 8] if hop == 1 else [12, 2, 10, 11, 0, 2]
    at, cols = sp.lpcColumns(("autocorr", "lpc", "error"), order)
    assert at["lpc"] == (order + 1, order) and cols == 2 * order + 2
    kw = dict(order=order, hop=hop, phase=7 if hop == 160 else 0)
    for dtype in (torch.float64, torch.float32):
        for padded in (True, False):
            lpc, second = bp.lpcTensor(nWin=400, fields=("autocorr", "lpc", "error"), utterances=sel, dtype=dtype, padded=padded, lagWindow=eng.lagWindow(order, 22050.0), **kw)
            coeff_rows = [r[:, order + 1:2 * order + 1].astype(np.float64) for r in rows_of(lpc, second, padded)[0]]
            assert any(c.any() for c in coeff_rows)
            got = check_inverse(bp, pcm, coeff_rows, lpc, kw, order + 1, ("analysis", hop, dtype, padded), sel=sel)
    # the pair is a signal: mu-law of the float32 residual
    out, second, want = got["residual", np.float32, True]
    decoded, codes, lens = bp.codedTensor("ulaw", codes=True, signal=(out, second))
    for i, w in enumerate(want):
        wd, wc = eng.signalCode(w, "ulaw", codes=True)
        assert same(decoded.cpu().numpy()[i, :len(w)], wd) and same(codes.cpu().numpy()[i, :len(w)], wc), i
    e, p = got["residual", np.float32, False][0], got["prediction", np.float32, False][0]
    x = np.concatenate([pcm[u] for u in sel]).astype(np.float32) / np.float32(32767.0)
    assert np.abs(e.cpu().numpy().astype(np.float64) + p.cpu().numpy() - x).max() < 1e-5      # x = e + p but for the two roundings


def test_the_callers_own_coefficients(batch):
    """Zeros: the residual is the float32 of x exactly and the prediction -0; random values in (-1, 1), float64 and float32, order 1 and
    32, at a column of their own."""
    import torch
    bp, pcm = batch
    dev = "cuda:%d" % bp.device
    sel = [2, 11, 10, 12]
    lens = [len(pcm[u]) for u in sel]
    for order, hop, phase in ((1, 40, 0), (32, 160, 7)):
        steps = [-(-(L - phase) // hop) if L > phase else 0 for L in lens]
        zeros = torch.zeros((len(sel), max(steps), order + 2), dtype=torch.float32, device=dev)
        out, second = bp.lpcResidualTensor(zeros, order=order, hop=hop, phase=phase, column=2, utterances=sel)
        for g, u in zip(rows_of(out, second, True)[0], sel):
            assert same(g, pcm[u].astype(np.float32) / np.float32(32767.0)), (order, u)
        out, second = bp.lpcResidualTensor(zeros, order=order, hop=hop, phase=phase, column=1, what="prediction", utterances=sel, padded=False)
        assert np.all(bits(out.cpu().numpy()) == 0x80000000)
        rng = np.random.default_rng(order)
        for dtype in (torch.float64, torch.float32):
            host = rng.uniform(-1, 1, (sum(steps), order + 3)).astype(np.float32 if dtype == torch.float32 else np.float64)
            own = torch.from_numpy(host).to(dev)
            ends = np.cumsum(steps)
            coeff_rows = [host[e - s:e, 3:].astype(np.float64) for s, e in zip(steps, ends)]
            check_inverse(bp, pcm, coeff_rows, own, dict(order=order, hop=hop, phase=phase), 3, ("own", order, dtype), sel=sel)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------------
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
    hop, order, nWin = 100, 8, 200
    steps = [-(-n // hop) for n in lens]
    most, mostSteps, cols = max(lens), max(steps), order + 1
    dev = "cuda:%d" % bp.device
    out = torch.full((s.n * mostSteps * cols + 8,), -7.0, dtype=torch.float64, device=dev)
    res = torch.full((s.n * most + 8,), -7, dtype=torch.int16, device=dev)
    coeff = torch.full((s.n * mostSteps * cols,), 0.25, dtype=torch.float64, device=dev)
    canary_out, canary_res, canary_coeff = out.clone(), res.clone(), coeff.clone()
    host = np.zeros(s.n * most * 8, np.float64)
    window, lag = np.ones(nWin), np.ones(order + 1)
    p = lambda a: None if a is None else a.ctypes.data

    def analysis(ptr=0, utterances=utt, n=None, order=order, nWin=nWin, hop=hop, phase=0, window=window, lag=lag, what=10, fmt=0, stride=mostSteps, batch=0):
        return L.speechPlayer_batch_exportLpc(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, order, nWin, hop, phase, p(window), p(lag), what,
                                              out.data_ptr() if ptr == 0 else ptr, fmt, stride, None)

    def inverse(ptr=0, cptr=0, utterances=utt, n=None, order=order, hop=hop, phase=0, cfmt=0, ccols=cols, col0=0, cstride=mostSteps, what=0, fmt=0, stride=most, batch=0):
        return L.speechPlayer_batch_exportLpcResidual(bp._h if batch == 0 else batch, p(utterances), len(utterances) if n is None else n, order, hop, phase,
                                                      coeff.data_ptr() if cptr == 0 else cptr, cfmt, ccols, col0, cstride, what, res.data_ptr() if ptr == 0 else ptr, fmt, stride, None)

    def refused(name, fn, entry, words=b"", **kw):
        assert fn(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert entry in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert torch.equal(out, canary_out) and torch.equal(res, canary_res) and torch.equal(coeff, canary_coeff), name

    refused("not synthesised since it was set", analysis, b"exportLpc", b"not been synthesised")
    refused("not synthesised since it was set", inverse, b"exportLpcResidual", b"not been synthesised")
    bp.synthesize()
    pcm = [bp.read(u).copy() for u in range(s.n)]
    shared = dict(no_batch=(dict(batch=None), b"no batch"), order_0=(dict(order=0), b"order 0"), order_33=(dict(order=33), b"order 33"), hop_0=(dict(hop=0), b"hop 0"),
                  phase_negative=(dict(phase=-1), b"phase -1"), format_2=(dict(fmt=2), b"format 2"), stride_negative=(dict(stride=-1), b"rowStride -1"),
                  utterance_beyond=(dict(utterances=np.array([0, s.n], np.int64)), b"utterances[1]"), negative_count=(dict(n=-1), b""), no_output=(dict(ptr=None), b"no output"),
                  host_memory=(dict(ptr=host.ctypes.data), b""), too_small=(dict(stride=1 << 34), b""))
    cases = dict(shared, nwin_order=(dict(nWin=order), b"nWin 8"), nwin_4097=(dict(nWin=4097), b"nWin 4097"), what_0=(dict(what=0), b"what 0"), what_32=(dict(what=32), b"what 32"),
                 window_nan=(dict(window=np.where(np.arange(nWin) == 5, np.nan, 1.0)), b"window[5] is not finite"),
                 lag_inf=(dict(lag=np.where(np.arange(order + 1) == 1, np.inf, 1.0)), b"lagWindow[1] is not finite"), stride_short=(dict(stride=mostSteps - 1), b"below the largest step count"),
                 misaligned=(dict(ptr=out.data_ptr() + 4), b"aligned"), misaligned_float=(dict(ptr=out.data_ptr() + 2, fmt=1), b"aligned"))
    for name, (kw, words) in cases.items():
        refused(name, analysis, b"exportLpc", words, **kw)
    cases = dict(shared, what_2=(dict(what=2), b"what 2"), coeff_format=(dict(cfmt=2), b"coefficient format 2"), col0_negative=(dict(col0=-1), b"columns -1"),
                 col0_beyond=(dict(col0=2), b"columns 2 .. 9 of 9"), coeff_stride_short=(dict(cstride=mostSteps - 1), b"coeffStride %d is below the largest step count" % (mostSteps - 1)),
                 coeff_stride_negative=(dict(cstride=-1), b"coeffStride -1"), coeff_host=(dict(cptr=host.ctypes.data), b"coefficients"), no_coeff=(dict(cptr=None), b"no coefficients"),
                 coeff_misaligned=(dict(cptr=coeff.data_ptr() + 4), b"aligned"), coeff_too_small=(dict(cstride=1 << 34), b"coefficients"), coeff_stride_wraps_to_nothing=(dict(cstride=1 << 62, utterances=utt[:4]), b"coeffStride 4611686018427387904"),
                 coeff_stride_wraps_to_little=(dict(cstride=(1 << 61) + 1, utterances=utt[:8]), b"coeffStride 2305843009213693953"), coeff_stride_most=(dict(cstride=(1 << 63) - 1), b"coeffStride 9223372036854775807"),
                 stride_short=(dict(stride=most - 1), b""), misaligned=(dict(ptr=res.data_ptr() + 1), b"aligned"),
                 overlap=(dict(ptr=coeff.data_ptr() + 64), b"overlaps the coefficients"))
    for name, (kw, words) in cases.items():
        refused(name, inverse, b"exportLpcResidual", words, **kw)
    if torch.cuda.device_count() > 1:
        other = torch.zeros(s.n * most, dtype=torch.float64, device="cuda:%d" % ((bp.device + 1) % torch.cuda.device_count()))
        refused("another device's memory", analysis, b"exportLpc", b"memory of device", ptr=other.data_ptr())
        refused("another device's coefficients", inverse, b"exportLpcResidual", b"memory of device", cptr=other.data_ptr())
    # a signal's table, and the output on the signal
    x = torch.zeros((4, 1000), dtype=torch.int16, device=dev)
    extent = np.full(4, 1000, np.int64)

    def of(rec=None, rows=None, which="analysis", **fields):
        if rec is None:
            rec = record(sp, x.data_ptr(), 0, 4, 1000, extent)
            for key, v in fields.items():
                rec[key] = v
            rec = rec.ctypes.data
        if which == "analysis":
            return L.speechPlayer_batch_exportLpcOf(bp._h, rec, p(rows), 0 if rows is None else len(rows), order, nWin, hop, 0, None, None, 10, out.data_ptr(), 0, 10, None)
        return L.speechPlayer_batch_exportLpcResidualOf(bp._h, rec, p(rows), 0 if rows is None else len(rows), order, hop, 0, coeff.data_ptr(), 0, cols, 0, 10, 0, res.data_ptr(), 0, 1000, None)

    bad_extent = np.array([1000, 1001, 0, 0], np.int64)
    for which, entry, mine in (("analysis", b"exportLpcOf", out), ("inverse", b"exportLpcResidualOf", res)):
        for name, kw, words in (("no signal", dict(rec=0), b"no signal"), ("signal format", dict(format=2), b"signal format 2"), ("signal rows", dict(nRows=-1), b"nRows"),
                                ("no extent", dict(extent=0), b"extent"), ("extent beyond the stride", dict(extent=bad_extent.ctypes.data), b"extent[1]"),
                                ("no data", dict(data=0), b"without data"), ("host data", dict(data=host.ctypes.data), b""), ("row beyond", dict(rows=np.array([4], np.int64)), b"rows[0] = 4"),
                                ("the output is the signal", dict(data=mine.data_ptr()), b"overlaps the signal")):
            refused(name, of, entry, words, which=which, **kw)
    # nothing to write needs no buffer; and the batch is as usable as before
    assert analysis(ptr=None, utterances=utt[:0]) == 0 and inverse(ptr=None, cptr=None, utterances=utt[:0]) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert of() == 4 * 10 * 9 and of(which="inverse") == 4000
    torch.cuda.synchronize()
    assert not out[:360].cpu().numpy().view(np.uint64).any() and not res[:4000].any()      # silence: +0 everywhere
    out.copy_(canary_out); res.copy_(canary_res)
    assert analysis() == s.n * mostSteps * cols and inverse() == s.n * most
    torch.cuda.synchronize()
    got, got_res = out[:s.n * mostSteps * cols].view(s.n, mostSteps, cols).cpu().numpy(), res[:s.n * most].view(s.n, most).cpu().numpy()
    quarter = np.full((mostSteps, order), 0.25)
    for u in range(s.n):
        w = eng.pcmLpc(pcm[u], order=order, nWin=nWin, hop=hop, window=window, lagWindow=lag, fields=("lpc", "error"))
        assert np.array_equal(bits(got[u, :len(w)]), bits(w)) and not bits(got[u, len(w):]).any(), u
        w = eng.pcmLpcResidual(pcm[u], quarter[:steps[u]], hop=hop, dtype=np.int16)
        assert same(got_res[u, :len(w)], w) and not got_res[u, len(w):].any(), u
    assert torch.equal(out[s.n * mostSteps * cols:], canary_out[s.n * mostSteps * cols:]) and torch.equal(res[s.n * most:], canary_res[s.n * most:]) and torch.equal(coeff, canary_coeff)
    # seventeen exports in flight: every slot, and one more
    outs = [bp.lpcTensor(order=4 + i, nWin=128, hop=200, padded=False, dtype=torch.float64) for i in range(17)]
    torch.cuda.synchronize()
    for i, (o, offsets) in enumerate(outs):
        for u, g in enumerate(rows_of(o, offsets, False)[0]):
            assert np.array_equal(bits(g), bits(eng.pcmLpc(pcm[u], order=4 + i, nWin=128, hop=200))), (i, u)
    set_host(bp, s.b)      # a set call makes the PCM stale again
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.lpcTensor()
    with pytest.raises(RuntimeError, match="not been synthesised"):
        bp.lpcResidualTensor(coeff.view(s.n, mostSteps, cols), order=order, hop=hop)
    with pytest.raises(ValueError, match="cuda"):
        bp.lpcResidualTensor(torch.zeros((s.n, mostSteps, cols)), order=order, hop=hop)
    with pytest.raises(ValueError, match="columns"):
        bp.lpcResidualTensor(coeff.view(s.n, mostSteps, cols), order=order, hop=hop, column=2)
    with pytest.raises(ValueError, match="steps"):
        bp.lpcResidualTensor(coeff.view(s.n, mostSteps, cols)[:, :5].contiguous(), order=order, hop=hop)
    bp.close()


# ---- 5. past elements 2^31 and 2^32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("name", ["analysis32", "analysis64", "residual"])
def test_far_outputs(name, padded):
    """exportLpc (order 8, nWin 64, hop 16, every field: 27 values a step; float32 past elements 2^31 and 2^32, float64 past 2^31) and
    exportLpcResidual (int16, the coefficients of the same periodic selection read from a tensor of the analysis' own) with the periodic
    selection of tests/far_offsets.py: every later cycle is the first on the device, the first, the straddling and the last are the
    host's."""
    import torch
    import nvspeechplayer_amd as eng
    from tests.test_gpu_far_offsets import ORDER, Export
    s = compared("plain")
    bp, pcm = player(s.b, s.sr)
    lens = np.array([len(p) for p in pcm], np.int64)
    if name != "residual":
        dtype, npt = (torch.float32, np.float32) if name == "analysis32" else (torch.float64, np.float64)
        kw = dict(order=8, nWin=64, hop=16, fields=ALL)
        case = Export((27,), npt, -(-lens // 16), lambda sel, pad: bp.lpcTensor(utterances=sel, dtype=dtype, padded=pad, **kw), [eng.pcmLpc(p, **kw).astype(npt) for p in pcm])
        case.run(bp, padded, (name,))
    else:
        kw = dict(order=2, hop=160, phase=0)
        plan = plan_cycles(lens, 1, (B31, B32), padded, ORDER)      # (the plan Export.run makes: the coefficients are those of its selection)
        lpc, _ = bp.lpcTensor(nWin=64, fields="lpc", utterances=plan.selection(), dtype=torch.float32, padded=padded, **kw)
        rows = [eng.pcmLpcResidual(p, eng.pcmLpc(p, nWin=64, fields="lpc", **kw).astype(np.float32), dtype=np.int16, **{k: kw[k] for k in ("hop", "phase")}) for p in pcm]
        case = Export((), np.int16, lens, lambda sel, pad: bp.lpcResidualTensor(lpc, utterances=sel, dtype=torch.int16, padded=pad, **kw), rows)
        got = case.run(bp, padded, (name,))[0]
        assert got.cycle == plan.cycle and got.repeats == plan.repeats
    bp.close()
    torch.cuda.empty_cache()
