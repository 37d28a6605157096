"""Signal stages on the step grid, on the device (include/speechPlayer_batch.h, "Signal stages on the step grid":
speechPlayer_batch_stageLpc / stagePitch, speechPlayer_stage_push; BatchPlayer.lpcStage / pitchStage, SignalStage, SignalChain with a fan;
csrc/klatt_stage_frames.h): for every row, the outputs of its pushes up to the one that ends it, concatenated, against the host's
whole-signal statement -- signalLpc, signalPitch -- on the concatenation of its chunks, BIT FOR BIT in every field.  Chunks are int16 or
float32, padded or packed, with poison around and between the rows; outputs float32 or float64, padded or packed, between guards.  The
inputs are tests/stage_frames.py's (run_stream of tests/test_gpu_stage.py draws its own, so its loop is restated here around them);
tests/test_stage_frames_host.py holds, without a GPU, that they run every stage of the recursion, hold silent steps, and hold voiced and
unvoiced steps.  Streams past 2^31 and 2^32 samples are tests/test_gpu_stage_frames_far.py.  Needs a GPU."""
import numpy as np
import pytest

from tests import stage_frames as sf
from tests.test_filter_host import TELEPHONE
from tests.test_gpu_signal import record
from tests.test_gpu_stage import ERR_ARGUMENT, F32, FORMS, bare, check_segments, same  # noqa: F401  (bare is a fixture)
from tests.test_gpu_stage_window import SpecRaw

pytestmark = pytest.mark.gpu


def p(a):
    return None if a is None else a.ctypes.data


def lpc_args(g):
    order, nWin, hop, phase, what, lag = g
    return order, nWin, hop, phase, None, sf.lag_window(order) if lag else None, what


def lpc_statement(g):
    import nvspeechplayer_amd as eng
    order, nWin, hop, phase, _, lag, what = lpc_args(g)
    return lambda x: eng.signalLpc(x, order, nWin, hop, phase, lagWindow=lag, fields=what)


def pitch_statement(g):
    import nvspeechplayer_amd as eng
    W, lagMin, lagMax, hop, phase, what = g
    return lambda x: eng.signalPitch(x, sf.PITCH_RATE, nWin=W, hop=hop, phase=phase, threshold=sf.PITCH_THRESHOLD, fields=what, lagMin=lagMin, lagMax=lagMax)


def make_lpc(L, batch, n, g):
    order, nWin, hop, phase, _, lag, what = lpc_args(g)
    return L.speechPlayer_batch_stageLpc(batch, n, order, nWin, hop, phase, None, p(lag), what)


def make_pitch(L, batch, n, g):
    W, lagMin, lagMax, hop, phase, what = g
    return L.speechPlayer_batch_stagePitch(batch, n, sf.PITCH_RATE, W, lagMin, lagMax, sf.PITCH_THRESHOLD, hop, phase, what)


def run_frames(raw, n, case):
    """run_stream of tests/test_gpu_stage.py around the chunks of tests/stage_frames.py: push after push, formats and layouts alternating
    (FORMS) -> per row its segments, a segment closing at the row's end."""
    lens, end, _, _, _, seed = case
    segments = [[dict(x=[], out=[])] for _ in range(n)]
    for k, (rows, ls, e) in enumerate(zip(sf.pushes(n, *case), lens, end)):
        assert rows[0].dtype == (np.int16, F32)[(k + seed) % 2] and [len(r) for r in rows] == ls
        form = dict(FORMS[(k + seed) % len(FORMS)])
        if form["in_stride"] < 0:
            form["in_stride"] = max(ls) + 5
        got = raw.push(rows, e, **form)()
        for i in range(n):
            seg = segments[i][-1]
            seg["x"].append(sf.x_of(rows[i]))
            seg["out"].append((form["fmt"], got[i]))
            if e[i]:
                segments[i].append(dict(x=[], out=[]))
    assert all(not s[-1]["x"] for s in segments)      # the last push ended every row
    return [s[:-1] for s in segments]


def stream_case(bare, handle, n, cols, case, emitted, statement, tag):
    from nvspeechplayer_amd import _native
    L = _native.load()
    raw = SpecRaw(bare, handle, n, cols)
    lens, end = case[:2]
    # the counts, from the host's closed form alone
    N, counts = np.zeros(n, np.int64), []
    for ls, e in zip(lens, end):
        counts.append([emitted(int(N[i]) + ls[i], bool(e[i])) - emitted(int(N[i]), False) for i in range(n)])
        N = np.where(e, 0, N + np.array(ls))
    segments = run_frames(raw, n, case)      # (every push's counts are speechPlayer_stage_plan's: SpecRaw.push)
    total = 0
    for i in range(n):
        got = [len(g[0]) for seg in segments[i] for _, g in seg["out"]]
        assert got == [c[i] for c in counts], tag + (i,)
        total += sum(got)
    assert total > 0
    consumed, emitted_ = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    assert L.speechPlayer_stage_counts(raw.h, p(consumed), p(emitted_)) == 0 and not consumed.any() and not emitted_.any()
    raw.free()
    check_segments(segments, lambda i, x, fmt: (statement(x).astype(F32 if fmt else np.float64),), tag)


# ---- 1. the two kinds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("g", sf.LPC_GEOMETRY)
def test_lpc_pushes_concatenate_to_the_statement(bare, g, n):
    """Four geometries -- an odd window whose 3000-sample pushes emit 375 steps, so groups of 64 straddle rows; a lag window; a hop above
    the frame and a phase, order 32 (four lag blocks of 8 and one lag more); a short second lag block -- on 1, 3 and 5 rows; seven pushes
    of chunk lengths drawn unsorted from {0, 1, H - 1, H, H + 1, hop, 1023, 3000}, rows ending at different pushes and going on as fresh
    rows; int16 and float32 chunks, float32 and float64, padded and packed outputs alternate.  Every field is signalLpc's bit for bit, the
    steps per push the difference of lpcEmitted, padding +0, and the counts zeros behind the last end."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    order, nWin, hop, phase, what = g[:5]
    cols = sp.lpcColumns(what, order)[1]
    stream_case(bare, make_lpc(_native.load(), bare._h, n, g), n, cols, sf.lpc_case(g, n), lambda N, ended: eng.lpcEmitted(N, nWin, hop, phase, ended=ended),
                lpc_statement(g), ("lpc", g[:4], n))


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("g", sf.PITCH_GEOMETRY)
def test_pitch_pushes_concatenate_to_the_statement(bare, g, n):
    """Four geometries -- four lags a lane and two scan blocks with the CMND curve among the fields, groups of 16 straddling rows; six lags a
    lane; four at their boundary lagMax 256 with a hop above the frame; six at theirs, lagMax 257 -- as the LPC case: every field is
    signalPitch's bit for bit, the steps per push the difference of pitchEmitted."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    W, lagMin, lagMax, hop, phase, what = g
    assert sp.PITCH_GROUP == 16
    cols = sp.pitchColumns(what, lagMin, lagMax)[1]
    stream_case(bare, make_pitch(_native.load(), bare._h, n, g), n, cols, sf.pitch_case(g, n), lambda N, ended: eng.pitchEmitted(N, W, lagMax, hop, phase, ended=ended),
                pitch_statement(g), ("pitch", g[:5], n))


# ---- 2. rows at unlike depths in one workgroup ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lpc", "pitch"])
def test_rows_at_unequal_depths_share_a_workgroup(bare, kind):
    """Five rows; a push of 1200 samples, two pushes of 300 and 150 -- both shorter than the history, so the next history mixes old
    history and chunk --, a reset of rows [0, 1, 0, 1, 1], and a push of 700 that ends every row: its steps of all five rows, at M > 0 and
    at M = 0, share one workgroup.  Rows 0 and 2 are the statement of their 2350 samples, rows 1, 3 and 4 of the last 700 alone."""
    import torch
    g = sf.LPC_GEOMETRY[1] if kind == "lpc" else sf.PITCH_GEOMETRY[1]
    if kind == "lpc":
        order, nWin, hop, phase, window, lag, what = lpc_args(g)
        stage, statement, H = bare.lpcStage(5, order, nWin, hop, phase, window, lag, what), lpc_statement(g), nWin - 1
    else:
        W, lagMin, lagMax, hop, phase, what = g
        stage = bare.pitchStage(5, sf.PITCH_RATE, nWin=W, hop=hop, phase=phase, threshold=sf.PITCH_THRESHOLD, fields=what, lagMin=lagMin, lagMax=lagMax)
        statement, H = pitch_statement(g), W + lagMax - 1
    assert stage.columns == statement(np.zeros(3000, F32)).shape[1] and 300 < H and stage.kind == kind
    period, frame = (sf.lpc_period(g), H + 1) if kind == "lpc" else (sf.pitch_period(g), H + 1)
    whole = [sf.chunk(i, 0, 0, 2350, F32, period, frame, hop, 77) for i in range(5)]
    outs, at = [], 0
    for k, c in enumerate((1200, 300, 150, 700)):
        if k == 3:
            stage.reset(np.array([False, True, False, True, True]))
            assert list(stage.consumed) == [1650, 0, 1650, 0, 0] and stage.emitted[0] > 0 and not stage.emitted[1]
        x = np.stack([w[at:at + c] for w in whole])
        out, counts = stage.push((torch.from_numpy(x).to("cuda:%d" % bare.device), np.full(5, c)), end=k == 3, dtype=torch.float64)
        assert out.dtype == torch.float64 and out.shape[0] == 5 and out.shape[2] == stage.columns
        outs.append([out[i, :counts[i]].cpu().numpy() for i in range(5)])
        at += c
    for i in range(5):
        kept = i in (0, 2)
        got = np.concatenate([o[i] for o in outs]) if kept else outs[3][i]
        assert same(got, statement(whole[i] if kept else whole[i][1650:])), (kind, i)
    assert not stage.consumed.any() and not stage.emitted.any()
    stage.close()


# ---- 3. the fan on live handles ------------------------------------------------------------------------------------------------------------------
def test_the_fan_at_the_end_of_a_live_chain():
    """Three live handles speaking different utterances, pulled 137, 8192 and 1 samples, through SignalChain([filterStage(TELEPHONE),
    resampleStage(22050 -> 16000), (lpcStage, pitchStage(16000), codeStage("ulaw"))]), end=True on the last push: per handle the LPC
    fields, the pitch and the mu-law samples are signalLpc, signalPitch and signalCode of signalResample(signalFilter(pcm)) of what was
    pulled, bit for bit, float32 between the stages."""
    import torch
    import nvspeechplayer_amd as eng
    from tests import scenarios
    ref = scenarios.Ref()
    n = 3
    players = [eng.SpeechPlayer(22050, noiseSeed=11 + k) for k in range(n)]
    for k, pl in enumerate(players):
        for fr, m, f in ref.ipa_case((7 * k + 1) % len(ref.ipa_meta)):
            pl.queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f)
    group = eng.LiveGroup(players)
    bp = eng.BatchPlayer(22050)
    fan = (bp.lpcStage(n), bp.pitchStage(n, 16000), bp.codeStage(n, "ulaw"))
    with pytest.raises(ValueError, match="an lpc stage comes last"):
        eng.SignalChain([fan[0], bp.filterStage(n, TELEPHONE)])
    chain = eng.SignalChain([bp.filterStage(n, TELEPHONE), bp.resampleStage(n, 22050, 16000), fan])
    pcm, lpc, pitch, code = ([[] for _ in range(n)] for _ in range(4))
    for k, pull in enumerate((137, 8192, 1)):
        out, produced = group.pullTensor(pull, dtype=torch.int16)
        produced = produced.copy()
        assert produced.max() <= pull and (k > 0 or list(produced) == [137] * n)
        (a, na), (b, nb), (c, nc) = chain.push((out, produced), end=k == 2)
        assert a.dtype == b.dtype == torch.float32 and c.dtype == torch.int16 and a.shape[2] == 17 and b.shape[2] == 2
        rows, a, b, c = out.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
        for i in range(n):
            pcm[i].append(rows[i, :produced[i]])
            lpc[i].append(a[i, :na[i]])
            pitch[i].append(b[i, :nb[i]])
            code[i].append(c[i, :nc[i]])
            assert not a[i, na[i]:].view(np.uint32).any() and not b[i, nb[i]:].view(np.uint32).any() and not c[i, nc[i]:].any()
    for i in range(n):
        y = eng.signalResample(eng.signalFilter(np.concatenate(pcm[i]), TELEPHONE), 22050, 16000)
        assert len(y) > 600
        assert same(np.concatenate(lpc[i]), eng.signalLpc(y).astype(F32)), i
        assert same(np.concatenate(pitch[i]), eng.signalPitch(y, 16000).astype(F32)), i
        assert same(np.concatenate(code[i]), eng.signalCode(y, "ulaw")), i
    assert all(not s.consumed.any() and not s.emitted.any() for s in chain.stages)
    chain.reset()
    for s in chain.stages:
        s.close()
    bp.close()
    for pl in players:
        pl.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lpc", "pitch"])
def test_refusals_write_nothing_and_leave_the_state_as_it_was(kind):
    """The makers' refusals, the 2^27 cap among them, and of a push: a wrong row count, an output that overlaps the chunk, deviceCodes, a
    freed stage.  After each refusal nothing is written, the counts are what they were, and the next pushes still concatenate to the
    statement."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    bp = eng.BatchPlayer(22050)
    dev = "cuda:%d" % bp.device
    n, c = 3, 500
    g = sf.LPC_GEOMETRY[0] if kind == "lpc" else sf.PITCH_GEOMETRY[0]
    name = b"stageLpc" if kind == "lpc" else b"stagePitch"

    def not_made(h, word):
        assert h is None and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and name in L.speechPlayer_lastError() and word in L.speechPlayer_lastError(), L.speechPlayer_lastError()

    if kind == "lpc":
        make = lambda rows=n, batch=bp._h: make_lpc(L, batch, rows, g)
        statement, per = lpc_statement(g), sp.lpcColumns(g[4], g[0])[1]
        emitted = lambda N: eng.lpcEmitted(N, g[1], g[2], g[3])
        for args, word in (((0, 33, 8, 0, None, None, 31), b"order"), ((33, 64, 8, 0, None, None, 31), b"order"), ((4, 4, 8, 0, None, None, 31), b"nWin"),
                           ((4, 4097, 8, 0, None, None, 31), b"nWin"), ((4, 33, 0, 0, None, None, 31), b"hop"), ((4, 33, 8, -1, None, None, 31), b"phase"),
                           ((4, 33, 8, 0, None, None, 0), b"what"), ((4, 33, 8, 0, None, None, 32), b"what"),
                           ((4, 33, 8, 0, p(np.full(33, np.inf)), None, 31), b"window"), ((4, 33, 8, 0, None, p(np.full(5, np.nan)), 31), b"lagWindow")):
            not_made(L.speechPlayer_batch_stageLpc(bp._h, n, *args), word)
        not_made(L.speechPlayer_batch_stageLpc(bp._h, 1 << 20, 4, 4096, 8, 0, None, None, 31), b"2^27")      # before anything is allocated
    else:
        make = lambda rows=n, batch=bp._h: make_pitch(L, batch, rows, g)
        statement, per = pitch_statement(g), 5 + g[2] - g[1] + 1
        emitted = lambda N: eng.pitchEmitted(N, g[0], g[2], g[3], g[4])
        for args, word in (((0, 32, 2, 65, 0.1, 8, 0, 63), b"sampleRate"), ((16000, 31, 2, 65, 0.1, 8, 0, 63), b"nWin"), ((16000, 2049, 2, 65, 0.1, 8, 0, 63), b"nWin"),
                           ((16000, 32, 1, 65, 0.1, 8, 0, 63), b"lagMin"), ((16000, 32, 65, 65, 0.1, 8, 0, 63), b"lagMin"), ((16000, 32, 2, 1025, 0.1, 8, 0, 63), b"lagMax"),
                           ((16000, 32, 2, 65, 1.5, 8, 0, 63), b"threshold"), ((16000, 32, 2, 65, float("nan"), 8, 0, 63), b"threshold"),
                           ((16000, 32, 2, 65, 0.1, 0, 0, 63), b"hop"), ((16000, 32, 2, 65, 0.1, 8, -1, 63), b"phase"), ((16000, 32, 2, 65, 0.1, 8, 0, 0), b"what"),
                           ((16000, 32, 2, 65, 0.1, 8, 0, 64), b"what")):
            not_made(L.speechPlayer_batch_stagePitch(bp._h, n, *args), word)
        not_made(L.speechPlayer_batch_stagePitch(bp._h, 1 << 20, 16000, 2048, 2, 1024, 0.1, 8, 0, 63), b"2^27")
    for rows in (0, -1, (1 << 20) + 1):
        not_made(make(rows=rows), b"")
    not_made(make(batch=None), b"no batch")

    h = make()
    assert h, L.speechPlayer_lastError()
    period, frame, hop = (sf.lpc_period(g), g[1], g[2]) if kind == "lpc" else (sf.pitch_period(g), g[0] + g[2], g[3])
    whole = [sf.chunk(i, 0, 0, 3 * c, F32, period, frame, hop, 5) for i in range(n)]
    chunks = [np.stack([w[k * c:(k + 1) * c] for w in whole]) for k in range(3)]
    data = [torch.from_numpy(x).to(dev) for x in chunks]
    extent = np.full(n, c, np.int64)
    width = c // hop + 12      # steps
    out = torch.full((n * width * per + 8,), -7.0, dtype=torch.float32, device=dev)
    cod = torch.full((n * width + 8,), 0x55, dtype=torch.uint8, device=dev)
    sentinel, sentinel_codes = out.clone(), cod.clone()
    lengths = np.zeros(n, np.int64)

    def push(k=0, handle=0, end=None, ptr=0, fmt=1, codes=None, stride=width, **sig):
        s = dict(data=data[k].data_ptr(), format=1, nRows=n, rowStride=c, extent=extent)
        s.update(sig)
        rec = record(sp, s["data"], s["format"], s["nRows"], s["rowStride"], s["extent"])
        return L.speechPlayer_stage_push(h if handle == 0 else handle, rec.ctypes.data, p(end), out.data_ptr() if ptr == 0 else ptr, fmt, codes, stride, lengths.ctypes.data, None)

    def rows_of(elements):
        torch.cuda.synchronize()
        counts = lengths.copy()
        got = out[:n * width * per].view(n, width, per).cpu().numpy()
        assert elements == n * width * per and not got[:, counts.max():].view(np.uint32).any(), L.speechPlayer_lastError()
        out.copy_(sentinel)
        return [got[i, :counts[i]].copy() for i in range(n)]

    first = rows_of(push(0))
    freed = make()
    L.speechPlayer_stage_free(freed)
    big = torch.cat([data[1].reshape(-1), torch.zeros(n * width * per, dtype=torch.float32, device=dev)])      # the chunk, and room behind it for an output
    consumed, emitted_ = np.zeros(n, np.int64), np.zeros(n, np.int64)
    cases = dict(no_stage=dict(handle=None), freed=dict(handle=freed), rows_fewer=dict(nRows=n - 1), rows_more=dict(nRows=n + 1, extent=np.full(n + 1, c, np.int64)),
                 format_2=dict(fmt=2), stride_negative=dict(stride=-1), stride_short=dict(stride=1), no_buffer=dict(ptr=None),
                 output_on_the_chunk=dict(data=big.data_ptr(), ptr=big.data_ptr()), output_into_the_chunk=dict(data=big.data_ptr(), ptr=big.data_ptr() + 4 * (n * c - 8)),
                 codes_on_a_frame_kind=dict(codes=cod.data_ptr()))
    for tag, kw in cases.items():
        kw.setdefault("k", 1)
        assert push(**kw) == -1, tag
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"stage_push" in L.speechPlayer_lastError(), (tag, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel) and torch.equal(cod, sentinel_codes), tag
        assert L.speechPlayer_stage_counts(h, p(consumed), p(emitted_)) == 0 and list(consumed) == [c] * n and list(emitted_) == [emitted(c)] * n, tag
    assert torch.equal(big[:n * c], data[1].reshape(-1)) and not big[n * c:].any()
    # nothing moved: the stream goes on, ends, and equals the statement
    second = rows_of(push(1))
    third = rows_of(push(2, end=np.ones(n, np.uint8)))
    for i in range(n):
        got = np.concatenate([first[i], second[i], third[i]])
        assert same(got, statement(whole[i]).astype(F32)), (kind, i)
    assert torch.equal(out[n * width * per:], sentinel[n * width * per:])
    L.speechPlayer_stage_free(h)
    bp.close()
