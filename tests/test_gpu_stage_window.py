"""Signal stages that keep a window, on the device (include/speechPlayer_batch.h, "Signal stages that keep a window":
speechPlayer_batch_stageConvolve / stageSpectrogram, speechPlayer_stage_push; BatchPlayer.convolveStage / spectrogramStage, SignalStage,
SignalChain; csrc/klatt_stage_window.h): for every row, the outputs of its pushes up to the one that ends it, concatenated, against the
host's whole-signal statement -- signalConvolve, signalSpectrogram -- on the concatenation of its chunks: bit for bit for the convolution
and for the spectrogram's linear values, at tests/test_gpu_spectrogram.py's bar through the logarithm.  Chunks are int16 or float32, padded
or packed, with poison around and between the rows; outputs padded or packed, between guards.  Every stream here is short: streams past
2^31 and 2^32 samples, and chunks and outputs past those elements, are tests/test_gpu_stage_far.py.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_filter_host import TELEPHONE
from tests.test_gpu_signal import edge_rows, lay_out, poison, record
from tests.test_gpu_stage import ERR_ARGUMENT, F32, FORMS, GUARD, Raw, bare, check_segments, run_stream, same, x_of  # noqa: F401  (bare is a fixture)
from tests.test_spectrogram_host import ulps

pytestmark = pytest.mark.gpu
TAPS = [1, 2, 5, 1023, 1024, 1025, 2500]      # 2500 spans three tap blocks
GEOMETRY = [(64, 16, 0), (64, 80, 5), (512, 160, 0), (512, 512, 300)]      # nFft, hop, phase: 80 is above nFft = 64, samples are skipped


def response(K, seed):
    rng = np.random.default_rng(seed)
    h = (rng.normal(0.0, 1.0, K) * np.exp(-np.arange(K) / (0.3 * K + 1.0))).astype(F32)
    h[2::7] = 0.0      # zero taps among them
    return h


def ends_for(n, pushes, seed):
    """Rows end at different pushes and go on afterwards as fresh rows; the last push ends them all."""
    end = np.zeros((pushes, n), np.uint8)
    for i in range(n):
        end[2 + (i + seed) % (pushes - 3), i] = 1
    end[-1, :] = 1
    return end


class SpecRaw(Raw):
    """Raw for a spectrogram stage: the output is [row][step][bands], float64 (fmt 0) or float32 (fmt 1), rowStride in steps."""

    def __init__(self, bp, handle, n, bands):
        Raw.__init__(self, bp, handle, n)
        self.bands = bands

    def push(self, rows, end, in_stride=0, in_shift=0, fmt=1, form="packed", shift=0, stream=None):
        import torch
        npt = rows[0].dtype.type
        assert all(r.dtype == npt for r in rows) and len(rows) == self.n
        host, first, extent = lay_out(rows, npt, in_stride, poison, in_shift)
        data = torch.from_numpy(host.view(np.int32 if npt == F32 else np.int16)).to(self.dev)
        rec = record(self.sp, data.data_ptr() + first * data.element_size(), 1 if npt == F32 else 0, self.n, in_stride, extent)
        flags = None if end is None else np.ascontiguousarray(np.asarray(end, np.uint8))
        counts = self.plan([len(r) for r in rows], flags)
        stride = 0 if form == "packed" else int(counts.max()) + 3
        steps = int(counts.sum()) if stride == 0 else self.n * stride
        elements = steps * self.bands
        buf = torch.full((elements + 2 * GUARD + shift,), -7, dtype=torch.float32 if fmt else torch.float64, device=self.dev)
        lengths = np.full(self.n, -1, np.int64)
        got = self.L.speechPlayer_stage_push(self.h, rec.ctypes.data, None if flags is None else flags.ctypes.data,
                                             None if elements == 0 else buf.data_ptr() + (GUARD + shift) * buf.element_size(), fmt, None, stride, lengths.ctypes.data, stream)
        assert got == elements, (got, elements, self.L.speechPlayer_lastError())
        assert list(lengths) == list(counts)      # what the push emitted is what the plan said
        torch.cuda.synchronize()
        held = (data, rec, extent)
        return lambda: self._steps(buf, counts, stride, elements, shift, held)

    def _steps(self, buf, counts, stride, elements, shift, held):
        got = buf.cpu().numpy()
        assert np.all(got[:GUARD + shift] == -7) and np.all(got[GUARD + shift + elements:] == -7), "guards"
        got = got[GUARD + shift:GUARD + shift + elements].reshape(-1, self.bands)
        rows, at = [], 0
        for c in counts:
            span = int(c) if stride == 0 else stride
            rows.append((got[at:at + c].copy(), None))
            assert not np.ascontiguousarray(got[at + c:at + span]).view(np.uint8).any(), "padding is +0"
            at += span
        return rows


# ---- 1. the convolution ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_convolution_pushes_concatenate_to_the_statement(bare, n, tail):
    """Responses of 1, 2, 5, 1023, 1024, 1025 and 2500 taps cycled over 1, 3 and 5 rows; seven pushes of chunk lengths drawn unsorted from
    {0, 1, K - 2, K - 1, K, 1023, 1025, 3000}, K the row's own; rows end at different pushes and go on as fresh rows, the last push ends
    all; int16 and float32 chunks alternate, the outputs alternate between padded and packed and between int16 and float32, between
    guards.  Bit for bit signalConvolve; every push's counts are speechPlayer_stage_plan's (Raw.push) and c, + K - 1 behind an end with tail."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    of = ((np.arange(n) * 3 + n + tail) % len(TAPS)).astype(np.int64)
    irs = [response(K, 80 + K) for K in TAPS]
    flat, start = np.concatenate(irs), np.concatenate([[0], np.cumsum(TAPS)]).astype(np.int64)
    raw = Raw(bare, L.speechPlayer_batch_stageConvolve(bare._h, n, flat.ctypes.data, start.ctypes.data, len(TAPS), of.ctypes.data, tail), n)
    rng = np.random.default_rng(17 * n + tail)
    pools = [[0, 1, max(TAPS[j] - 2, 0), TAPS[j] - 1, TAPS[j], 1023, 1025, 3000] for j in of]
    lens = [[int(pools[i][rng.integers(0, 8)]) for i in range(n)] for _ in range(7)]
    end = ends_for(n, 7, n + tail)
    segments = run_stream(raw, lens, end, n + tail)
    for i in range(n):
        got = [len(g[0]) for seg in segments[i] for _, g in seg["out"]]
        assert got == [ls[i] + (TAPS[of[i]] - 1 if e[i] and tail else 0) for ls, e in zip(lens, end)], (n, tail, i)
    consumed, emitted = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    assert L.speechPlayer_stage_counts(raw.h, consumed.ctypes.data, emitted.ctypes.data) == 0 and not consumed.any() and not emitted.any()
    check_segments(segments, lambda i, x, fmt: (eng.signalConvolve(x, irs[of[i]], tail=bool(tail), dtype=F32 if fmt else np.int16),), ("convolution", n, tail))
    raw.free()


def test_histories_of_unequal_lengths_at_unequal_offsets(bare):
    """Five rows whose irOf names responses of 1, 2, 5, 1025 and 2 taps: histories of 0, 1, 4, 1024 and 1 samples, at the offsets 0, 0, 1,
    5 and 1029 of either buffer, one row with none.  Two pushes of 7 and 3 float32 samples a row, both shorter than the longest history, so
    its next history mixes old history and chunk; a reset of rows [0, 1, 0, 1, 1]; a push of 9 that ends every row.  Rows 0 and 2 are
    signalConvolve of their 19 samples, rows 1, 3 and 4 of the last 9 alone, bit for bit."""
    import torch
    import nvspeechplayer_amd as eng
    irs = [response(K, 80 + K) for K in (1, 2, 5, 1025)]
    of = [0, 1, 2, 3, 1]
    stage = bare.convolveStage(5, irs, irOf=of, tail=False)
    rng = np.random.default_rng(27)
    chunks = [rng.uniform(-1.0, 1.0, (5, c)).astype(F32) for c in (7, 3, 9)]
    outs = []
    for k, x in enumerate(chunks):
        if k == 2:
            stage.reset(np.array([False, True, False, True, True]))
            assert list(stage.consumed) == [10, 0, 10, 0, 0]
        out, counts = stage.push((torch.from_numpy(x).to("cuda:%d" % bare.device), np.full(5, x.shape[1])), end=k == 2)
        assert out.dtype == torch.float32 and list(counts) == [x.shape[1]] * 5
        outs.append(out.cpu().numpy())
    for i in range(5):
        kept = i in (0, 2)
        got = np.concatenate([o[i] for o in outs]) if kept else outs[2][i]
        x = np.concatenate([c[i] for c in chunks]) if kept else chunks[2][i]
        assert len(got) == (19 if kept else 9) and same(got, eng.signalConvolve(x, irs[of[i]], tail=False)), i
    assert not stage.consumed.any()
    stage.close()


# ---- 2. the spectrogram ----------------------------------------------------------------------------------------------------------------------
def spectrogram_stream(bare, n, geometry, bank, power, scale, floor, seed):
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    nFft, hop, phase = geometry
    bands = nFft // 2 + 1 if bank is None else len(bank)
    raw = SpecRaw(bare, L.speechPlayer_batch_stageSpectrogram(bare._h, n, nFft, hop, phase, None, None if bank is None else bank.ctypes.data,
                                                              0 if bank is None else len(bank), power, scale, floor), n, bands)
    rng = np.random.default_rng(seed)
    pool = [0, 1, hop - 1, hop, nFft // 2 - 1, nFft // 2, nFft - 1, nFft, 1000]
    lens = [[int(pool[rng.integers(0, len(pool))]) for _ in range(n)] for _ in range(7)]
    end = ends_for(n, 7, seed)
    # the counts, from the host's closed form alone
    N, counts = np.zeros(n, np.int64), []
    for ls, e in zip(lens, end):
        counts.append([eng.spectrogramEmitted(int(N[i]) + ls[i], nFft, hop, phase, ended=bool(e[i])) - eng.spectrogramEmitted(int(N[i]), nFft, hop, phase) for i in range(n)])
        N = np.where(e, 0, N + np.array(ls))
    segments = run_stream(raw, lens, end, seed)
    total = 0
    for i in range(n):
        got = [len(g[0]) for seg in segments[i] for _, g in seg["out"]]
        assert got == [c[i] for c in counts], (geometry, n, i)
        total += sum(got)
    assert total > 0
    consumed, emitted = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    assert L.speechPlayer_stage_counts(raw.h, consumed.ctypes.data, emitted.ctypes.data) == 0 and not consumed.any() and not emitted.any()
    raw.free()
    return segments


@pytest.mark.parametrize("mel", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("geometry", GEOMETRY)
def test_spectrogram_pushes_concatenate_to_the_statement(bare, geometry, n, mel):
    """Four step grids -- a hop above nFft, a phase above the hop -- on 1, 3 and 5 rows (five rows at different M share workgroups of four
    steps), the bins and a 20-band mel bank, power 1 and 2; seven pushes of chunk lengths drawn unsorted from {0, 1, hop - 1, hop,
    nFft / 2 - 1, nFft / 2, nFft - 1, nFft, 1000}, rows ending at different pushes; float64 and float32, padded and packed outputs
    alternate.  The linear values are signalSpectrogram's bit for bit, the steps per push the difference of spectrogramEmitted, padding +0."""
    import nvspeechplayer_amd as eng
    nFft, hop, phase = geometry
    bank = eng.melFilterbank(16000, nFft, 20) if mel else None
    power = 1 + (n + mel + GEOMETRY.index(geometry)) % 2
    segments = spectrogram_stream(bare, n, geometry, bank, power, 0.0, 0.0, 3 * n + mel + 11 * GEOMETRY.index(geometry))

    def statement(i, x, fmt):
        return (eng.signalSpectrogram(x, nFft, hop, phase, bank=bank, power=power).astype(F32 if fmt else np.float64),)
    check_segments(segments, statement, (geometry, n, mel, power))


def test_both_powers_are_covered_by_the_linear_cases():
    assert {1 + (n + mel + g) % 2 for n in (1, 3, 5) for mel in (0, 1) for g in range(4)} == {1, 2}


@pytest.mark.parametrize("power", [1, 2])
def test_spectrogram_pushes_through_the_logarithm(bare, power):
    """One log case per power -- "db" of a power on the mel bank, "ln" of a magnitude on the bins --: float64 within 4 ulp of the host's
    statement, float32 within one float32 ulp of the rounded host value (each side calls its own log10)."""
    import nvspeechplayer_amd as eng
    geometry = (512, 160, 0) if power == 2 else (64, 16, 0)
    bank = eng.melFilterbank(16000, geometry[0], 20) if power == 2 else None
    scale, floor, log = (10.0, 1e-10, "db") if power == 2 else (float(np.log(10.0)), 1e-5, "ln")
    segments = spectrogram_stream(bare, 3, geometry, bank, power, scale, floor, 40 + power)
    checked = 0
    for i, row in enumerate(segments):
        for seg in row:
            x = np.concatenate(seg["x"]) if seg["x"] else np.zeros(0, F32)
            want = eng.signalSpectrogram(x, *geometry, bank=bank, power=power, log=log, floor=floor)
            at = 0
            for fmt, (g, _) in seg["out"]:
                w = want[at:at + len(g)]
                assert g.shape == w.shape and g.dtype == (F32 if fmt else np.float64), (power, i)
                if fmt == 0:
                    assert g.size == 0 or ulps(g, w).max() <= 4, (power, i, "float64")
                else:
                    w32 = w.astype(F32)
                    assert np.all(np.abs(g.astype(np.float64) - w32) <= np.spacing(np.abs(w32)).astype(np.float64)), (power, i, "float32")
                at += len(g)
                checked += g.size
            assert at == len(want), (power, i, "length")
    assert checked > 0


# ---- 3. the stage kernel against the whole-row kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "padded"])
@pytest.mark.parametrize("kind", ["convolution", "spectrogram"])
def test_one_push_that_ends_every_row_is_the_whole_row_export(bare, kind, form):
    """A single push that ends every row of a fresh stage writes, between its guards, exactly the bytes exportConvolvedOf /
    exportSpectrogramOf write for the same signal -- rows, padding and guards, both output formats."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    n, dev = 9, "cuda:%d" % bare.device
    p = lambda a: None if a is None else a.ctypes.data
    pool = [0, 1, 255, 256, 1023, 1025, 2100, 3000, 511]
    rng = np.random.default_rng(len(kind) + len(form))
    lens = [pool[k] for k in rng.permutation(n)]
    rows = edge_rows(lens, F32, 70 + len(kind))
    in_stride = 0 if form == "packed" else max(lens) + 5
    host, first, extent = lay_out(rows, F32, in_stride, poison, 1)
    data = torch.from_numpy(host.view(np.int32)).to(dev)
    rec = record(sp, data.data_ptr() + 4 * first, 1, n, in_stride, extent)
    if kind == "convolution":
        irs = [response(K, 80 + K) for K in TAPS]
        flat, start = np.concatenate(irs), np.concatenate([[0], np.cumsum(TAPS)]).astype(np.int64)
        of = ((np.arange(n) * 3) % len(TAPS)).astype(np.int64)
        h = L.speechPlayer_batch_stageConvolve(bare._h, n, p(flat), p(start), len(TAPS), p(of), 1)
        export = lambda d, fmt, stride: L.speechPlayer_batch_exportConvolvedOf(bare._h, p(rec), None, 0, p(flat), p(start), len(TAPS), p(of), 1, d, fmt, stride, None)
        per, types = 1, (torch.int16, torch.float32)
    else:
        bank = eng.melFilterbank(16000, 512, 20)
        h = L.speechPlayer_batch_stageSpectrogram(bare._h, n, 512, 160, 7, None, p(bank), 20, 2, 10.0, 1e-10)
        export = lambda d, fmt, stride: L.speechPlayer_batch_exportSpectrogramOf(bare._h, p(rec), None, 0, 512, 160, 7, None, p(bank), 20, 2, 10.0, 1e-10, d, fmt, stride, None)
        per, types = 20, (torch.float64, torch.float32)
    assert h, _native.last_error()
    end, counts, lengths = np.ones(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
    shift = 2
    for fmt in (1, 0):      # (the push ends every row, so the stage is fresh again for the second format)
        assert L.speechPlayer_stage_plan(h, p(np.array(lens, np.int64)), p(end), p(counts)) == counts.sum() > 0
        stride = 0 if form == "packed" else int(counts.max()) + 3
        elements = (int(counts.sum()) if stride == 0 else n * stride) * per
        bufs = {}
        for who in ("push", "export"):
            d = torch.full((elements + 2 * GUARD + shift,), -7, dtype=types[fmt], device=dev)
            bufs[who] = d
            dptr = d.data_ptr() + (GUARD + shift) * d.element_size()
            got = L.speechPlayer_stage_push(h, p(rec), p(end), dptr, fmt, None, stride, p(lengths), None) if who == "push" else export(dptr, fmt, stride)
            assert got == elements, (kind, form, fmt, who, got, elements, _native.last_error())
        assert list(lengths) == list(counts)
        torch.cuda.synchronize()
        a, b = bufs["push"].cpu().numpy(), bufs["export"].cpu().numpy()
        assert a.tobytes() == b.tobytes(), (kind, form, fmt)
        assert np.all(a[:GUARD + shift] == -7) and np.all(a[GUARD + shift + elements:] == -7), (kind, form, fmt, "guards")
        assert np.any(a[GUARD + shift:GUARD + shift + elements] != -7)
    consumed = np.full(n, -1, np.int64)
    assert L.speechPlayer_stage_counts(h, p(consumed), None) == 0 and not consumed.any()
    L.speechPlayer_stage_free(h)


# ---- 4. the chain on live handles ------------------------------------------------------------------------------------------------------------------
def test_the_chain_on_live_handles():
    """Five live handles speaking different utterances, pulled 137 samples at a time, then 8192 at a time, through SignalChain([convolveStage
    (a room), filterStage(TELEPHONE), resampleStage(22050 -> 16000), spectrogramStage(512, 160, a 20-band mel bank)]), end=True on the last
    push: per handle the steps are signalSpectrogram(signalResample(signalFilter(signalConvolve(pcm)))) of the handle's whole PCM, bit for
    bit, float32 between the stages.  A spectrogram stage that is not last is refused."""
    import torch
    import nvspeechplayer_amd as eng
    from tests import scenarios
    ref = scenarios.Ref()
    players = [eng.SpeechPlayer(22050, noiseSeed=11 + k) for k in range(5)]
    for k, p in enumerate(players):
        for fr, m, f in ref.ipa_case((7 * k + 1) % len(ref.ipa_meta)):
            p.queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f)
    group = eng.LiveGroup(players)
    bp = eng.BatchPlayer(22050)
    room, bank = response(300, 5), eng.melFilterbank(16000, 512, 20)
    stages = [bp.convolveStage(5, room), bp.filterStage(5, TELEPHONE), bp.resampleStage(5, 22050, 16000), bp.spectrogramStage(5, 512, 160, bank=bank)]
    with pytest.raises(ValueError, match="spectrogram stage comes last"):
        eng.SignalChain([stages[3], stages[1]])
    chain = eng.SignalChain(stages)
    pcm, steps = [[] for _ in range(5)], [[] for _ in range(5)]
    pulls = 0
    while True:
        out, produced = group.pullTensor(137 if pulls < 12 else 8192, dtype=torch.int16)
        produced = produced.copy()
        last = not produced.any()
        spec, counts = chain.push((out, produced), end=last)
        counts = counts.numpy()
        assert spec.dtype == torch.float32 and spec.shape[0] == 5 and spec.shape[2] == 20
        rows, spec = out.cpu().numpy(), spec.cpu().numpy()
        for i in range(5):
            pcm[i].append(rows[i, :produced[i]])
            steps[i].append(spec[i, :counts[i]])
            assert not spec[i, counts[i]:].view(np.uint32).any()
        pulls += 1
        if last:
            break
        assert pulls < 2000
    lens = {len(np.concatenate(p)) for p in pcm}
    assert len(lens) > 1 and min(lens) > 2000 and pulls > 13      # different utterances, both pull sizes
    for i in range(5):
        whole = np.concatenate(pcm[i])
        want = eng.signalSpectrogram(eng.signalResample(eng.signalFilter(eng.signalConvolve(whole, room), TELEPHONE), 22050, 16000), 512, 160, bank=bank)
        assert same(np.concatenate(steps[i]), want.astype(F32)), i
    assert not chain.stages[0].consumed.any() and not chain.stages[3].emitted.any()
    for s in chain.stages:
        s.close()
    bp.close()
    for p in players:
        p.close()


# ---- 5. ordering ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["convolution", "spectrogram"])
def test_pushes_on_two_streams_follow_one_another(bare, kind):
    """Pushes of one stage issued alternately on two torch streams, the first of them behind a busy kernel: they still concatenate to the
    statement, by the stage's events alone."""
    import torch
    import nvspeechplayer_amd as eng
    n = 3
    room = response(700, 3)
    stage = bare.convolveStage(n, room) if kind == "convolution" else bare.spectrogramStage(n, 512, 160)
    statement = (lambda x: eng.signalConvolve(x, room)) if kind == "convolution" else (lambda x: eng.signalSpectrogram(x, 512, 160).astype(F32))
    dev = bare.device
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    rng = np.random.default_rng(5)
    chunks = [rng.uniform(-1.0, 1.0, (n, 700)).astype(F32) for _ in range(6)]
    data = [torch.from_numpy(c).to("cuda:%d" % dev) for c in chunks]
    torch.cuda.synchronize()
    outs = []
    for k, t in enumerate(data):
        with torch.cuda.stream(streams[k % 2]):
            if k % 2 == 0:
                torch.cuda._sleep(20_000_000)
            outs.append(stage.push((t, np.full(n, 700)), end=k == len(data) - 1))
    torch.cuda.synchronize()
    for i in range(n):
        got = np.concatenate([o[0].cpu().numpy()[i, :o[-1][i]] for o in outs])
        assert same(got, statement(np.concatenate([c[i] for c in chunks]))), (kind, i)
    stage.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["convolution", "spectrogram"])
def test_refusals_write_nothing_and_leave_the_state_as_it_was(kind):
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    bp = eng.BatchPlayer(22050)
    dev = "cuda:%d" % bp.device
    n, c = 3, 500
    conv = kind == "convolution"
    room = response(300, 8)
    start = np.array([0, 300], np.int64)
    p = lambda a: None if a is None else a.ctypes.data
    nFft, hop = 64, 16
    per = 1 if conv else nFft // 2 + 1

    def make(rows=n, batch=0, **kw):
        b = bp._h if batch == 0 else batch
        if conv:
            a = dict(ir=room, starts=start, nIr=1, irOf=None, tail=1)
            a.update(kw)
            return L.speechPlayer_batch_stageConvolve(b, rows, p(a["ir"]), p(a["starts"]), a["nIr"], p(a["irOf"]), a["tail"])
        a = dict(nFft=nFft, hop=hop, phase=0, window=None, bank=None, nBands=0, power=2, scale=0.0, floor=0.0)
        a.update(kw)
        return L.speechPlayer_batch_stageSpectrogram(b, rows, a["nFft"], a["hop"], a["phase"], p(a["window"]), p(a["bank"]), a["nBands"], a["power"], a["scale"], a["floor"])

    def not_made(name, **kw):
        assert make(**kw) is None and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        assert (b"stageConvolve" if conv else b"stageSpectrogram") in L.speechPlayer_lastError(), name

    not_made("no batch", batch=None)
    for rows in (0, -1, (1 << 20) + 1):
        not_made("nRows", rows=rows)
    huge, nan = np.full(300, 1e10, F32), room.copy()
    nan[7] = np.nan
    if conv:
        cases = dict(tail=dict(tail=2), no_responses=dict(nIr=0), no_taps=dict(ir=None), start=dict(starts=np.array([1, 300], np.int64)),
                     empty=dict(starts=np.array([0, 0], np.int64)), too_long=dict(ir=np.zeros(65537, F32), starts=np.array([0, 65537], np.int64)),
                     tap_size=dict(ir=huge), tap_nan=dict(ir=nan), irOf=dict(irOf=np.array([0, 1, 0], np.int64)),
                     irOf_missing=dict(ir=np.tile(room, 2), starts=np.array([0, 300, 600], np.int64), nIr=2),
                     # 2^20 rows of 65535 samples of history: refused before anything is allocated
                     history=dict(rows=1 << 20, ir=np.ones(65536, F32), starts=np.array([0, 65536], np.int64)))
    else:
        cases = dict(nFft_odd=dict(nFft=100), nFft_small=dict(nFft=32), nFft_large=dict(nFft=8192), hop=dict(hop=0), phase=dict(phase=-1), power=dict(power=3),
                     bands=dict(bank=np.ones((2, 33)), nBands=0), window=dict(window=np.full(64, np.inf)), bank=dict(bank=np.full((2, 33), np.nan), nBands=2),
                     floor=dict(scale=10.0, floor=0.0), scale=dict(scale=float("inf")), history=dict(rows=1 << 20, nFft=4096))
    for name, kw in cases.items():
        not_made(name, **kw)
    assert b"2^27" in L.speechPlayer_lastError()      # (the last case: the sum is checked before the first allocation)

    h = make()
    assert h, L.speechPlayer_lastError()
    rng = np.random.default_rng(9)
    chunks = [rng.uniform(-1.0, 1.0, (n, c)).astype(F32) for _ in range(3)]
    data = [torch.from_numpy(x).to(dev) for x in chunks]
    extent = np.full(n, c, np.int64)
    width = 2 * c if conv else 40      # samples, or steps
    out = torch.full((n * width * per + 8,), -7.0, dtype=torch.float32, device=dev)
    cod = torch.full((n * width + 8,), 0x55, dtype=torch.uint8, device=dev)
    sentinel, sentinel_codes = out.clone(), cod.clone()
    host = np.zeros(n * width * per, F32)
    lengths = np.zeros(n, np.int64)

    def push(k=0, handle=0, signal=0, end=None, ptr=0, fmt=1, codes=None, stride=width, **sig):
        s = dict(data=data[k].data_ptr(), format=1, nRows=n, rowStride=c, extent=extent)
        s.update(sig)
        rec = record(sp, s["data"], s["format"], s["nRows"], s["rowStride"], s["extent"])
        return L.speechPlayer_stage_push(h if handle == 0 else handle, rec.ctypes.data if signal == 0 else signal, p(end), out.data_ptr() if ptr == 0 else ptr, fmt,
                                         codes, stride, lengths.ctypes.data, None)

    def refused(name, **kw):
        assert push(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"stage_push" in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel) and torch.equal(cod, sentinel_codes), name

    def rows_of(elements):
        torch.cuda.synchronize()
        counts = lengths.copy()
        got = out[:n * width * per].view(n, width, per).cpu().numpy()
        assert elements == n * width * per and not got[:, counts.max():].view(np.uint32).any()
        out.copy_(sentinel)
        return [got[i, :counts[i]].copy() for i in range(n)]

    first = rows_of(push(0))
    other = eng.BatchPlayer(22050)
    gone = make(batch=other._h)
    assert gone
    other.close()      # a stage goes with its batch
    freed = make()
    L.speechPlayer_stage_free(freed)
    big = torch.cat([data[1].reshape(-1), torch.zeros(n * width * per, dtype=torch.float32, device=dev)])      # the chunk, and room behind it for an output
    cases = dict(
        no_stage=dict(handle=None), freed=dict(handle=freed), freed_with_its_batch=dict(handle=gone), no_signal=dict(signal=None),
        rows_fewer=dict(nRows=n - 1), rows_more=dict(nRows=n + 1, extent=np.full(n + 1, c, np.int64)), signal_format=dict(format=2), signal_stride=dict(rowStride=-1),
        no_extent=dict(extent=None), extent_beyond=dict(extent=np.array([c, c + 1, c], np.int64)), extent_negative=dict(extent=np.array([c, -1, c], np.int64)),
        no_data=dict(data=0), host_data=dict(data=host.ctypes.data), misaligned_data=dict(data=data[1].data_ptr() + 2),
        past_2_44=dict(rowStride=1 << 44, extent=np.array([c, 1 << 44, c], np.int64)),
        format_2=dict(fmt=2), stride_negative=dict(stride=-1), stride_short=dict(stride=1), too_large=dict(stride=1 << 48),
        no_buffer=dict(ptr=None), host_memory=dict(ptr=host.ctypes.data), misaligned=dict(ptr=out.data_ptr() + 2),
        misaligned_low=dict(ptr=out.data_ptr() + (1 if conv else 4), fmt=0),
        output_on_the_chunk=dict(ptr=data[1].data_ptr(), stride=c if conv else 31),
        output_into_the_chunk=dict(data=big.data_ptr(), ptr=big.data_ptr() + 4 * (n * c - 8)),
        codes_on_another_kind=dict(codes=cod.data_ptr()))
    for name, kw in cases.items():
        kw.setdefault("k", 1)
        refused(name, **kw)
    assert torch.equal(big[:n * c], data[1].reshape(-1)) and not big[n * c:].any()
    consumed, emitted = np.zeros(n, np.int64), np.zeros(n, np.int64)
    assert L.speechPlayer_stage_counts(h, consumed.ctypes.data, emitted.ctypes.data) == 0 and list(consumed) == [c] * n
    assert list(emitted) == [c if conv else eng.spectrogramEmitted(c, nFft, hop)] * n

    def statement(x):
        return eng.signalConvolve(x, room) if conv else eng.signalSpectrogram(x, nFft, hop).astype(F32)

    # nothing moved: the stream goes on, ends, and equals the statement
    second = rows_of(push(1))
    third = rows_of(push(2, end=np.ones(n, np.uint8)))
    for i in range(n):
        x = np.concatenate([ch[i] for ch in chunks])
        got = np.concatenate([first[i], second[i], third[i]])
        assert same(got.reshape(-1), statement(x).reshape(-1)), i
    assert torch.equal(out[n * width * per:], sentinel[n * width * per:])
    # reset makes the chosen rows fresh, behind the last push
    assert push(0) == n * width * per
    rows_of(n * width * per)
    assert L.speechPlayer_stage_reset(h, np.array([1, 0, 1], np.uint8).ctypes.data, None) == 0
    assert L.speechPlayer_stage_counts(h, consumed.ctypes.data, None) == 0 and list(consumed) == [0, c, 0]
    again = rows_of(push(1, end=np.ones(n, np.uint8)))
    for i, x in enumerate((chunks[1][0], np.concatenate([chunks[0][1], chunks[1][1]]), chunks[1][2])):
        want = statement(x)
        assert same(again[i].reshape(-1), want[len(want) - len(again[i]):].reshape(-1)), i
    L.speechPlayer_stage_free(h)
    bp.close()
