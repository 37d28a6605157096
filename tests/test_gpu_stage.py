"""Signal stages on the device (include/speechPlayer_batch.h, "Signal stages": speechPlayer_batch_stageResample / stageFilter / stageCode,
speechPlayer_stage_push; BatchPlayer.resampleStage / filterStage / codeStage, SignalStage, SignalChain; csrc/klatt_stage.h): for every row,
the outputs of its pushes up to the one that ends it, concatenated, against the host's whole-signal statement -- signalResample,
signalFilter, signalCode -- on the concatenation of its chunks, bit for bit.  Chunks are int16 or float32, padded or packed, with poison
around and between the rows; outputs float32 or int16, padded or packed, between guards.  Every stream here is short: streams past 2^31
and 2^32 samples, and chunks and outputs past those elements, are tests/test_gpu_stage_far.py.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_filter_host import TELEPHONE, seven
from tests.test_gpu_signal import edge_rows, lay_out, poison, record

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
GUARD = 64
F32 = np.float32
RATES = [(22050, 16000), (22050, 48000), (22050, 44100), (22050, 8000), (22050, 11025), (48000, 4000), (16000, 16000)]


def same(got, want):
    """Equality of type, shape and every bit."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def x_of(row):
    """The reader's conversion: an int16 s is (float)s / 32767.0f, a float32 as it is."""
    return row.astype(F32) / F32(32767.0) if row.dtype == np.int16 else row.astype(F32)


@pytest.fixture(scope="module")
def bare():
    """A player that was never set: a stage needs no batch content."""
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    yield bp
    bp.close()


class Raw:
    """The C entry points on one stage, every output between guards: push(rows, end, ...) -> per row (decoded or None, codes or None)."""

    def __init__(self, bp, handle, n, code=False):
        from nvspeechplayer_amd import _native, speechPlayer as sp
        assert handle, _native.last_error()
        self.L, self.sp, self.bp, self.h, self.n, self.code = _native.load(), sp, bp, handle, n, code
        self.dev = "cuda:%d" % bp.device

    def plan(self, lens, end):
        lens, out = np.ascontiguousarray(lens, np.int64), np.zeros(self.n, np.int64)
        total = self.L.speechPlayer_stage_plan(self.h, lens.ctypes.data, None if end is None else end.ctypes.data, out.ctypes.data)
        assert total == out.sum(), self.L.speechPlayer_lastError()
        return out

    def push(self, rows, end, in_stride=0, in_shift=0, fmt=1, form="packed", shift=0, decoded=True, codes=False, stream=None):
        import torch
        npt = rows[0].dtype.type
        assert all(r.dtype == npt for r in rows) and len(rows) == self.n
        host, first, extent = lay_out(rows, npt, in_stride, poison, in_shift)
        data = torch.from_numpy(host.view(np.int32 if npt == F32 else np.int16)).to(self.dev)
        rec = record(self.sp, data.data_ptr() + first * data.element_size(), 1 if npt == F32 else 0, self.n, in_stride, extent)
        flags = None if end is None else np.ascontiguousarray(np.asarray(end, np.uint8))
        counts = self.plan([len(r) for r in rows], flags)
        stride = 0 if form == "packed" else int(counts.max()) + 3
        elements = int(counts.sum()) if stride == 0 else self.n * stride
        bufs = []
        for want, dtype in ((decoded, torch.float32 if fmt else torch.int16), (codes, torch.uint8)):
            if want:
                buf = torch.full((elements + 2 * GUARD + shift,), 0x55 if dtype == torch.uint8 else -7, dtype=dtype, device=self.dev)
                assert buf.data_ptr() % 16 == 0
                bufs.append(buf)
            else:
                bufs.append(None)
        ptr = lambda b: None if b is None or elements == 0 else b.data_ptr() + (GUARD + shift) * b.element_size()
        lengths = np.full(self.n, -1, np.int64)
        got = self.L.speechPlayer_stage_push(self.h, rec.ctypes.data, None if flags is None else flags.ctypes.data, ptr(bufs[0]), fmt, ptr(bufs[1]), stride,
                                             lengths.ctypes.data, stream)
        assert got == elements, (got, elements, self.L.speechPlayer_lastError())
        assert list(lengths) == list(counts)      # what the push emitted is what the plan said
        if stream is None:
            torch.cuda.synchronize()
        return lambda: self._rows(bufs, counts, stride, elements, shift, (data, rec, extent))

    def _rows(self, bufs, counts, stride, elements, shift, held):
        import torch
        torch.cuda.synchronize()
        out = []
        for buf in bufs:
            if buf is None:
                out.append([None] * self.n)
                continue
            got = buf.cpu().numpy()
            canary = got[0]
            assert np.all(got[:GUARD + shift] == canary) and np.all(got[GUARD + shift + elements:] == canary), "guards"
            got = got[GUARD + shift:GUARD + shift + elements]
            rows, at = [], 0
            for c in counts:
                span = int(c) if stride == 0 else stride
                rows.append(got[at:at + c].copy())
                assert not got[at + c:at + span].view(np.uint8).any(), "padding"
                at += span
            out.append(rows)
        return list(zip(*out))

    def free(self):
        self.L.speechPlayer_stage_free(self.h)


def schedule(n, pushes, pool, seed, ends=True):
    """Per push the rows' chunk lengths, drawn unsorted from `pool`, and their end flags: rows end at different pushes, go on after their
    end (a fresh row), and the last push ends them all."""
    rng = np.random.default_rng(seed)
    lens = [[int(pool[rng.integers(0, len(pool))]) for _ in range(n)] for _ in range(pushes)]
    end = np.zeros((pushes, n), np.uint8)
    for i in range(n):
        if ends:
            end[2 + (i + seed) % (pushes - 3), i] = 1
    end[-1, :] = 1
    return lens, end


FORMS = [dict(in_stride=0, in_shift=1, fmt=1, form="packed", shift=1), dict(in_stride=-1, in_shift=2, fmt=0, form="padded", shift=3),
         dict(in_stride=0, in_shift=0, fmt=0, form="packed", shift=3), dict(in_stride=-1, in_shift=3, fmt=1, form="padded", shift=0)]


def run_stream(raw, lens, end, seed, **kw):
    """Push after push, formats and layouts alternating: -> per row its segments [(chunks as float32 concatenated, the push's formats, the
    outputs per push)], a segment closing at the row's end."""
    n = raw.n
    segments = [[dict(x=[], out=[])] for _ in range(n)]
    for k, (ls, e) in enumerate(zip(lens, end)):
        npt = (np.int16, F32)[(k + seed) % 2]
        rows = edge_rows(ls, npt, 1000 * seed + k)
        form = dict(FORMS[(k + seed) % len(FORMS)])
        if form["in_stride"] < 0:
            form["in_stride"] = max(ls) + 5
        form.update(kw)
        got = raw.push(rows, e, **form)()
        for i in range(n):
            seg = segments[i][-1]
            seg["x"].append(x_of(rows[i]))
            seg["out"].append((form["fmt"], got[i]))
            if e[i]:
                segments[i].append(dict(x=[], out=[]))
    assert all(not s[-1]["x"] for s in segments)      # the last push ended every row
    return [s[:-1] for s in segments]


def check_segments(segments, statement, tag):
    """Every segment's outputs, each push in its own format, are the statement's values on the segment's input, cut at the pushes' counts."""
    for i, row in enumerate(segments):
        for j, seg in enumerate(row):
            x = np.concatenate(seg["x"]) if seg["x"] else np.zeros(0, F32)
            want = {fmt: statement(i, x, fmt) for fmt in {f for f, _ in seg["out"]}}
            at = 0
            for k, (fmt, got) in enumerate(seg["out"]):
                for part, (g, w) in enumerate(zip(got, want[fmt])):
                    if g is not None:
                        assert same(g, w[at:at + len(g)]), tag + (i, j, k, part, len(g))
                at += len([g for g in got if g is not None][0])
            assert at == len(want[seg["out"][0][0]][0]), tag + (i, j, "length")


# ---- 1. the resampler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("rates", RATES)
def test_resample_pushes_concatenate_to_the_statement(bare, rates, n):
    """Seven rates -- 48000 -> 4000 has down / up = 12, so a tile splits into spans; 16000 -> 16000 passes through -- on 1, 3 and 65 rows,
    every row its own seeded sequence of seven chunks from {0, 1, Z - 1, Z, 2 Z - 1, 2 Z, 137, 3000}, rows ending at different pushes and
    going on afterwards as fresh rows; every push's lengths are speechPlayer_stage_plan's and the difference of resampleEmitted."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    src, dst = rates
    Z = eng.resampleKernel(src, dst)[0].shape[1] // 2
    raw = Raw(bare, L.speechPlayer_batch_stageResample(bare._h, n, src, dst, 6, 0.99, 0, 0.0), n)
    lens, end = schedule(n, 7, [0, 1, Z - 1, Z, 2 * Z - 1, 2 * Z, 137, 3000], 7 * n + src % 11 + dst % 13)
    # the counts, from the host's closed form alone
    N, counts = np.zeros(n, np.int64), []
    for ls, e in zip(lens, end):
        counts.append([eng.resampleEmitted(int(N[i]) + ls[i], src, dst, ended=bool(e[i])) - eng.resampleEmitted(int(N[i]), src, dst) for i in range(n)])
        N = np.where(e, 0, N + np.array(ls))
    segments = run_stream(raw, lens, end, n + src % 7)
    k = 0
    for i in range(n):
        got = [len(g[0]) for seg in segments[i] for _, g in seg["out"]]
        assert got == [c[i] for c in counts], (rates, n, i)
        k += sum(got)
    assert k > 0
    consumed, emitted = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    assert L.speechPlayer_stage_counts(raw.h, consumed.ctypes.data, emitted.ctypes.data) == 0 and not consumed.any() and not emitted.any()
    check_segments(segments, lambda i, x, fmt: (eng.signalResample(x, src, dst, dtype=F32 if fmt else np.int16),), (rates, n))
    raw.free()


# ---- 2. the filter ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_filter_pushes_concatenate_to_the_statement(bare, n):
    """The seven filters cycled over the rows; three pushes of chunk lengths drawn unsorted from {0, 1, T - 1, T, T + 1, 2 T + 3} -- within
    a wavefront short rows beside long ones, where a state stepped past a row's own end shows --, then the end, with tail T + 3."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    T = sp.FILTER_TILE
    filters = seven()
    flat, start = np.concatenate(filters), np.concatenate([[0], np.cumsum([len(f) for f in filters])]).astype(np.int64)
    of = ((np.arange(n) * 3) % 7).astype(np.int64)
    raw = Raw(bare, L.speechPlayer_batch_stageFilter(bare._h, n, flat.ctypes.data, start.ctypes.data, 7, of.ctypes.data, T + 3), n)
    lens, end = schedule(n, 4, [0, 1, T - 1, T, T + 1, 2 * T + 3], 40 + n, ends=False)
    assert n < 6 or any(sorted(ls) != ls and sorted(ls, reverse=True) != ls for ls in lens)
    segments = run_stream(raw, lens, end, n)
    check_segments(segments, lambda i, x, fmt: (eng.signalFilter(x, filters[of[i]], tail=T + 3, dtype=F32 if fmt else np.int16),), ("filter", n))
    # ... and the rows are fresh: the same stream again, now with rows that end midway
    lens, end = schedule(n, 5, [0, 1, T - 1, T, T + 1, 2 * T + 3], 50 + n)
    segments = run_stream(raw, lens, end, n + 1)
    check_segments(segments, lambda i, x, fmt: (eng.signalFilter(x, filters[of[i]], tail=T + 3, dtype=F32 if fmt else np.int16),), ("filter again", n))
    raw.free()


# ---- 3. the codecs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("codec", ["adpcm", "ulaw", "alaw"])
def test_code_pushes_concatenate_to_the_statement(bare, codec, n):
    """The filter's layout through the three codecs: the codes and the decoded samples, alone and together."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    T = sp.FILTER_TILE
    raw = Raw(bare, L.speechPlayer_batch_stageCode(bare._h, n, sp.CODECS.index(codec)), n, code=True)

    def statement(i, x, fmt):
        return eng.signalCode(x, codec, codes=True, decoded=True, dtype=F32 if fmt else np.int16)

    for k, outputs in enumerate((dict(decoded=True, codes=True), dict(decoded=False, codes=True), dict(decoded=True, codes=False))):
        lens, end = schedule(n, 5, [0, 1, T - 1, T, T + 1, 2 * T + 3, 1100], 60 + n + k)
        check_segments(run_stream(raw, lens, end, n + k, **outputs), statement, (codec, n, k))
    raw.free()


# ---- 4. the chain on live handles ------------------------------------------------------------------------------------------------------------------
def test_the_chain_on_live_handles():
    """Five live handles speaking different utterances, pulled 137 samples at a time, then 1000 at a time, through
    SignalChain([filterStage(TELEPHONE), resampleStage(22050 -> 8000), codeStage("adpcm")]), end=True on the last push: per handle the codes
    and the decoded samples are signalCode(signalResample(signalFilter(pcm))) of the handle's whole PCM, float32 between the stages."""
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
    chain = eng.SignalChain([bp.filterStage(5, TELEPHONE), bp.resampleStage(5, 22050, 8000), bp.codeStage(5, "adpcm")])
    pcm, decoded, codes = [[] for _ in range(5)], [[] for _ in range(5)], [[] for _ in range(5)]
    pulls = 0
    while True:
        out, produced = group.pullTensor(137 if pulls < 12 else 1000, dtype=torch.int16)
        produced = produced.copy()
        last = not produced.any()
        d, c, lengths = chain.push((out, produced), end=last, codes=True)
        lengths = lengths.numpy()
        assert d.dtype == torch.int16 and c.dtype == torch.uint8 and d.shape == c.shape
        rows, d, c = out.cpu().numpy(), d.cpu().numpy(), c.cpu().numpy()
        for i in range(5):
            pcm[i].append(rows[i, :produced[i]])
            decoded[i].append(d[i, :lengths[i]])
            codes[i].append(c[i, :lengths[i]])
            assert not d[i, lengths[i]:].any() and not c[i, lengths[i]:].any()
        pulls += 1
        if last:
            break
        assert pulls < 2000
    lens = {len(np.concatenate(p)) for p in pcm}
    assert len(lens) > 1 and min(lens) > 2000 and pulls > 14      # different utterances, both pull sizes
    for i in range(5):
        whole = np.concatenate(pcm[i])
        d, c = eng.signalCode(eng.signalResample(eng.signalFilter(whole, TELEPHONE), 22050, 8000), "adpcm", codes=True)
        assert same(np.concatenate(decoded[i]), d) and same(np.concatenate(codes[i]), c), i
    assert not chain.stages[1].consumed.any() and not chain.stages[2].emitted.any()
    for s in chain.stages:
        s.close()
    bp.close()
    for p in players:
        p.close()


# ---- 5. ordering ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["resample", "filter", "code"])
def test_pushes_on_two_streams_follow_one_another(bare, kind):
    """Pushes of one stage issued alternately on two torch streams, the first of them behind a busy kernel: they still concatenate to the
    statement, by the stage's events alone."""
    import torch
    import nvspeechplayer_amd as eng
    n = 3
    stage = dict(resample=lambda: bare.resampleStage(n, 22050, 16000), filter=lambda: bare.filterStage(n, TELEPHONE), code=lambda: bare.codeStage(n, "adpcm"))[kind]()
    statement = dict(resample=lambda x: eng.signalResample(x, 22050, 16000), filter=lambda x: eng.signalFilter(x, TELEPHONE),
                     code=lambda x: eng.signalCode(x, "adpcm"))[kind]
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
@pytest.mark.parametrize("kind", ["resample", "filter", "code"])
def test_refusals_write_nothing_and_leave_the_state_as_it_was(kind):
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    bp = eng.BatchPlayer(22050)
    dev = "cuda:%d" % bp.device
    n, c = 3, 500
    sec = np.ascontiguousarray((TELEPHONE[:, [0, 1, 2, 4, 5]] / TELEPHONE[:, 3:4]).astype(F32))
    start = np.array([0, 4], np.int64)
    p = lambda a: None if a is None else a.ctypes.data

    def make(rows=n, batch=0, **kw):
        b = bp._h if batch == 0 else batch
        if kind == "resample":
            a = dict(src=22050, dst=8000, zeros=6, rolloff=0.99, window=0, beta=0.0)
            a.update(kw)
            return L.speechPlayer_batch_stageResample(b, rows, a["src"], a["dst"], a["zeros"], a["rolloff"], a["window"], a["beta"])
        if kind == "filter":
            a = dict(sections=sec, starts=start, nFilters=1, filterOf=None, tail=3)
            a.update(kw)
            return L.speechPlayer_batch_stageFilter(b, rows, p(a["sections"]), p(a["starts"]), a["nFilters"], p(a["filterOf"]), a["tail"])
        return L.speechPlayer_batch_stageCode(b, rows, kw.get("codec", 2))

    def not_made(name, **kw):
        assert make(**kw) is None and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name

    not_made("no batch", batch=None)
    for rows in (0, -1, (1 << 20) + 1):
        not_made("nRows", rows=rows)
    unstable = sec.copy()
    unstable[2, 4] = 1.0
    for name, kw in dict(resample=dict(zeros=dict(zeros=0), rate=dict(dst=0), rolloff=dict(rolloff=0.0), window=dict(window=2), beta=dict(window=1, beta=-1.0),
                                       up=dict(dst=22051), taps=dict(dst=100, zeros=200)),
                         filter=dict(tail=dict(tail=-1), no_filters=dict(nFilters=0), no_sections=dict(sections=None), start=dict(starts=np.array([1, 4], np.int64)),
                                     unstable=dict(sections=unstable), filterOf=dict(filterOf=np.array([0, 1, 0], np.int64)),
                                     filterOf_missing=dict(sections=np.tile(sec, (2, 1)), starts=np.array([0, 4, 8], np.int64), nFilters=2)),
                         code=dict(codec_3=dict(codec=3), codec_negative=dict(codec=-1)))[kind].items():
        not_made(name, **kw)

    h = make()
    assert h, L.speechPlayer_lastError()
    rng = np.random.default_rng(9)
    chunks = [rng.uniform(-1.0, 1.0, (n, c)).astype(F32) for _ in range(3)]
    data = [torch.from_numpy(x).to(dev) for x in chunks]
    extent = np.full(n, c, np.int64)
    width = 2 * c
    out = torch.full((n * width + 8,), -7.0, dtype=torch.float32, device=dev)
    cod = torch.full((n * width + 8,), 0x55, dtype=torch.uint8, device=dev)
    sentinel, sentinel_codes = out.clone(), cod.clone()
    host = np.zeros(n * width, F32)
    lengths = np.zeros(n, np.int64)
    is_code = kind == "code"

    def push(k=0, handle=0, signal=0, end=None, ptr=0, fmt=1, codes=0, stride=width, **sig):
        s = dict(data=data[k].data_ptr(), format=1, nRows=n, rowStride=c, extent=extent)
        s.update(sig)
        rec = record(sp, s["data"], s["format"], s["nRows"], s["rowStride"], s["extent"])
        return L.speechPlayer_stage_push(h if handle == 0 else handle, rec.ctypes.data if signal == 0 else signal, p(end), out.data_ptr() if ptr == 0 else ptr, fmt,
                                         (cod.data_ptr() if is_code else None) if codes == 0 else codes, stride, lengths.ctypes.data, None)

    def refused(name, **kw):
        assert push(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"stage_push" in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        assert torch.equal(out, sentinel) and torch.equal(cod, sentinel_codes), name

    def rows_of(elements):
        torch.cuda.synchronize()
        counts = lengths.copy()
        got = out[:n * width].view(n, width).cpu().numpy()
        gc = cod[:n * width].view(n, width).cpu().numpy()
        assert elements == n * width and not got[:, counts.max():].any()
        out.copy_(sentinel)
        cod.copy_(sentinel_codes)
        return [got[i, :counts[i]].copy() for i in range(n)], [gc[i, :counts[i]].copy() for i in range(n)]

    first = rows_of(push(0))
    other = eng.BatchPlayer(22050)
    gone = make(batch=other._h)
    assert gone
    other.close()      # a stage goes with its batch
    freed = make()
    L.speechPlayer_stage_free(freed)
    big = torch.cat([data[1].reshape(-1), torch.zeros(n * width, dtype=torch.float32, device=dev)])      # the chunk, and room behind it for an output
    cases = dict(
        no_stage=dict(handle=None), freed=dict(handle=freed), freed_with_its_batch=dict(handle=gone), no_signal=dict(signal=None),
        rows_fewer=dict(nRows=n - 1), rows_more=dict(nRows=n + 1, extent=np.full(n + 1, c, np.int64)), signal_format=dict(format=2), signal_stride=dict(rowStride=-1),
        no_extent=dict(extent=None), extent_beyond=dict(extent=np.array([c, c + 1, c], np.int64)), extent_negative=dict(extent=np.array([c, -1, c], np.int64)),
        no_data=dict(data=0), host_data=dict(data=host.ctypes.data), misaligned_data=dict(data=data[1].data_ptr() + 2),
        past_2_44=dict(rowStride=1 << 44, extent=np.array([c, 1 << 44, c], np.int64)),
        format_2=dict(fmt=2), stride_negative=dict(stride=-1), stride_short=dict(stride=1), too_large=dict(stride=1 << 40),
        no_buffer=dict(ptr=None, codes=None), host_memory=dict(ptr=host.ctypes.data), misaligned=dict(ptr=out.data_ptr() + 2), misaligned_int16=dict(ptr=out.data_ptr() + 1, fmt=0),
        output_on_the_chunk=dict(ptr=data[1].data_ptr(), stride=c if kind != "resample" else 400),
        output_into_the_chunk=dict(data=big.data_ptr(), ptr=big.data_ptr() + 4 * (n * c - 8)))
    if is_code:
        cases.update(codes_on_the_chunk=dict(codes=data[1].data_ptr(), stride=c), codes_on_the_decoded=dict(codes=out.data_ptr() + 16), host_codes=dict(codes=host.ctypes.data))
    else:
        cases.update(codes_on_another_kind=dict(codes=cod.data_ptr()))
    for name, kw in cases.items():
        kw.setdefault("k", 1)
        refused(name, **kw)
    assert torch.equal(big[:n * c], data[1].reshape(-1)) and not big[n * c:].any()
    consumed = np.zeros(n, np.int64)
    assert L.speechPlayer_stage_counts(h, consumed.ctypes.data, None) == 0 and list(consumed) == [c] * n
    # nothing moved: the stream goes on, ends, and equals the statement
    second = rows_of(push(1))
    third = rows_of(push(2, end=np.ones(n, np.uint8)))
    for i in range(n):
        x = np.concatenate([ch[i] for ch in chunks])
        got = np.concatenate([first[0][i], second[0][i], third[0][i]])
        if kind == "resample":
            assert same(got, eng.signalResample(x, 22050, 8000)), i
        elif kind == "filter":
            assert same(got, eng.signalFilter(x, TELEPHONE, tail=3)), i
        else:
            d, cc = eng.signalCode(x, "adpcm", codes=True, dtype=F32)
            assert same(got, d) and same(np.concatenate([first[1][i], second[1][i], third[1][i]]), cc), i
    assert torch.equal(out[n * width:], sentinel[n * width:])
    # reset makes the chosen rows fresh, behind the last push
    assert push(0) == n * width
    rows_of(n * width)
    assert L.speechPlayer_stage_reset(h, np.array([1, 0, 1], np.uint8).ctypes.data, None) == 0
    assert L.speechPlayer_stage_counts(h, consumed.ctypes.data, None) == 0 and list(consumed) == [0, c, 0]
    again = rows_of(push(1, end=np.ones(n, np.uint8)))
    for i, x in enumerate((chunks[1][0], np.concatenate([chunks[0][1], chunks[1][1]]), chunks[1][2])):
        want = (eng.signalResample(x, 22050, 8000) if kind == "resample" else eng.signalFilter(x, TELEPHONE, tail=3) if kind == "filter"
                else eng.signalCode(x, "adpcm", dtype=F32))
        assert same(again[0][i], want[len(want) - len(again[0][i]):]), i
    L.speechPlayer_stage_free(h)
    bp.close()


# ---- 7. the stage kernel against the whole-row kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "padded"])
@pytest.mark.parametrize("kind", ["resample 22050 -> 16000", "resample 48000 -> 4000", "filter", "adpcm"])
def test_one_push_that_ends_every_row_is_the_whole_row_export(bare, kind, form):
    """The stage kernels against the whole-row kernels on the device -- two entry points on one body for the resampler (resample_rows of
    csrc/klatt_resample.h), siblings for the filter and for ADPCM (csrc/klatt_stage.h beside klatt_filter.h and klatt_codec.h):
    on 65 float32 rows of lengths drawn unsorted from {0, 1, T - 1, T, T + 1, 2 T + 3} (T the kind's tile), a single push that ends every
    row of a fresh stage writes, between its guards, exactly the bytes exportResampledOf / exportFilteredOf (the same tail) / exportCodedOf
    write for the same signal -- rows, padding and guards, float32 and int16, the codes as well."""
    import torch
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    n, dev = 65, "cuda:%d" % bare.device
    p = lambda a: None if a is None else a.ctypes.data
    T = sp.RESAMPLE_TILE if kind.startswith("resample") else sp.FILTER_TILE
    pool = [0, 1, T - 1, T, T + 1, 2 * T + 3]
    rng = np.random.default_rng(len(kind) + len(form))
    lens = [pool[rng.integers(0, len(pool))] for _ in range(n)]
    assert set(lens) == set(pool) and sorted(lens) != lens and sorted(lens, reverse=True) != lens
    rows = edge_rows(lens, F32, 70 + len(kind))
    host, first, extent = lay_out(rows, F32, 0 if form == "packed" else max(lens) + 5, poison, 1)
    data = torch.from_numpy(host.view(np.int32)).to(dev)
    rec = record(sp, data.data_ptr() + 4 * first, 1, n, 0 if form == "packed" else max(lens) + 5, extent)
    filters = seven()
    flat, start = np.concatenate(filters), np.concatenate([[0], np.cumsum([len(f) for f in filters])]).astype(np.int64)
    of = ((np.arange(n) * 3) % 7).astype(np.int64)
    if kind.startswith("resample"):
        src, dst = (int(w) for w in kind.split()[1::2])
        h = L.speechPlayer_batch_stageResample(bare._h, n, src, dst, 6, 0.99, 0, 0.0)
        export = lambda d, fmt, c, stride: L.speechPlayer_batch_exportResampledOf(bare._h, p(rec), None, 0, src, dst, 6, 0.99, 0, 0.0, d, fmt, stride, None)
    elif kind == "filter":
        h = L.speechPlayer_batch_stageFilter(bare._h, n, p(flat), p(start), 7, p(of), T + 3)
        export = lambda d, fmt, c, stride: L.speechPlayer_batch_exportFilteredOf(bare._h, p(rec), None, 0, p(flat), p(start), 7, p(of), T + 3, d, fmt, stride, None)
    else:
        h = L.speechPlayer_batch_stageCode(bare._h, n, sp.CODECS.index("adpcm"))
        export = lambda d, fmt, c, stride: L.speechPlayer_batch_exportCodedOf(bare._h, p(rec), None, 0, sp.CODECS.index("adpcm"), d, fmt, c, stride, None)
    assert h, _native.last_error()
    end, counts, lengths = np.ones(n, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
    shift = 3
    for fmt in (1, 0):      # (the push ends every row, so the stage is fresh again for the second format)
        assert L.speechPlayer_stage_plan(h, p(np.array(lens, np.int64)), p(end), p(counts)) == counts.sum() > 0
        stride = 0 if form == "packed" else int(counts.max()) + 3
        elements = int(counts.sum()) if stride == 0 else n * stride
        bufs = {}
        for who in ("push", "export"):
            d = torch.full((elements + 2 * GUARD + shift,), -7, dtype=torch.float32 if fmt else torch.int16, device=dev)
            c = torch.full((elements + 2 * GUARD + shift,), 0x55, dtype=torch.uint8, device=dev) if kind == "adpcm" else None
            bufs[who] = (d, c)
            dptr, cptr = d.data_ptr() + (GUARD + shift) * d.element_size(), None if c is None else c.data_ptr() + GUARD + shift
            got = L.speechPlayer_stage_push(h, p(rec), p(end), dptr, fmt, cptr, stride, p(lengths), None) if who == "push" else export(dptr, fmt, cptr, stride)
            assert got == elements, (kind, form, fmt, who, got, elements, _native.last_error())
        assert list(lengths) == list(counts)
        torch.cuda.synchronize()
        for a, b in zip(bufs["push"], bufs["export"]):
            if a is not None:
                a, b = a.cpu().numpy(), b.cpu().numpy()
                assert a.tobytes() == b.tobytes(), (kind, form, fmt, a.dtype)
                assert np.all(a[:GUARD + shift] == a[0]) and np.all(a[GUARD + shift + elements:] == a[0]) and a[0] in (-7, 0x55), (kind, form, fmt, "guards")
                assert np.any(a[GUARD + shift:GUARD + shift + elements] != a[0])
    consumed = np.full(n, -1, np.int64)
    assert L.speechPlayer_stage_counts(h, p(consumed), None) == 0 and not consumed.any()
    L.speechPlayer_stage_free(h)
