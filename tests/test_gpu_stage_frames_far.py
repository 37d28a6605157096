"""The LPC and the pitch stage's 64-bit bookkeeping run where it matters (include/speechPlayer_batch.h, "Signal stages on the step grid";
csrc/klatt_stage_frames.h: phase + (M + j) hop, klatt_stage.h: stage_sample's n - (N - H)): a device-resident periodic int16 chunk of 2^27
samples is pushed again and again until (M + j) hop and N pass 2^31 and 2^32.  The hop is large, so a push emits a handful of steps, and
the table's period is odd, so no two steps near a bound see the same frame.  Every emitted step must equal the host statement on its frame
rebuilt from the table at the step's stream position -- signalLpc / signalPitch of that one frame with phase = before and hop = the frame's
length, which gives exactly one step --, bit for bit: a product or a position cut to 32 bits reads another part of the table, or +0.  Row 1
is reset midway and starts again from sample 0 beside row 0 deep in its stream; the last push ends both rows.  Needs a GPU."""
import numpy as np
import pytest

from tests.test_gpu_signal import record
from tests.test_gpu_stage import F32, bare, same  # noqa: F401  (bare is a fixture)

pytestmark = pytest.mark.gpu
C = 1 << 27                  # samples of the chunk, a row
P = 30011                    # the table's period (odd, prime): the chunk is the table again and again, cut at 2^27
HOP, PHASE = 26_843_551, 12_345      # five steps a push or so; hop odd
B31, B32 = 1 << 31, 1 << 32
PUSHES = 34                  # 34 x 2^27 > 2^32
RESET_AFTER = 16             # row 1 is reset behind the push that takes N past 2^31, and passes it again in the 17 pushes that follow


def table(i):
    rng = np.random.default_rng(40 + i)
    n = np.arange(P, dtype=np.float64)
    v = 0.5 * np.sin(2.0 * np.pi * n / 97.3 + i) + 0.2 * np.sin(2.0 * np.pi * n / 48.65) + 0.02 * rng.normal(0.0, 1.0, P)
    v[5000:9000] = 0.0       # a stretch of exact zeros longer than a frame
    return np.round(12000.0 * v).astype(np.int16)


def frame_at(tab, t0, length, N):
    """Samples t0 .. t0 + length - 1 of a stream of N samples that repeats a chunk of C samples, itself the table repeated: +0 outside."""
    t = t0 + np.arange(length, dtype=np.int64)
    x = tab[(t % C) % P].astype(F32) / F32(32767.0)
    x[(t < 0) | (t >= N)] = 0.0
    return x


@pytest.mark.parametrize("kind", ["lpc", "pitch"])
def test_steps_past_2_31_and_2_32_samples_of_a_stream(bare, kind):
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, speechPlayer as sp
    L = _native.load()
    n, dev = 2, "cuda:%d" % bare.device
    p = lambda a: None if a is None else a.ctypes.data
    if kind == "lpc":
        order, nWin, what = 16, 512, 31
        length, cols = nWin, sp.lpcColumns(what, order)[1]
        h = L.speechPlayer_batch_stageLpc(bare._h, n, order, nWin, HOP, PHASE, None, None, what)
        one = lambda x: eng.signalLpc(x, order, nWin, length, length // 2, fields=what)
        emitted = lambda N, ended: eng.lpcEmitted(N, nWin, HOP, PHASE, ended=ended)
    else:
        W, lagMin, lagMax, what = 160, 44, 300, 63
        length, cols = W + lagMax, sp.pitchColumns(what, lagMin, lagMax)[1]
        h = L.speechPlayer_batch_stagePitch(bare._h, n, 16000, W, lagMin, lagMax, 0.15, HOP, PHASE, what)
        one = lambda x: eng.signalPitch(x, 16000, nWin=W, hop=length, phase=length // 2, threshold=0.15, fields=what, lagMin=lagMin, lagMax=lagMax)
        emitted = lambda N, ended: eng.pitchEmitted(N, W, lagMax, HOP, PHASE, ended=ended)
    assert h, _native.last_error()
    assert one(np.zeros(length, F32)).shape == (1, cols)      # one frame, one step
    tabs = [table(i) for i in range(n)]
    chunk = torch.stack([torch.from_numpy(t).to(dev).repeat(C // P + 1)[:C] for t in tabs])
    assert chunk.shape == (n, C) and chunk.is_contiguous() and chunk.dtype == torch.int16
    extent = np.full(n, C, np.int64)
    rec = record(sp, chunk.data_ptr(), 0, n, C, extent)
    stride = C // HOP + 3
    out = torch.empty((n, stride, cols), dtype=torch.float64, device=dev)
    lengths, consumed, made = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    N, M = [0] * n, [0] * n
    crossed, voiced, checked, resets = set(), set(), 0, 0
    for k in range(PUSHES):
        last = k == PUSHES - 1
        end = np.full(n, last, np.uint8)
        out.fill_(-7.0)
        got = L.speechPlayer_stage_push(h, p(rec), p(end), out.data_ptr(), 0, None, stride, p(lengths), None)
        assert got == n * stride * cols, (kind, k, L.speechPlayer_lastError())
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        for i in range(n):
            count = emitted(N[i] + C, last) - emitted(N[i], False)
            assert lengths[i] == count and 4 <= count <= stride, (kind, k, i, lengths[i], count)
            assert not host[i, count:].view(np.uint64).any(), (kind, k, i, "padding")
            for e in range(count):
                j = M[i] + e
                t0 = PHASE + j * HOP - length // 2
                want = one(frame_at(tabs[i], t0, length, N[i] + C))
                assert same(host[i, e], want[0]), (kind, "push", k, "row", i, "step", j, "first sample", t0)
                checked += 1
                for bound in (B31, B32):
                    if j * HOP > bound and N[i] + C > bound:
                        crossed.add((i, bound, resets if i == 1 else 0))
                if kind == "pitch":
                    voiced.add(bool(want[0, 4]))
                else:
                    voiced.add(int(want[0, -1]) == order)
            N[i], M[i] = (0, 0) if last else (N[i] + C, M[i] + count)
        assert L.speechPlayer_stage_counts(h, p(consumed), p(made)) == 0 and list(consumed) == N and list(made) == M, (kind, k)
        if k == RESET_AFTER:
            assert N[1] > B31 >= N[1] - C
            assert L.speechPlayer_stage_reset(h, p(np.array([0, 1], np.uint8)), None) == 0
            N[1], M[1], resets = 0, 0, 1
    # row 0 went past 2^32, row 1 past 2^31 before its reset and again behind it
    assert {(0, B31, 0), (0, B32, 0), (1, B31, 0), (1, B31, 1)} <= crossed and (PUSHES - RESET_AFTER - 1) * C > B31
    assert voiced == {True, False} and checked > 2 * 4 * PUSHES      # full recursions and silent frames; voiced and unvoiced steps
    L.speechPlayer_stage_free(h)
