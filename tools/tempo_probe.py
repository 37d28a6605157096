"""The tempo exports (speechPlayer_batch_exportTempoPositions, exportTempo; csrc/klatt_tempo.h) on a cut of BASELINE configs[2] set from IPA
text, in ONE process, packed rows throughout.  The search (tempoPositionsTensor) and the render from its positions (tempoTensor with
positions=, float32 and int16) at window 512 and search 160 -- the defaults -- and at window 256 and search 80, every row at tempo 0.8 and
then the rows cycling 0.8, 1.25, beside resampledTensor(16000) of the same batch for scale.  Each case is timed with events on torch's
stream over REPS launches after WARM warm-ups; medians, with the spread (min, max).  Two rows of every case are checked against the
host's statement.  The operations counted are the binary64 multiply-adds the definition needs, sum (K - 1)(2 D + 1) N over the rows, set
against the device's vector binary64 peak (78.6 TFLOP/s: 39.3e12 multiply-adds a second); the render's bytes are what it must move --
two input samples read and one output written per output -- against 8 TB/s.  No target is set in advance.
Usage: python tools/tempo_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import speechPlayer as sp, workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
WARM, REPS = 2, 5
F64_FMA_PEAK, HBM_PEAK = 39.3e12, 8.0e12


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def median_of(bp, fn):
    stream = torch.cuda.current_stream(bp.device)
    ms = []
    for r in range(WARM + REPS):
        t, out = timed(stream, fn)
        del out
        if r >= WARM:
            ms.append(t)
    return float(np.median(ms)), {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
samples = int(bp.totalSamples)
lens = np.array([bp.utteranceSamples(u) for u in range(bp.nUtterances)], np.int64)
two = [bp.read(u) for u in range(2)]
res, res_ms = median_of(bp, lambda: bp.resampledTensor(16000, padded=False)[0])
print(json.dumps({"case": "resampled", "rate": 16000, "n_utt": int(bp.nUtterances), "samples": samples, "ms": res_ms}), flush=True)
for nWin, search in ((512, 160), (256, 80)):
    for name, tempo in (("0.8", np.full(len(lens), 0.8)), ("0.8, 1.25", np.where(np.arange(len(lens)) % 2, 1.25, 0.8))):
        outLens = sp._tempo_lengths(lens, tempo)
        frames = sp._tempo_frames(outLens, nWin)
        fma = int(np.sum(np.maximum(frames - 1, 0))) * (2 * search + 1) * nWin
        y, second, pos, counts = bp.tempoTensor(tempo[:2], nWin, search, utterances=np.arange(2), padded=False, returnPositions=True)
        want = [eng.pcmTempo(two[u], float(tempo[u]), nWin, search, returnPositions=True) for u in range(2)]
        ok = all(same(pos[int(counts[u]):int(counts[u + 1])].cpu().numpy(), want[u][1]) and same(y[int(second[u]):int(second[u + 1])].cpu().numpy(), want[u][0]) for u in range(2))
        del y, pos
        t, ms = median_of(bp, lambda: bp.tempoPositionsTensor(tempo, nWin, search, padded=False)[0])
        print(json.dumps({"case": "search", "nWin": nWin, "search": search, "tempo": name, "n_utt": int(bp.nUtterances), "samples": samples, "outputs": int(outLens.sum()),
                          "frames": int(frames.sum()), "statement_bits": ok, "ms": ms, "over_resampled": round(t / res, 2), "f64_fma": fma,
                          "f64_fma_per_second": float("%.4g" % (fma / (t * 1e-3))), "of_vector_f64_peak": round(fma / (t * 1e-3) / F64_FMA_PEAK, 4)}), flush=True)
        positions = bp.tempoPositionsTensor(tempo, nWin, search, padded=False)[0]
        for dtype, size in ((torch.float32, 4), (torch.int16, 2)):
            t, ms = median_of(bp, lambda: bp.tempoTensor(tempo, nWin, positions=positions, dtype=dtype, padded=False)[0])
            moved = int(outLens.sum()) * (2 * 2 + size) + int(frames.sum()) * 8
            print(json.dumps({"case": "render", "nWin": nWin, "tempo": name, "out": str(dtype).replace("torch.", ""), "outputs": int(outLens.sum()), "ms": ms,
                              "over_resampled": round(t / res, 2), "bytes": moved, "bytes_per_second": float("%.4g" % (moved / (t * 1e-3))),
                              "of_hbm_peak": round(moved / (t * 1e-3) / HBM_PEAK, 4)}), flush=True)
        del positions
bp.close()
