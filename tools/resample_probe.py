"""The resampled export (speechPlayer_batch_exportResampled, csrc/klatt_resample.h) on a cut of BASELINE configs[2] set from IPA text, in
ONE process, beside (a) pcmTensor(float32) of the same rows -- the HBM floor: the same reads and up / down times the writes -- and (b) the
torch composition over the public API it replaces: pcmTensor(float32) -> conv1d of stride `down` with `up` output channels over the same
table (channel j holds row (j down) mod up, shifted by floor(j down / up)) -> transpose.  float32, padded.  Each is timed with events
on torch's stream over REPS launches after WARM warm-ups, the three alternating; medians.  No ratio is set in advance.
Usage: python tools/resample_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
WARM, REPS = 2, 7
CASES = [(16000, dict(zeros=6, window="hann")), (24000, dict(zeros=6, window="hann")), (16000, dict(zeros=16, window="kaiser", beta=8.6))]


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def conv_weights(table, up, down, dev):
    """[up, 1, W]: channel j is row (j down) mod up of the table, placed floor(j down / up) samples in."""
    taps = table.shape[1]
    shift = np.arange(up) * down // up
    w = np.zeros((up, 1, taps + int(shift.max())), np.float32)
    for j in range(up):
        w[j, 0, shift[j]:shift[j] + taps] = table[(j * down) % up]
    return torch.from_numpy(w).to(dev)


def probe(bp, rate, kw):
    dev = "cuda:%d" % bp.device
    stream = torch.cuda.current_stream(bp.device)
    table, up, down = eng.resampleKernel(bp.sampleRate, rate, **kw)
    taps = table.shape[1]
    w = conv_weights(table, up, down, dev)

    def export():
        return bp.resampledTensor(rate, **kw)[0]

    def floor():
        return bp.pcmTensor()[0]

    def composition():
        pcm, _ = bp.pcmTensor()
        x = torch.nn.functional.pad(pcm, (taps // 2 - 1, w.shape[2]))[:, None, :]
        y = torch.nn.functional.conv1d(x, w, stride=down)          # [n, up, Q]
        return y.transpose(1, 2).reshape(y.shape[0], -1)

    ms = {"export": [], "pcm_float32": [], "composition": []}
    for r in range(WARM + REPS):
        for case, fn in (("export", export), ("pcm_float32", floor), ("composition", composition)):      # alternating
            t, out = timed(stream, fn)
            del out
            if r >= WARM:
                ms[case].append(t)
    a, lens = bp.resampledTensor(rate, utterances=np.arange(4), **kw)
    b = composition()[:4]
    worst = max(float((a[i, :int(lens[i])] - b[i, :int(lens[i])]).abs().max()) for i in range(4))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    samples = int(bp.totalSamples)
    return {"rate": rate, "filter": kw, "up": up, "down": down, "taps": taps, "n_utt": int(bp.nUtterances), "samples": samples,
            "ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
            "export_over_floor": round(med["export"] / med["pcm_float32"], 2), "composition_over_export": round(med["composition"] / med["export"], 2),
            "largest_difference_from_the_composition": worst}


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
for rate, kw in CASES:
    print(json.dumps(probe(bp, rate, kw)), flush=True)
bp.close()
