"""The convolved export (speechPlayer_batch_exportConvolved, csrc/klatt_convolve.h) on a cut of BASELINE configs[2] set from IPA text, in
ONE process: float32, padded, tail = 0, one seeded response of 64, 1024 and 8192 taps, beside (a) pcmTensor(float32) of the same rows --
the traffic floor: 2 B read and 4 B written per sample -- and (b) the torch composition over the public API it replaces:
pcmTensor(float32) -> conv1d with the flipped response, or (from RFFT_FROM taps on, where conv1d is unreasonable) an rfft product.  Each is
timed with events on torch's stream over REPS launches after WARM warm-ups, the three alternating; medians.  Terms per second are
sum(Lout) * K / time, beside the packed-FMA VALU peak of the part (157.3 TFLOP/s counting a fused multiply-add as two).  No ratio is set
in advance.
Usage: python tools/convolve_probe.py [n_utt]"""
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
TAPS = [64, 1024, 8192]
RFFT_FROM = 4096
PEAK_TERMS = 157.3e12 / 2


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def response(K):
    rng = np.random.default_rng(K)
    return (0.5 * rng.uniform(-1, 1, K) * np.exp(-5.0 * np.arange(K) / K)).astype(np.float32)


def probe(bp, K):
    dev = "cuda:%d" % bp.device
    stream = torch.cuda.current_stream(bp.device)
    h = response(K)
    flipped = torch.from_numpy(h[::-1].copy()).to(dev)[None, None, :]
    hd = torch.from_numpy(h).to(dev)
    how = "rfft" if K >= RFFT_FROM else "conv1d"

    def export():
        return bp.convolvedTensor(h, tail=False)[0]

    def floor():
        return bp.pcmTensor()[0]

    def composition():
        pcm, _ = bp.pcmTensor()
        L = pcm.shape[1]
        if how == "conv1d":
            return torch.nn.functional.conv1d(torch.nn.functional.pad(pcm, (K - 1, 0))[:, None, :], flipped)[:, 0, :]
        size = 1 << int(np.ceil(np.log2(L + K - 1)))
        return torch.fft.irfft(torch.fft.rfft(pcm, size) * torch.fft.rfft(hd, size)[None, :], size)[:, :L]

    ms = {"export": [], "pcm_float32": [], "composition": []}
    for r in range(WARM + REPS):
        for case, fn in (("export", export), ("pcm_float32", floor), ("composition", composition)):      # alternating
            t, out = timed(stream, fn)
            del out
            if r >= WARM:
                ms[case].append(t)
    a, lens = bp.convolvedTensor(h, tail=False, utterances=np.arange(4))
    b = composition()[:4]
    worst = max(float((a[i, :int(lens[i])] - b[i, :int(lens[i])]).abs().max()) for i in range(4))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    samples = int(bp.totalSamples)
    terms = samples * K / (med["export"] * 1e-3)
    return {"taps": K, "n_utt": int(bp.nUtterances), "samples": samples, "composition": how,
            "ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
            "export_over_floor": round(med["export"] / med["pcm_float32"], 2), "composition_over_export": round(med["composition"] / med["export"], 2),
            "terms_per_second": float("%.4g" % terms), "of_the_packed_fma_peak": round(terms / PEAK_TERMS, 3),
            "largest_difference_from_the_composition": worst}


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
for K in TAPS:
    print(json.dumps(probe(bp, K)), flush=True)
bp.close()
