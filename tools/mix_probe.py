"""The mixed export (speechPlayer_batch_exportMixed, csrc/klatt_mix.h) on a cut of BASELINE configs[2] set from IPA text, in ONE process:
float32, padded, (a) one looped bank clip at 10 dB per row, (b) the clip plus one interfering utterance (the next one, looped) at 0 dB,
beside the torch composition over the public API that does the same work: pcmTensor(float32) -> per-row power -> gather with remainder ->
scaled add -> mask (the lengths and the sample numbers are on the device before the timing starts).  Each is timed with events on
torch's stream over REPS launches after WARM warm-ups, the two alternating; medians.
The algorithmic bytes of a launch are counted from the shapes: per live sample 2 B of speech for the powers and 2 B for the mixture, 4 B
per clip term and 2 B per utterance term, and 4 B written per padded element; they are set against the 6.3 TB/s a float4 copy reaches on
the part (8 TB/s on paper).  The clip is shared by every row and stays in cache: its 4 B per sample are counted as the algorithm's, not as
HBM traffic.  No ratio is set in advance.
Usage: python tools/mix_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
WARM, REPS = 3, 9
CLIP = 220500      # ten seconds of noise
HBM_MEASURED, HBM_SPEC = 6.3e12, 8.0e12


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def probe(bp, clip, case):
    dev = "cuda:%d" % bp.device
    stream = torch.cuda.current_stream(bp.device)
    M = eng.MixTerm
    N = int(bp.nUtterances)
    other = (np.arange(N) + 1) % N
    terms = np.zeros(N * (1 if case == "a" else 2), eng.mixTermDtype)
    per = 1 if case == "a" else 2
    terms[0::per] = M(noise=0, snr=10.0).record()
    if case == "b":
        for u in range(N):
            terms[2 * u + 1] = M(utterance=int(other[u]), snr=0.0).record()
    start = np.arange(N + 1, dtype=np.int64) * per
    clip_d = torch.from_numpy(clip).to(dev)
    other_d = torch.from_numpy(other).to(dev)
    clip_power = float(bp.noiseBankPowers()[0])
    # what a caller keeps between launches: the lengths on the device and the sample numbers
    lens_d = torch.from_numpy(bp._lengths().astype(np.int64)).to(dev)
    m = torch.arange(int(bp._lengths().max()), device=dev)

    def export():
        return bp.mixedTensor((terms, start))[0]

    def composition():
        pcm, _ = bp.pcmTensor()
        lens = lens_d
        power = (pcm * pcm).sum(1) / lens
        g = torch.sqrt(power / (clip_power * 10.0))
        y = pcm + g[:, None] * clip_d[m % CLIP][None, :]
        if case == "b":
            idx = m[None, :] % lens[other_d][:, None]
            v = torch.gather(pcm[other_d], 1, idx)
            y = y + torch.sqrt(power / power[other_d])[:, None] * v
        return torch.where(m[None, :] < lens[:, None], y, torch.zeros((), device=dev))

    ms = {"export": [], "composition": []}
    for r in range(WARM + REPS):
        for name, fn in (("export", export), ("composition", composition)):      # alternating
            t, out = timed(stream, fn)
            del out
            if r >= WARM:
                ms[name].append(t)
    a, lens = bp.mixedTensor((terms[:4 * per], start[:5]), utterances=np.arange(4))
    b = composition()[:4]
    worst = max(float((a[i, :int(lens[i])] - b[i, :int(lens[i])]).abs().max()) for i in range(4))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    samples = int(bp.totalSamples)
    elements = N * int(bp._lengths().max())
    algorithmic = samples * (2 + 2 + 4 + (2 if case == "b" else 0)) + elements * 4
    rate = algorithmic / (med["export"] * 1e-3)
    return {"case": case, "terms_per_row": per, "n_utt": N, "samples": samples, "padded_elements": elements,
            "ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
            "algorithmic_bytes": algorithmic, "bytes_per_second": float("%.4g" % rate),
            "of_6.3_TB/s_measured_copy": round(rate / HBM_MEASURED, 3), "of_8_TB/s_spec": round(rate / HBM_SPEC, 3),
            "composition_over_export": round(med["composition"] / med["export"], 2), "largest_difference_from_the_composition": worst}


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
clip = (0.1 * np.random.default_rng(1).standard_normal(CLIP)).astype(np.float32)
bp.setNoiseBank([clip])
for case in ("a", "b"):
    print(json.dumps(probe(bp, clip, case)), flush=True)
bp.close()
