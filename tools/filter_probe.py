"""The filtered export (speechPlayer_batch_exportFiltered, csrc/klatt_filter.h) on a cut of BASELINE configs[2] set from IPA text, in ONE
process: float32, padded, tail = 0, one seeded stable filter of 1, 4, 8 and 16 sections for every row, beside pcmTensor(float32) of the
same rows -- the traffic floor: 2 B read and 4 B written per sample.  Each is timed with events on torch's stream over REPS launches after
WARM warm-ups, the export and the floor alternating; medians.  Beside the times, the arithmetic estimate: one wavefront per SIMD issues
5 K dependent float32 operations per sample column of its 64 rows at about 4 cycles each, so a device of `cus` CUs at `clock` does
cus * 4 * 64 * clock / (20 K) samples per second at best.  No target is set in advance.
Usage: python tools/filter_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
WARM, REPS = 3, 10
SECTIONS = [1, 4, 8, 16]
CYCLES_PER_OP = 4.0


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def sections(K):
    """K seeded sections with poles at radius 0.3 .. 0.93, each passing white noise at its power."""
    rng = np.random.default_rng(K)
    z = np.exp(-1j * np.linspace(0, np.pi, 512))
    out = np.zeros((K, 5))
    for j in range(K):
        r, th = rng.uniform(0.3, 0.93), rng.uniform(0.05, 0.95) * np.pi
        b = np.array([1.0, rng.uniform(-1, 1), rng.uniform(-1, 1)])
        a1, a2 = -2 * r * np.cos(th), r * r
        gain = np.sqrt(np.mean(np.abs((b[0] + b[1] * z + b[2] * z * z) / (1 + a1 * z + a2 * z * z)) ** 2))
        out[j] = [*(b / gain), a1, a2]
    return out.astype(np.float32)


def probe(bp, K, cus, clock):
    stream = torch.cuda.current_stream(bp.device)
    sec = sections(K)
    ms = {"export": [], "pcm_float32": []}
    for r in range(WARM + REPS):
        for case, fn in (("export", lambda: bp.filteredTensor(sec)[0]), ("pcm_float32", lambda: bp.pcmTensor()[0])):      # alternating
            t, out = timed(stream, fn)
            del out
            if r >= WARM:
                ms[case].append(t)
    a, lens = bp.filteredTensor(sec, utterances=np.arange(2))
    pcm = [bp.read(u) for u in range(2)]
    exact = all(np.array_equal(a[u, :int(lens[u])].cpu().numpy().view(np.uint32), eng.pcmFilter(pcm[u], sec).view(np.uint32)) for u in range(2))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    samples = int(bp.totalSamples)
    lengths = np.sort(np.array([bp.utteranceSamples(u) for u in range(bp.nUtterances)]))[::-1]
    walked = int(sum(int(lengths[i]) * min(64, len(lengths) - i) for i in range(0, len(lengths), 64)))      # lane-samples the wavefronts walk: idle lanes included
    estimate = samples / (cus * 4 * 64 * clock / (5 * K * CYCLES_PER_OP)) * 1e3
    return {"sections": K, "n_utt": int(bp.nUtterances), "samples": samples, "statement_bits": exact,
            "ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
            "export_over_floor": round(med["export"] / med["pcm_float32"], 2), "arithmetic_estimate_ms": round(estimate, 3),
            "export_over_estimate": round(med["export"] / estimate, 2), "samples_per_second": float("%.4g" % (samples / (med["export"] * 1e-3))),
            "lane_samples_walked_over_samples": round(walked / samples, 3), "wavefronts": -(-int(bp.nUtterances) // 64), "simds": cus * 4}


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
props = torch.cuda.get_device_properties(bp.device)
cus, clock = props.multi_processor_count, getattr(props, "clock_rate", 2400000) * 1e3      # (kHz; 2.4 GHz where torch does not say)
for K in SECTIONS:
    print(json.dumps(probe(bp, K, cus, clock)), flush=True)
bp.close()
