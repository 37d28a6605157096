"""Alignment export of BASELINE configs[2] on one GPU (speechPlayer_batch_exportAlignment / _exportUnits, csrc/klatt_align.h) beside the
project's two other store-bound exports, in ONE process: the batch set from IPA text (setIpa: 65 536 utterances over 512 labelled
lists), every case timed with events on torch's stream after a warm-up, the cases alternating.
  (a) pcmTensor(float32, packed)                         the yardstick
  (b) trackTensor("cf1", hop 1, float32, packed)         the same bytes written
  (c) alignmentTensor("phoneme", hop 1, int32, packed)   the same bytes written
  (d) unitTensor(hop 256, padded)                        the segment table
Expectation, stated before it was measured: (c) is bound by its stores and lands within a factor of two of (a) in bytes written per
second; anything slower wants a `rocprofv3 --kernel-trace --stats` summary beside the numbers (profiles/r9_alignment_export.txt).
Usage: python tools/alignment_probe.py [n_utt] [reps]"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARM = 3
bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
dev = bp.device
stream = torch.cuda.current_stream(dev)
total = bp.totalSamples

cases = {
    "a_pcm_float32_packed": lambda: bp.pcmTensor(dtype=torch.float32, padded=False)[0],
    "b_track_cf1_hop1_float32_packed": lambda: bp.trackTensor("cf1", padded=False)[0],
    "c_align_phoneme_hop1_int32_packed": lambda: bp.alignmentTensor("phoneme", dtype=torch.int32, padded=False)[0],
    "d_units_hop256_padded": lambda: bp.unitTensor(hop=256)[0],
}
ms = {k: [] for k in cases}
written = {}
for r in range(WARM + REPS):
    for name, fn in cases.items():      # alternating: no case always follows the same one
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        written[name] = out.numel() * out.element_size()
        del out
        if r >= WARM:
            ms[name].append(e0.elapsed_time(e1))
res = {"n_utt": n, "samples": int(total), "units": int(bp.unitCounts().sum()), "reps": REPS, "warm": WARM}
for name in cases:
    med = float(np.median(ms[name]))
    res[name] = {"ms_median": round(med, 3), "ms_min": round(float(np.min(ms[name])), 3), "ms_max": round(float(np.max(ms[name])), 3),
                 "gb_written": round(written[name] / 1e9, 3), "gb_written_per_s": round(written[name] / 1e9 / (med / 1e3), 1)}
a, b, c = (res[k]["gb_written_per_s"] for k in list(cases)[:3])
res["c_over_a_in_bytes_written_per_second"] = round(c / a, 3)
res["b_over_a_in_bytes_written_per_second"] = round(b / a, 3)
bp.close()


def clock_state():
    """What the machine says about its clocks (read only): the sclk / mclk lines of `rocm-smi --showclocks`, or why there are none."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return [" ".join(l.split()) for l in out.splitlines() if "sclk" in l or "mclk" in l][:16] or ["rocm-smi --showclocks printed no clock lines"]
    except Exception as e:      # noqa: BLE001
        return ["not read: %s" % e]


res["clock_state"] = clock_state()
res["device"] = torch.cuda.get_device_name(dev)
print(json.dumps(res))
