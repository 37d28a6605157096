"""Track export of BASELINE configs[2] on one GPU (speechPlayer_batch_exportTracks, csrc/klatt_timeline.h) beside pcm_export, the
project's existing store-bound export, in ONE process: the batch set from shared lists, every case timed with events on torch's stream
after a warm-up, the cases alternating.
  (a) pcmTensor(float32, packed)                       (b) one column, cf1, hop 1, float32, packed: the same bytes written
  (c) the same for voicePitch (adds the per-list pass) (d) all 49 columns, hop 256, float32, packed
  (e) the per-list pass alone: voicePitch of workloads.all_different at one step per utterance (65 536 lists)
Expectation: (b) within a factor of two of (a) in bytes written per second -- the frames it reads are cache-resident and the arithmetic
per 16-byte store is a handful of f64 operations; anything slower means the kernel is not bound by its stores.
Usage: python tools/track_export_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
lists, list_of, seeds = workloads.shared("cfg2", n)
bp = eng.BatchPlayer(22050)
bp.setUtterancesShared(lists["frame_start"], lists["frames"], lists["min"], lists["fade"], list_of, lists["index"], lists["isnull"], seeds)
bp.synthesize()
dev = bp.device
stream = torch.cuda.current_stream(dev)
total = bp.totalSamples

cases = {
    "a_pcm_float32_packed": lambda: bp.pcmTensor(dtype=torch.float32, padded=False)[0],
    "b_cf1_hop1_float32_packed": lambda: bp.trackTensor("cf1", padded=False)[0],
    "c_voicePitch_hop1_float32_packed": lambda: bp.trackTensor("voicePitch", padded=False)[0],
    "d_49_columns_hop256_float32_packed": lambda: bp.trackTensor(list(range(49)), hop=256, padded=False)[0],
}
ms = {k: [] for k in cases}
written = {}
WARM, REPS = 2, 6
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
res = {"n_utt": n, "lists": int(len(lists["frame_start"]) - 1), "samples": int(total)}
for name in cases:
    med = float(np.median(ms[name]))
    res[name] = {"ms_median": round(med, 3), "ms_min": round(float(np.min(ms[name])), 3), "gb_written": round(written[name] / 1e9, 3),
                 "gb_written_per_s": round(written[name] / 1e9 / (med / 1e3), 1)}
res["b_over_a_in_bytes_written_per_second"] = round(res["b_cf1_hop1_float32_packed"]["gb_written_per_s"] / res["a_pcm_float32_packed"]["gb_written_per_s"], 3)
bp.close()

# (e) one list per utterance, one step per utterance: what the sequential voicePitch pass costs by itself
b = workloads.all_different(workloads.make("cfg2", n))
bp = eng.BatchPlayer(22050)
bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
e_ms = []
for r in range(WARM + REPS):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = bp.trackTensor("voicePitch", hop=1 << 30, padded=False)[0]
    e1.record(stream)
    e1.synchronize()
    assert out.numel() == n
    e_ms.append(e0.elapsed_time(e1))
res["e_per_list_pass_all_different"] = {"lists": n, "samples_walked": int(bp.totalSamples), "first_export_after_set_ms": round(e_ms[0], 3),
                                        "ms_median": round(float(np.median(e_ms[WARM:])), 3), "ms_min": round(float(np.min(e_ms[WARM:])), 3)}
bp.close()
print(json.dumps(res))
