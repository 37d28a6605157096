"""The glottal-source exports (speechPlayer_batch_exportSource / _exportEpochs, csrc/klatt_source.h) beside the existing serial walk,
trackTensor(["voicePitch"], hop=256) (klatt_timeline_pitch), and beside one synthesis launch, on two batches in ONE process:
  cfg2_ipa        BASELINE configs[2] set from IPA text: 65 536 utterances over 512 distinct frame lists
  all_different   workloads.all_different of configs[2]: 65 536 utterances, 65 536 distinct lists
Every case is timed with events on torch's stream after a warm-up, the cases alternating; medians of REPS runs.  The epoch counts are
taken once before the timed runs (the counting walk is timed by itself as the first epochCounts call after the set call).
Usage: python tools/source_export_probe.py [n_utt [source_lane_lists]]   (the second argument moves the threshold between the two walks:
2147483647 keeps every walk on the wavefront-per-list kernel)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
lane_lists = int(sys.argv[2]) if len(sys.argv) > 2 else None
WARM, REPS = 2, 11


def measure(bp, name):
    stream = torch.cuda.current_stream(bp.device)
    t0 = time.perf_counter()
    counts = bp.epochCounts()
    first_counts_ms = (time.perf_counter() - t0) * 1e3
    cases = {
        "source_f0_phase_hop256": lambda: bp.sourceTensor(["f0", "phase"], hop=256)[0],
        "epochs": lambda: bp.epochTensor()[0],
        "yardstick_voicePitch_hop256": lambda: bp.trackTensor(["voicePitch"], hop=256)[0],
    }
    ms = {k: [] for k in cases}
    written = {}
    for r in range(WARM + REPS):
        for case, fn in cases.items():      # alternating: no case always follows the same one
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
            written[case] = out.numel() * out.element_size()
            del out
            if r >= WARM:
                ms[case].append(e0.elapsed_time(e1))
    synth = []
    for r in range(WARM + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bp.synthesize()
        synth.append((time.perf_counter() - t0) * 1e3)
    res = {"batch": name, "source_lane_lists": lane_lists, "n_utt": int(bp.nUtterances), "samples": int(bp.totalSamples), "epoch_count": int(counts.sum()),
           "first_epochCounts_after_set_ms_host_clock": round(first_counts_ms, 3),
           "synthesize_ms_host_clock_median": round(float(np.median(synth[WARM:])), 3)}
    for case in cases:
        res[case] = {"ms_median": round(float(np.median(ms[case])), 3), "ms_min": round(float(np.min(ms[case])), 3),
                     "ms_max": round(float(np.max(ms[case])), 3), "mb_written": round(written[case] / 1e6, 2)}
    return res


bp = eng.BatchPlayer(22050)
if lane_lists is not None:
    bp.setOption("source_lane_lists", lane_lists)
bp.setIpa(**workloads.cfg2_spec(n))
print(json.dumps(measure(bp, "cfg2_ipa")), flush=True)
bp.close()

b = workloads.all_different(workloads.make("cfg2", n))
bp = eng.BatchPlayer(22050)
if lane_lists is not None:
    bp.setOption("source_lane_lists", lane_lists)
bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
print(json.dumps(measure(bp, "all_different")), flush=True)
bp.close()
