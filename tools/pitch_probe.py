"""The pitch export (speechPlayer_batch_exportPitch; csrc/klatt_pitch.h) on a cut of BASELINE configs[2] set from IPA text, in ONE process,
padded rows throughout, float32: lags 44 .. 368 (60 .. 500 Hz at 22050 Hz) at hop 256 over windows of 1024 and of 512 samples with the
fields f0 + aperiodicity, and the first again with the CMND curve (330 values a step), each beside spectrogramTensor(nFft=1024) on the
same grid: the same rows through the same masked reader.  Each pair is timed with events on torch's stream over REPS launches after WARM
warm-ups, the export and its comparison alternating; medians, with the spread (min, max) of each.  Two rows of every case are checked
against the host's statement.
The bound is binary64 issue, counted from the PAIRS the definition needs -- steps x W x lagMax --: one f64 fma (4 issue cycles a wave64
instruction) and one conversion (2) per pair and 64 lanes, on 1024 SIMDs at the clock the chip holds, the unit costs bench.py bills
(F64_ISSUE_CYCLES, OTHER_ISSUE_CYCLES, SIMDS, CLOCK_HZ_HELD_DEFAULT).  The float32 subtraction of a pair (2 more cycles), the lanes of
a pass of 256 lags that lie above lagMax and the scan are what the kernel spends beyond it.  No target is set in advance.
Usage: python tools/pitch_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
WARM, REPS = 2, 5
SIMDS, F64_ISSUE_CYCLES, OTHER_ISSUE_CYCLES, CLOCK_HZ_HELD = 1024, 4.0, 2.0, 2.07e9      # bench.py's


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def pair(bp, export, beside_name, beside):
    stream = torch.cuda.current_stream(bp.device)
    ms = {"export": [], beside_name: []}
    for r in range(WARM + REPS):
        for case, fn in (("export", export), (beside_name, beside)):      # alternating
            t, out = timed(stream, fn)
            del out
            if r >= WARM:
                ms[case].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return med, {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
samples = int(bp.totalSamples)
two = [bp.read(u) for u in range(2)]
lagMin, lagMax = eng.pitchLags(22050)
hop = 256
total = int(np.sum(-(-np.array([bp.utteranceSamples(u) for u in range(bp.nUtterances)], np.int64) // hop)))
for nWin, fields in ((1024, ("f0", "aperiodicity")), (512, ("f0", "aperiodicity")), (1024, ("f0", "aperiodicity", "cmnd"))):
    kw = dict(nWin=nWin, lagMin=lagMin, lagMax=lagMax, hop=hop, threshold=0.1, fields=fields)
    got, steps = bp.pitchTensor(utterances=np.arange(2), **kw)
    ok = all(same(got[u, :int(steps[u])].cpu().numpy(), eng.pcmPitch(two[u], 22050, **kw).astype(np.float32)) for u in range(2))
    del got
    med, ms = pair(bp, lambda: bp.pitchTensor(**kw)[0], "spectrogram", lambda: bp.spectrogramTensor(nFft=1024, hop=hop)[0])
    pairs = total * nWin * lagMax
    bound_ms = pairs / 64.0 * (F64_ISSUE_CYCLES + OTHER_ISSUE_CYCLES) / (SIMDS * CLOCK_HZ_HELD) * 1e3
    print(json.dumps({"case": "pitch", "nWin": nWin, "lagMin": lagMin, "lagMax": lagMax, "hop": hop, "fields": list(fields), "n_utt": int(bp.nUtterances), "samples": samples,
                      "steps": total, "statement_bits": ok, "ms": ms, "export_over_spectrogram": round(med["export"] / med["spectrogram"], 3),
                      "steps_per_second": float("%.4g" % (total / (med["export"] * 1e-3))), "pairs_per_second": float("%.4g" % (pairs / (med["export"] * 1e-3))),
                      "f64_issue_bound_ms": round(bound_ms, 3), "kernel_over_bound": round(med["export"] / bound_ms, 3)}), flush=True)
bp.close()
