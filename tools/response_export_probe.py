"""The vocal-tract response export (speechPlayer_batch_exportResponse, csrc/klatt_response.h) on BASELINE configs[2] set from IPA text
(65 536 utterances over 512 distinct frame lists), at hop 256, float32, the two dB kinds, K = 80 and K = 513 bins -- beside pcmTensor
(pcm_export, float32) of the same synthesised batch as the store-rate yardstick, in ONE process.  Every case is timed with events on
torch's stream after a warm-up, the cases alternating; medians of REPS runs; GB/s = bytes written / median.
Usage: python tools/response_export_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
WARM, REPS = 2, 7
KINDS = ["cascade_db", "parallel_db"]

bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
stream = torch.cuda.current_stream(bp.device)
cases = {
    "response_K80_hop256": lambda: bp.responseTensor(80, KINDS, hop=256)[0],
    "response_K513_hop256": lambda: bp.responseTensor(513, KINDS, hop=256)[0],
    "response_K80_hop256_one_row_per_list": lambda: bp.responseTensor(80, KINDS, hop=256, utterances=np.arange(min(n, workloads.CFG2_PERIOD)))[0],
    "yardstick_pcmTensor_float32": lambda: bp.pcmTensor()[0],
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
res = {"n_utt": int(bp.nUtterances), "samples": int(bp.totalSamples), "kinds": KINDS}
for case in cases:
    med = float(np.median(ms[case]))
    res[case] = {"ms_median": round(med, 3), "ms_min": round(float(np.min(ms[case])), 3), "ms_max": round(float(np.max(ms[case])), 3),
                 "mb_written": round(written[case] / 1e6, 2), "gb_per_s": round(written[case] / 1e6 / med, 1),
                 "elements_per_us": round(written[case] / 4 / 1e3 / med, 1)}
print(json.dumps(res), flush=True)
bp.close()
