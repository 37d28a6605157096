"""Tensor I/O of BASELINE configs[2] on one GPU: the set call from a device tensor (speechPlayer_batch_setUtterancesDevice) against the
set call from page-locked host frames, and pcm_export (speechPlayer_batch_exportPcm) -- packed int16, packed float32, and padded
float32 in 64-utterance minibatches of utterances sorted by length -- timed with events on torch's stream, with the bytes it moves.
Usage: python tools/tensor_io_probe.py [n_utt]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import _native, host_array, workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
b = workloads.make("cfg2", n)
bp = eng.BatchPlayer(22050)
dev = bp.device
args = (b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
pinned = host_array(b["frames"].shape, np.float64)
pinned[...] = b["frames"]
tensor = torch.from_numpy(b["frames"]).to("cuda:%d" % dev)
torch.cuda.synchronize()


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


res = {"n_utt": n, "frames": int(len(b["min"])), "frames_mb": round(b["frames"].nbytes / 2 ** 20, 1)}
# alternate the two forms so that neither always follows the other
host_ms, dev_ms = [], []
for _ in range(4):
    host_ms += timed(lambda: bp.setUtterances(b["frame_start"], pinned, *args), 1)
    plan_host = bp.kernelInfo()
    dev_ms += timed(lambda: bp.setUtterancesTensor(b["frame_start"], tensor, *args), 1)
    plan_dev = bp.kernelInfo()
res["set_pinned_host_ms"] = [round(x, 2) for x in host_ms]
res["set_device_tensor_ms"] = [round(x, 2) for x in dev_ms]
res["set_pinned_host_ms_median"] = round(float(np.median(host_ms[1:])), 2)
res["set_device_tensor_ms_median"] = round(float(np.median(dev_ms[1:])), 2)
res["same_plan"] = plan_host == plan_dev
del tensor

bp.synthesize()
total = bp.totalSamples
lens = np.array([bp.utteranceSamples(u) for u in range(n)], dtype=np.int64)
L = _native.load()
stream = torch.cuda.current_stream(dev)


def export_ms(calls, reps=10, warm=2):
    """median ms of `calls` (a list of (sel, n, out, fmt, stride)) between two events on the stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for r in range(warm + reps):
        e0.record(stream)
        for sel, cnt, out, fmt, stride in calls:
            got = L.speechPlayer_batch_exportPcm(bp._h, sel, cnt, out.data_ptr(), fmt, stride, stream.cuda_stream)
            assert got == out.numel(), (got, out.numel(), _native.last_error())
        e1.record(stream)
        e1.synchronize()
        if r >= warm:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


for name, dtype, fmt in (("packed_int16", torch.int16, 0), ("packed_float32", torch.float32, 1)):
    out = torch.empty(total, dtype=dtype, device="cuda:%d" % dev)
    med, best = export_ms([(None, n, out, fmt, 0)])
    moved = total * 2 + total * out.element_size()
    res[name] = {"samples": int(total), "ms_median": round(med, 3), "ms_min": round(best, 3), "gb": round(moved / 1e9, 2),
                 "gb_per_s": round(moved / 1e9 / (med / 1e3), 1)}
    del out

order = np.argsort(-lens, kind="stable")
calls, keep, written = [], [], 0
for a in range(0, n, 64):
    sel = np.ascontiguousarray(order[a:a + 64], dtype=np.int64)
    width = int(lens[sel].max())
    out = torch.empty((len(sel), width), dtype=torch.float32, device="cuda:%d" % dev)
    keep.append(sel)
    calls.append((sel.ctypes.data, len(sel), out, 1, width))
    written += out.numel()
torch.cuda.synchronize()
t = time.perf_counter()
med, best = export_ms(calls, reps=5, warm=1)
wall = (time.perf_counter() - t) * 1e3 / 6
moved = total * 2 + written * 4
res["padded_float32_minibatch64"] = {"calls": len(calls), "elements": int(written), "pad_fraction": round(1 - total / written, 4),
                                     "ms_median": round(med, 3), "ms_min": round(best, 3), "host_ms_per_pass": round(wall, 2),
                                     "gb": round(moved / 1e9, 2), "gb_per_s": round(moved / 1e9 / (med / 1e3), 1)}
res["synthesis_ms_median"] = round(float(np.median(bp.time(10))), 3)
print(json.dumps(res))
bp.close()
