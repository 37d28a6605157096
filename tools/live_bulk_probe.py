"""Bulk queueing and tensor PCM of live handles on one GPU (speechPlayer_queueFramesMany / _queueFramesManyDevice /
_synthesizeManyExport, through nvspeechplayer_amd.LiveGroup.queue / queueTensor / pullTensor).
  python tools/live_bulk_probe.py [handles] [frames]   host seconds to queue handles x frames frames three ways: the per-frame Python loop
                                                       (a Frame built field by field, one ctypes call per frame -- what bench.py's live
                                                       extra does in its set-up), LiveGroup.queue and LiveGroup.queueTensor; then an
                                                       in-step 8192-sample pull of the handles: call ms of pullDevice (PCM left in the
                                                       engine's pull buffer) and of pullTensor (exported into a caller's float32 tensor)
  python tools/live_bulk_probe.py --export-only        a queueTensor and pullTensor calls alone, for rocprofv3 --kernel-trace --stats
                                                       (live_place's and pcm_export's kernel time)
One JSON line per part.  Defaults: 8192 handles x 32 frames (about 8.5 frames per handle make an 8192-sample pull of speech)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import _native, workloads  # noqa: E402

PULL = 8192
L = _native.load()
b = workloads.make("cfg2", 8)          # the eight sampleIpa sentences as configs[2] speaks them


def sentence(s, count):
    """`count` frames of sentence s from its start, cycled: (frames [count, 47], min, fade, isNull)."""
    a, z = int(b["frame_start"][s]), int(b["frame_start"][s + 1])
    k = a + np.arange(count) % (z - a)
    return b["frames"][k], b["min"][k], b["fade"][k], b["isnull"][k]


def group_of(n):
    players = [eng.SpeechPlayer(22050, noiseSeed=k) for k in range(n)]
    return players, eng.LiveGroup(players)


def close(players):
    for p in players:
        p.close()


def queue_probe(n, per):
    parts = [sentence(k % 8, per) for k in range(n)]
    frames, m, f, nu = (np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(4))
    fs = np.arange(n + 1, dtype=np.int64) * per
    res = {"handles": n, "frames_per_handle": per, "frames": n * per}
    for rep in range(2):               # the first pass is a cold start (pinned buffers, code objects); the second is reported
        players, group = group_of(n)
        tensor = torch.from_numpy(frames).cuda(group.device)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k, p in enumerate(players):
            for r in range(k * per, (k + 1) * per):
                p.queueFrameSamples(None if nu[r] else eng.Frame.from_array(frames[r]), int(m[r]), int(f[r]))
        t_loop = time.perf_counter() - t
        t = time.perf_counter()
        group.queue(fs, frames, m, f, isNull=nu)
        t_queue = time.perf_counter() - t
        t = time.perf_counter()
        group.queueTensor(fs, tensor, m, f, isNull=nu)
        t_tensor = time.perf_counter() - t
        # every handle now holds the same frames three times over, all in its ring: a pull gives each a full 8192 samples
        produced = group.pullDevice(PULL)[2]
        res.update({"pass": rep, "per_frame_loop_s": round(t_loop, 4), "queue_s": round(t_queue, 4), "queueTensor_s": round(t_tensor, 4),
                    "per_frame_loop_us_per_frame": round(t_loop / (n * per) * 1e6, 3), "queue_us_per_frame": round(t_queue / (n * per) * 1e6, 4),
                    "queueTensor_us_per_frame": round(t_tensor / (n * per) * 1e6, 4), "queue_speedup_over_loop": round(t_loop / t_queue, 1),
                    "queueTensor_speedup_over_loop": round(t_loop / t_tensor, 1), "pull_after_all_full": bool((produced == PULL).all())})
        close(players)
        del group, tensor
    return res


def in_step(n):
    """n handles speaking one sentence from the same sample, 64 to a wavefront ("live_alone" 1: what in-step handles want)."""
    assert L.speechPlayer_setGlobalOption(b"live_alone", 1) == 0
    players, group = group_of(n)
    fr, m, f, nu = sentence(5, 200)
    group.queue(np.arange(n + 1, dtype=np.int64) * 200, np.tile(fr, (n, 1)), np.tile(m, n), np.tile(f, n), isNull=np.tile(nu, n))
    return players, group


def pull_probe(n, pulls=8):
    players, group = in_step(n)
    dev = group.device
    out = torch.empty((n, PULL), dtype=torch.float32, device="cuda:%d" % dev)
    group.pullDevice(64)
    group.pullTensor(64, out=out)
    torch.cuda.synchronize()
    dev_ms, ten_ms, ten_sync_ms, kms_dev, kms_ten, full = [], [], [], [], [], True
    for _ in range(pulls):             # alternated, so that neither always follows the other
        t = time.perf_counter()
        produced = group.pullDevice(PULL)[2]
        dev_ms.append((time.perf_counter() - t) * 1e3)
        kms_dev.append(float(L.speechPlayer_lastLiveKernelMs(dev)))
        full = full and bool((produced == PULL).all())
        torch.cuda.synchronize()
        t = time.perf_counter()
        produced = group.pullTensor(PULL, out=out)[1]
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        ten_ms.append((t1 - t) * 1e3)
        ten_sync_ms.append((time.perf_counter() - t) * 1e3)
        kms_ten.append(float(L.speechPlayer_lastLiveKernelMs(dev)))
        full = full and bool((produced == PULL).all())
    close(players)
    L.speechPlayer_setGlobalOption(b"live_alone", 1536)
    med = lambda v: round(float(np.median(v)), 3)
    return {"handles": n, "samples_per_pull": PULL, "pulls": pulls, "all_handles_full": full,
            "pullDevice_call_ms_median": med(dev_ms), "pullTensor_call_ms_median": med(ten_ms),
            "pullTensor_call_and_export_done_ms_median": med(ten_sync_ms),
            "live_kernel_ms_median_pullDevice": med(kms_dev), "live_kernel_ms_median_pullTensor": med(kms_ten),
            "export_bytes": n * PULL * (2 + 4)}


def export_only(n, pulls=6):
    players, group = in_step(n)
    fr, m, f, nu = sentence(3, 32)
    tensor = torch.from_numpy(np.tile(fr, (n, 1))).cuda(group.device)
    group.queueTensor(np.arange(n + 1, dtype=np.int64) * 32, tensor, np.tile(m, n), np.tile(f, n), isNull=np.tile(nu, n))
    out = torch.empty((n, PULL), dtype=torch.float32, device="cuda:%d" % group.device)
    for _ in range(pulls):
        group.pullTensor(PULL, out=out)
    torch.cuda.synchronize()
    close(players)
    L.speechPlayer_setGlobalOption(b"live_alone", 1536)
    return {"handles": n, "pullTensor_calls": pulls, "queueTensor_frames": n * 32}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 8192
    per = int(args[1]) if len(args) > 1 else 32
    if "--export-only" in sys.argv:
        print(json.dumps({"export_only": export_only(n)}), flush=True)
    else:
        print(json.dumps({"queue": queue_probe(n, per)}), flush=True)
        print(json.dumps({"pull": pull_probe(n)}), flush=True)
