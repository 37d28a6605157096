"""The mix onto a signal (speechPlayer_batch_exportMixedOf, csrc/klatt_mix.h, klatt_sigpower.h) beside the mix on the pool, on the workload
of tools/mix_probe.py in ONE process: a cut of BASELINE configs[2] set from IPA text, float32 out, padded, (a) one looped bank clip at
10 dB per row, (b) the clip plus one interfering utterance (the next one, looped) at 0 dB.  Timed with events on torch's stream over
REPS launches after WARM warm-ups, the paths alternating; medians, min and max.
  pool     mixedTensor(terms): the yardstick.  Run this tool with --root pointing at a built checkout of the PARENT commit for the
           parent's figure and its run-to-run spread (a parent has no signal path: only `pool` is timed there).
  signal   mixedTensor(terms, signal=pcmTensor(float32)): the float32 signal is made once, before the timing.
--pool-only times the pool path alone, back to back, as a parent's run does: between two pool launches that alternate with the signal
path the 676 MB signal and its output pass through the caches, which a run of the pool alone does not see.
The expectation, set before any number: the signal path over the pool path is the ratio of their algorithmic bytes.  Per live sample
the pool reads 2 B for the powers and 2 B of speech, the float32 signal 4 B for the power pass and 4 B of speech; a clip term is 4 B in
both, an utterance term 2 B on the pool and 4 B on the signal; both write 4 B per padded element.
Usage: python tools/signal_mix_probe.py [n_utt] [--root DIR] [--pool-only]"""
import json
import os
import sys

import numpy as np
import torch

args = sys.argv[1:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in args:
    at = args.index("--root")
    root = os.path.abspath(args[at + 1])
    del args[at:at + 2]
POOL_ONLY = "--pool-only" in args
args = [a for a in args if a != "--pool-only"]
sys.path.insert(0, root)
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(args[0]) if args else 4096
WARM, REPS = 3, 9
CLIP = 220500      # ten seconds of noise
HAS_SIGNAL = hasattr(eng, "signalMix") and not POOL_ONLY


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def probe(bp, case, signal):
    stream = torch.cuda.current_stream(bp.device)
    M = eng.MixTerm
    N = int(bp.nUtterances)
    other = (np.arange(N) + 1) % N
    per = 1 if case == "a" else 2
    terms = np.zeros(N * per, eng.mixTermDtype)
    terms[0::per] = M(noise=0, snr=10.0).record()
    if case == "b":
        for u in range(N):
            terms[2 * u + 1] = M(utterance=int(other[u]), snr=0.0).record()
    start = np.arange(N + 1, dtype=np.int64) * per
    paths = [("pool", lambda: bp.mixedTensor((terms, start))[0])]
    if signal is not None:
        paths.append(("signal", lambda: bp.mixedTensor((terms, start), signal=signal)[0]))
    ms = {name: [] for name, _ in paths}
    for r in range(WARM + REPS):
        for name, fn in paths:      # alternating
            t, out = timed(stream, fn)
            del out
            if r >= WARM:
                ms[name].append(t)
    samples, elements = int(bp.totalSamples), N * int(bp._lengths().max())
    bytes_of = {"pool": samples * (2 + 2 + 4 + (2 if case == "b" else 0)) + elements * 4, "signal": samples * (4 + 4 + 4 + (4 if case == "b" else 0)) + elements * 4}
    out = {"case": case, "terms_per_row": per, "n_utt": N, "samples": samples, "padded_elements": elements,
           "ms": {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
           "algorithmic_bytes": {k: bytes_of[k] for k in ms}}
    if signal is not None:
        a, b = bp.mixedTensor((terms[:4 * per], start[:5]), utterances=np.arange(4)), bp.mixedTensor((terms[:4 * per], start[:5]), utterances=np.arange(4), signal=signal)
        out["expected_signal_over_pool"] = round(bytes_of["signal"] / bytes_of["pool"], 3)
        out["measured_signal_over_pool"] = round(float(np.median(ms["signal"]) / np.median(ms["pool"])), 3)
        out["largest_difference_between_the_paths"] = float((a[0] - b[0]).abs().max())      # (the float32 form of the PCM is not the PCM: the powers differ in the last bits)
    return out


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
bp.setNoiseBank([(0.1 * np.random.default_rng(1).standard_normal(CLIP)).astype(np.float32)])
signal = bp.pcmTensor(dtype=torch.float32) if HAS_SIGNAL else None
print(json.dumps({"package": root, "signal_path": HAS_SIGNAL}), flush=True)
for case in ("a", "b"):
    print(json.dumps(probe(bp, case, signal)), flush=True)
bp.close()
