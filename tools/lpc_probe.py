"""The linear-prediction exports (speechPlayer_batch_exportLpc, exportLpcResidual; csrc/klatt_lpc.h) on a cut of BASELINE configs[2] set
from IPA text, in ONE process, padded rows throughout.  The analysis (lpc + error, float32) at three requests -- order 16 over 512 samples
at hop 256, order 32 over 1024 at hop 256, order 10 over 400 at hop 160 -- beside spectrogramTensor of the nearest power-of-two frame on
the same grid: the same frames read through the same masked reader, an FFT in float32 in place of the binary64 lags and recursion.  The
residual (order 16, float32 and int16, coefficients float32 from the analysis) at hop 256 (coefficient rows staged in LDS) and at hop 8
(read per lane) beside pcmTensor(float32) of the same rows: the traffic floor of 2 B read and 4 B written per sample.  Each pair is timed
with events on torch's stream over REPS launches after WARM warm-ups, the export and its comparison alternating; medians, with the spread
(min, max) of each.  Two rows of every case are checked against the host's statement.  The operations counted are the binary64
multiply-adds the definition needs: nWin (order + 1) for the lags and order^2 for the recursion per step, order per sample for the
inverse filter.  No target is set in advance.
The synthesis row (speechPlayer_batch_exportLpcSynthesisOf; csrc/klatt_lpcsynth.h) needs no batch content: a float32 signal of `rows` rows
of 16 000 samples (1 s at 16 kHz) of noise through 1 / A(z) of order 16 at hop 160, float32 coefficients of stable random filters, float32
out, beside filteredTensor with 8 resonator sections on the same rows -- the other lane-per-row recursion, with a comparable count of
dependent multiply-adds per sample (16 binary64 against 8 x 5 binary32, two of the five on the critical path of each section).
Usage: python tools/lpc_probe.py [n_utt]
       python tools/lpc_probe.py synthesis [rows]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

synthesis_only = len(sys.argv) > 1 and sys.argv[1] == "synthesis"
n = int(sys.argv[2 if synthesis_only else 1]) if len(sys.argv) > (2 if synthesis_only else 1) else (4096 if synthesis_only else 65536)
WARM, REPS = 3, 10


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


def synthesis_row(rows, length=16000, order=16, hop=160):
    bp = eng.BatchPlayer(16000)
    dev = "cuda:%d" % bp.device
    rng = np.random.default_rng(1)
    steps = -(-length // hop)
    bank = np.array([eng.lpcFromReflection(rng.uniform(-0.9, 0.9, order)) for _ in range(512)], np.float32)
    lpc = torch.from_numpy(bank[rng.integers(0, 512, (rows, steps))]).to(dev)
    x = torch.from_numpy((rng.standard_normal((rows, length)) * 0.01).astype(np.float32)).to(dev)
    signal = (x, torch.full((rows,), length, dtype=torch.int64))
    centres = np.array([500.0, 900.0, 1500.0, 2100.0, 2500.0, 3300.0, 4200.0, 5000.0])
    sections = eng.resonatorSections(centres, 80.0 + 0.02 * centres, 16000)
    kw = dict(order=order, hop=hop)
    got, lens = bp.lpcSynthesisTensor(lpc[:2].contiguous(), utterances=np.arange(2), signal=signal, **kw)
    two = x[:2].cpu().numpy()
    ok = all(same(got[u].cpu().numpy(), eng.signalLpcSynthesis(two[u], lpc[u].cpu().numpy(), hop=hop)) for u in range(2))
    del got
    med, ms = pair(bp, lambda: bp.lpcSynthesisTensor(lpc, signal=signal, **kw)[0], "filtered_8_sections", lambda: bp.filteredTensor(sections, signal=signal)[0])
    samples = rows * length
    print(json.dumps({"case": "synthesis", "order": order, "hop": hop, "rows": rows, "samples": samples, "in": "float32", "coefficients": "float32", "out": "float32",
                      "statement_bits": ok, "ms": ms, "export_over_filtered": round(med["export"] / med["filtered_8_sections"], 3),
                      "samples_per_second": float("%.4g" % (samples / (med["export"] * 1e-3))), "f64_fma_per_second": float("%.4g" % (samples * order / (med["export"] * 1e-3))),
                      "filtered_samples_per_second": float("%.4g" % (samples / (med["filtered_8_sections"] * 1e-3)))}), flush=True)
    bp.close()


if synthesis_only:
    synthesis_row(n)
    sys.exit(0)
bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
samples = int(bp.totalSamples)
two = [bp.read(u) for u in range(2)]
for order, nWin, hop, nFft in ((16, 512, 256, 512), (32, 1024, 256, 1024), (10, 400, 160, 512)):
    kw = dict(order=order, nWin=nWin, hop=hop, fields=("lpc", "error"))
    got, steps = bp.lpcTensor(utterances=np.arange(2), **kw)
    ok = all(same(got[u, :int(steps[u])].cpu().numpy(), eng.pcmLpc(two[u], **kw).astype(np.float32)) for u in range(2))
    del got
    med, ms = pair(bp, lambda: bp.lpcTensor(**kw)[0], "spectrogram", lambda: bp.spectrogramTensor(nFft=nFft, hop=hop)[0])
    total = int(np.sum(-(-np.array([bp.utteranceSamples(u) for u in range(bp.nUtterances)], np.int64) // hop)))
    fma = total * (nWin * (order + 1) + order * order)
    print(json.dumps({"case": "analysis", "order": order, "nWin": nWin, "hop": hop, "beside_nFft": nFft, "n_utt": int(bp.nUtterances), "samples": samples, "steps": total,
                      "statement_bits": ok, "ms": ms, "export_over_spectrogram": round(med["export"] / med["spectrogram"], 3),
                      "steps_per_second": float("%.4g" % (total / (med["export"] * 1e-3))), "f64_fma_per_second": float("%.4g" % (fma / (med["export"] * 1e-3)))}), flush=True)
for hop in (256, 8):
    for dtype, npt in ((torch.float32, np.float32), (torch.int16, np.int16)):
        kw = dict(order=16, hop=hop)
        lpc, _ = bp.lpcTensor(nWin=512, fields="lpc", **kw)
        got, lens = bp.lpcResidualTensor(lpc[:2].contiguous(), utterances=np.arange(2), dtype=dtype, **kw)
        ok = all(same(got[u, :int(lens[u])].cpu().numpy(), eng.pcmLpcResidual(two[u], eng.pcmLpc(two[u], nWin=512, fields="lpc", **kw).astype(np.float32), hop=hop, dtype=npt))
                 for u in range(2))
        del got
        med, ms = pair(bp, lambda: bp.lpcResidualTensor(lpc, dtype=dtype, **kw)[0], "pcm_float32", lambda: bp.pcmTensor(dtype=torch.float32)[0])
        print(json.dumps({"case": "residual", "order": 16, "hop": hop, "out": np.dtype(npt).name, "n_utt": int(bp.nUtterances), "samples": samples, "statement_bits": ok, "ms": ms,
                          "export_over_pcm_float32": round(med["export"] / med["pcm_float32"], 3), "samples_per_second": float("%.4g" % (samples / (med["export"] * 1e-3))),
                          "f64_fma_per_second": float("%.4g" % (samples * 16 / (med["export"] * 1e-3)))}), flush=True)
        del lpc
bp.close()
synthesis_row(4096)
