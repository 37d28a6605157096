"""The exports of a signal (speechPlayer_batch_exportSpectrogramOf / exportResampledOf / exportConvolvedOf, csrc/klatt_tiles.h: the reader)
on a cut of BASELINE configs[2] set from IPA text, in ONE process: each export on pcmTensor(float32) handed back as signal= beside the same
export on the pool -- the same rows, the same arithmetic after the load, a 4-byte read against a 2-byte one -- and on pcmTensor(int16)
handed back, which differs from the pool only in where the rows lie; then the four-stage chain mix -> room -> 16 kHz -> log-mel beside
its torch composition over the public API (pcmTensor + noise, conv1d, a polyphase resampler as a gather of frames against the library's
own table, torch.stft and a matmul).  Each is timed with events on torch's stream over REPS launches after WARM warm-ups, alternating; medians.
No ratio is set in advance.
Usage: python tools/signal_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
WARM, REPS = 2, 7


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternating(stream, cases):
    ms = {k: [] for k in cases}
    for r in range(WARM + REPS):
        for case, fn in cases.items():
            t, out = timed(stream, fn)
            del out
            if r >= WARM:
                ms[case].append(t)
    return {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()}


def response(K):
    rng = np.random.default_rng(K)
    return (0.5 * rng.uniform(-1, 1, K) * np.exp(-5.0 * np.arange(K) / K)).astype(np.float32)


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
dev = "cuda:%d" % bp.device
stream = torch.cuda.current_stream(bp.device)
f32, i16 = bp.pcmTensor(dtype=torch.float32), bp.pcmTensor(dtype=torch.int16)
h = response(1024)
bank = eng.melFilterbank(16000, 512, 80)
spec = dict(nFft=512, hop=160, bank=bank, log="ln", floor=1e-5, dtype=torch.float32)

for name, pool, of in (
        ("resampled 22050 -> 16000", lambda: bp.resampledTensor(16000)[0], lambda s: bp.resampledTensor(16000, signal=s)[0]),
        ("convolved, 1024 taps, tail 0", lambda: bp.convolvedTensor(h, tail=False)[0], lambda s: bp.convolvedTensor(h, tail=False, signal=s)[0]),
        ("spectrogram nFft 512 hop 160 mel 80 ln", lambda: bp.spectrogramTensor(**spec)[0], lambda s: bp.spectrogramTensor(signal=s, **spec)[0])):
    ms = alternating(stream, {"pool": pool, "signal_float32": lambda: of(f32), "signal_int16": lambda: of(i16)})
    print(json.dumps({"export": name, "n_utt": int(bp.nUtterances), "samples": int(bp.totalSamples), "ms": ms,
                      "float32_over_pool": round(ms["signal_float32"]["median"] / ms["pool"]["median"], 3),
                      "int16_over_pool": round(ms["signal_int16"]["median"] / ms["pool"]["median"], 3)}), flush=True)

# ---- the chain beside its torch composition ----
rng = np.random.default_rng(1)
bp.setNoiseBank([rng.uniform(-0.5, 0.5, 50000).astype(np.float32)])
terms = [[eng.MixTerm(noise=0, snr=10.0, offset=u)] for u in range(int(bp.nUtterances))]
room = response(1024)
table, up, down = eng.resampleKernel(22050, 16000)
taps = table.shape[1]
flipped = torch.from_numpy(room[::-1].copy()).to(dev)[None, None, :]
noise = torch.from_numpy(rng.uniform(-0.5, 0.5, f32[0].shape[1]).astype(np.float32)).to(dev)
phases = torch.from_numpy(table.astype(np.float32)).to(dev)[:, None, :]      # [up, 1, taps]
mel = torch.from_numpy(bank.astype(np.float32)).to(dev)
window = torch.hann_window(512, periodic=True, device=dev)


def chain():
    noisy = bp.mixedTensor(terms)
    wet = bp.convolvedTensor(room, signal=noisy)
    x16k = bp.resampledTensor(16000, signal=wet)
    return bp.spectrogramTensor(signal=x16k, **spec)[0]


def composition():
    """The same stages in torch: the polyphase resampler gathers every output's `taps` inputs and multiplies them by its phase's row of the
    table -- what a user without a resampling library writes."""
    pcm, _ = bp.pcmTensor()
    noisy = pcm + 0.3 * noise[None, :]
    wet = torch.nn.functional.conv1d(torch.nn.functional.pad(noisy, (len(room) - 1, len(room) - 1))[:, None, :], flipped)[:, 0, :]
    L = wet.shape[1]
    m = torch.arange(-(-L * up // down), device=dev)
    n0, p = (m * down) // up, (m * down) % up
    frames = torch.nn.functional.pad(wet, (taps // 2 - 1, taps // 2 + 1)).unfold(1, taps, 1)      # [n, L + 1, taps] (a view)
    rows = 256      # (the gathered frames of all rows at once would not fit)
    out = []
    for a in range(0, wet.shape[0], rows):
        out.append((frames[a:a + rows][:, n0, :] * phases[p, 0, :][None]).sum(-1))
    x16k = torch.cat(out)
    S = torch.stft(x16k, 512, hop_length=160, window=window, center=True, pad_mode="constant", return_complex=True).abs() ** 2
    return torch.log(torch.clamp(torch.matmul(mel, S), min=1e-5))


try:
    ms = alternating(stream, {"chain": chain, "torch_composition": composition})
except RuntimeError as e:      # (the composition's gathered frames may not fit: the chain alone, then)
    print(json.dumps({"torch_composition": "unmeasured", "why": str(e)[:200]}), flush=True)
    ms = alternating(stream, {"chain": chain})
    ms["torch_composition"] = {"median": float("nan")}
print(json.dumps({"chain": "mixed -> convolved 1024 taps -> resampled 16000 -> log-mel 80", "n_utt": int(bp.nUtterances), "ms": ms,
                  "composition_over_chain": round(ms["torch_composition"]["median"] / ms["chain"]["median"], 2)}), flush=True)
bp.close()
