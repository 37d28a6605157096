"""The spectrogram export (speechPlayer_batch_exportSpectrogram, csrc/klatt_spectrum.h) beside the torch composition over the public API
it replaces -- pcmTensor(float32) -> torch.stft(center=True, pad_mode="constant", periodic Hann) -> abs() ** 2 -> matmul with the mel
matrix -> clamp -> log -- on BASELINE configs[1] (4096 one-second vowels) and a 4096-utterance cut of configs[2], in ONE process:
nFft 1024, hop 256, 80 slaney mel bands, power 2, natural log, float32, padded.  Each is timed with events on torch's stream over REPS
launches after WARM warm-ups, the two alternating; the composition's peak memory is torch's peak allocation above what the batch's PCM
export already holds.  Algorithmic bytes of the export: 2 B per sample read + 4 B per (step, band) written; roofline 8 TB/s.
Usage: python tools/spectrogram_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
WARM, REPS = 3, 20
NFFT, HOP, MELS, FLOOR = 1024, 256, 80, 1e-10
PEAK_TBS = 8.0

bank = eng.melFilterbank(22050, NFFT, MELS, norm="slaney")


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def probe(name, bp):
    bp.synthesize()
    dev = "cuda:%d" % bp.device
    stream = torch.cuda.current_stream(bp.device)
    mel = torch.from_numpy(bank.astype(np.float32)).to(dev)
    window = torch.hann_window(NFFT, periodic=True, device=dev)

    def export():
        return bp.spectrogramTensor(nFft=NFFT, hop=HOP, bank=bank, power=2, log="ln", floor=FLOOR)[0]

    def composition():
        pcm, _ = bp.pcmTensor()
        power = torch.stft(pcm, NFFT, hop_length=HOP, window=window, center=True, pad_mode="constant", return_complex=True).abs() ** 2
        return torch.log(torch.clamp(torch.matmul(mel, power), min=FLOOR)).transpose(1, 2)

    ms = {"export": [], "composition": []}
    peak = 0
    for r in range(WARM + REPS):
        for case, fn in (("export", export), ("composition", composition)):      # alternating
            if case == "composition":
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(bp.device)
                before = torch.cuda.memory_allocated(bp.device)
            t, out = timed(stream, fn)
            if case == "composition":
                peak = max(peak, torch.cuda.max_memory_allocated(bp.device) - before)
            else:
                steps = out.shape[0] * out.shape[1]
            del out
            if r >= WARM:
                ms[case].append(t)
    # the two agree where both have frames (the composition frames the padding past each utterance's end as well)
    a, steps_of = bp.spectrogramTensor(nFft=NFFT, hop=HOP, bank=bank, power=2, log="ln", floor=FLOOR, utterances=np.arange(4))
    b = composition()[:4]
    worst = max(float((a[i, :int(steps_of[i]) - 2] - b[i, :int(steps_of[i]) - 2]).abs().max()) for i in range(4))
    samples, total_steps = int(bp.totalSamples), int(bp._steps("probe", None, HOP, 0)[2].sum())
    bytes_ = 2 * samples + 4 * total_steps * MELS
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"case": name, "n_utt": int(bp.nUtterances), "samples": samples, "steps": total_steps, "padded_steps": int(steps),
            "export_ms": {"median": round(med["export"], 3), "min": round(min(ms["export"]), 3), "max": round(max(ms["export"]), 3)},
            "composition_ms": {"median": round(med["composition"], 3), "min": round(min(ms["composition"]), 3), "max": round(max(ms["composition"]), 3)},
            "composition_peak_mb": round(peak / 1e6, 1), "algorithmic_mb": round(bytes_ / 1e6, 2),
            "export_gb_per_s": round(bytes_ / 1e6 / med["export"], 1), "export_roofline_fraction": round(bytes_ / 1e9 / med["export"] / PEAK_TBS, 4),
            "speedup": round(med["composition"] / med["export"], 2), "largest_difference_of_logs": worst}


b = workloads.make("cfg1", n)
bp = eng.BatchPlayer(22050)
bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
print(json.dumps(probe("configs[1]", bp)), flush=True)
bp.close()
bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
print(json.dumps(probe("configs[2] cut", bp)), flush=True)
bp.close()
