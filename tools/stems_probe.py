"""The stems export (speechPlayer_batch_exportStems, csrc/klatt_stems.h) beside its yardstick, the lane kernel's synthesis of the same
batch (options layout 0, tracks 0, direct 0: the same per-lane arithmetic with 2 bytes stored per sample), in ONE process on
scenarios.random_batch(default_rng(3), n, quiet_fraction=0.0).  Every export is timed with events on the export's stream after a warm-up,
the cases alternating; medians of REPS runs.  Writes profiles/stems_export.txt, the kernels' resource figures (tools/kernel_resources.py)
at its head.
Usage: python tools/stems_probe.py [n_utt [out_path]]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nvspeechplayer_amd as eng  # noqa: E402
from tests import scenarios  # noqa: E402
import kernel_resources  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "stems_export.txt")
WARM, REPS = 1, 5

b = scenarios.random_batch(np.random.default_rng(3), n, quiet_fraction=0.0)
bp = eng.BatchPlayer(22050)
for name in ("layout", "tracks", "direct"):
    bp.setOption(name, 0)
bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
samples = int(bp.totalSamples)
lens = bp._lengths()
cases = {
    '["source"] float32': (["source"], torch.float32),
    '["source", "output"] float32': (["source", "output"], torch.float32),
    "all seven float32": (list(range(7)), torch.float32),
    "all seven float64": (list(range(7)), torch.float64),
}
stream = torch.cuda.current_stream(bp.device)
ms = {k: [] for k in cases}
written = {}
lane = []
for r in range(WARM + REPS):
    for case, (cols, dtype) in cases.items():      # alternating: no case always follows the same one
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = bp.stemTensor(cols, dtype=dtype, padded=False)[0]
        e1.record(stream)
        e1.synchronize()
        written[case] = out.numel() * out.element_size()
        del out
        if r >= WARM:
            ms[case].append(e0.elapsed_time(e1))
    t = float(bp.time(1)[0])
    if r >= WARM:
        lane.append(t)
info = bp.kernelInfo()
bp.close()

yard = float(np.median(lane))
lines = ["Stems export (speechPlayer_batch_exportStems, csrc/klatt_stems.h) -- tools/stems_probe.py", "",
         "Registers, scratch and LDS (gfx950 code object of the built library; dynamic LDS is sized at launch: 46 080 B of frame slots +",
         "64 x (distinct columns x tile samples x element size + 8) + 1 024 B: 51 712 B for one float32 column, 80 384 B at most):", "",
         "%-60s %5s %5s %5s %8s %6s" % ("kernel", "vgpr", "agpr", "sgpr", "scratch", "spills")]
for k in sorted(kernel_resources.kernels(), key=lambda k: k["pretty"]):
    if "klatt_stems" in k["pretty"] or "klatt_synthesize<0, false, true>" in k["pretty"]:
        lines.append("%-60s %5d %5d %5d %8d %6d" % (k["pretty"].split("(")[0][:60], k["vgpr"], k["agpr"], k["sgpr"], k["scratch"], k["spill"]))
lines += ["", "One MI355X, one process: scenarios.random_batch(default_rng(3), %d, quiet_fraction=0.0) at 22 050 Hz, %d utterances, %d samples,"
          % (n, n, samples),
          "longest %d, shortest %d; packed output.  Events on the export's stream around stemTensor, the cases alternating with one lane-kernel"
          % (int(lens.max()), int(lens.min())),
          "synthesis launch (speechPlayer_batch_time, options layout 0, tracks 0, direct 0: %d wavefronts), %d warm-up, medians of %d (min .. max)."
          % (info["wavefronts"], WARM, REPS), "",
          "%-34s %-30s %12s %10s %14s" % ("", "ms", "MB written", "GB/s", "x lane kernel")]
for case in cases:
    m = float(np.median(ms[case]))
    lines.append("%-34s %-30s %12.1f %10.1f %14.2f" % (case, "%.3f (%.3f .. %.3f)" % (m, min(ms[case]), max(ms[case])), written[case] / 1e6,
                                                       written[case] / m / 1e6, m / yard))
lines.append("%-34s %-30s %12.1f %10.1f %14.2f" % ("yardstick: lane kernel, int16 PCM", "%.3f (%.3f .. %.3f)" % (yard, min(lane), max(lane)),
                                                   samples * 2 / 1e6, samples * 2 / yard / 1e6, 1.0))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
