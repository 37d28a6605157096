"""The coded export (speechPlayer_batch_exportCoded, csrc/klatt_codec.h) on a cut of BASELINE configs[2] set from IPA text, in ONE process,
padded rows throughout.  G.711 (mu-law and A-law; decoded int16, codes only, both) beside pcmTensor(int16) of the same rows: the same 2 B
read per sample and no more bytes written than its 2 B, so the copy is the traffic floor.  ADPCM (decoded int16, codes only, both) beside
filteredTensor of one section, int16 out: the same walk -- a wavefront per 64 rows, tiles of 64 samples through LDS -- with the integer
recursion in place of five float32 operations.  Each pair is timed with events on torch's stream over REPS launches after WARM warm-ups,
the export and its comparison alternating; medians, with the spread (min, max) of each.  Two rows of every case are checked against the
host's statement.  The mu-law cases run twice, before and behind A-law's: a control against the order of the cases.  No target is set in
advance.
Usage: python tools/codec_probe.py [n_utt]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nvspeechplayer_amd as eng  # noqa: E402
from nvspeechplayer_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
WARM, REPS = 3, 10
OUTPUTS = {"decoded_int16": dict(), "codes": dict(codes=True, decoded=False), "both": dict(codes=True)}
BYTES_OUT = {"decoded_int16": 2, "codes": 1, "both": 3}


def timed(stream, fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def exact(bp, codec, kw):
    """Rows 0 and 1 of the export against pcmCode."""
    got = bp.codedTensor(codec, utterances=np.arange(2), **kw)
    lens = got[-1]
    want = eng.pcmCode
    for u in range(2):
        w = want(bp.read(u), codec, codes=kw.get("codes", False), decoded=kw.get("decoded", True))
        w = w if isinstance(w, tuple) else (w,)
        for g, x in zip(got[:-1], w):
            if not np.array_equal(g[u, :int(lens[u])].cpu().numpy(), x):
                return False
    return True


def probe(bp, codec, name, floor_name, floor):
    stream = torch.cuda.current_stream(bp.device)
    kw = OUTPUTS[name]
    ms = {"export": [], floor_name: []}
    for r in range(WARM + REPS):
        for case, fn in (("export", lambda: bp.codedTensor(codec, **kw)[0]), (floor_name, floor)):      # alternating
            t, out = timed(stream, fn)
            del out
            if r >= WARM:
                ms[case].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    samples = int(bp.totalSamples)
    padded = int(bp.nUtterances) * max(bp.utteranceSamples(u) for u in range(bp.nUtterances))
    spread = (max(ms[floor_name]) - min(ms[floor_name])) / med[floor_name]
    return {"codec": codec, "outputs": name, "n_utt": int(bp.nUtterances), "samples": samples, "padded_elements": padded, "statement_bits": exact(bp, codec, kw),
            "ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
            "export_over_" + floor_name: round(med["export"] / med[floor_name], 3), floor_name + "_spread": round(spread, 3),
            "bytes_moved": 2 * samples + BYTES_OUT[name] * padded, "bytes_per_second": float("%.4g" % ((2 * samples + BYTES_OUT[name] * padded) / (med["export"] * 1e-3))),
            "samples_per_second": float("%.4g" % (samples / (med["export"] * 1e-3)))}


bp = eng.BatchPlayer(22050)
bp.setIpa(**workloads.cfg2_spec(n))
bp.synthesize()
identity = np.array([[1, 0, 0, 0, 0]], np.float32)
for codec in ("ulaw", "alaw", "ulaw"):      # (mu-law again behind A-law: a control against the order of the cases)
    for name in OUTPUTS:
        print(json.dumps(probe(bp, codec, name, "pcm_int16", lambda: bp.pcmTensor(dtype=torch.int16)[0])), flush=True)
for name in OUTPUTS:
    print(json.dumps(probe(bp, "adpcm", name, "filtered_1_int16", lambda: bp.filteredTensor(identity, dtype=torch.int16)[0])), flush=True)
bp.close()
