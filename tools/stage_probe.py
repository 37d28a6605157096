"""Times the signal stages (BatchPlayer.resampleStage / filterStage / codeStage; csrc/klatt_stage.h; convolveStage / spectrogramStage;
csrc/klatt_stage_window.h) beside the whole-row exports of a signal on the same tensor in the same run, alternating the two: one push of
1024 rows x 8192 float32 samples at 22050 -> 16000 against resampledTensor(signal=), the same through the four-section telephone band
against filteredTensor(signal=), through a 4096-tap response against convolvedTensor(signal=) and into a 1024-point, 80-band mel
spectrogram against spectrogramTensor(signal=), and -- --families lpc,pitch; csrc/klatt_stage_frames.h -- into the LPC analysis (order 16,
512 / 256) against lpcTensor(signal=) and the pitch (1024 / 256, lags 44 .. 368) against pitchTensor(signal=), and the single-row
8192-sample push a one-stream caller pays, per kind; then, --long, 64
rows through a 65536-tap response, where a push copies 65535 float32 of history per row, and, --short, 16384 rows x 256 samples through the
resampler, where the history copy's share of a push is largest.  Two figures per call: `queued`, device events around REPS calls issued back to back, per call --
what the kernels and the staging copy take once the host runs ahead --, and `alone`, a host clock around one call and a synchronise.
Prints one JSON object; --out writes it to a file as well.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# scipy.signal.butter(4, [300, 3400], "bandpass", fs=22050, output="sos"): the telephone band, four sections
TELEPHONE = np.array([
    [0.015031869558932728, 0.030063739117865456, 0.015031869558932728, 1.0, -0.790740694160057, 0.1990626472143866],
    [1.0, 2.0, 1.0, 1.0, -0.9114585623463567, 0.5756179539149701],
    [1.0, -2.0, 1.0, 1.0, -1.829051960405075, 0.8381042282374366],
    [1.0, -2.0, 1.0, 1.0, -1.9368246537081515, 0.9441864241806792]])
REPS, ROUNDS, SAMPLES = 20, 5, 8192


def measure(calls, dev, reps=None):
    """calls: name -> function.  ROUNDS rounds, the functions alternating within a round: -> name -> (queued ms per call: the median and the
    range over the rounds, alone ms per call: the same)."""
    import torch
    for fn in calls.values():      # warm up: code objects, staging slots, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    queued, alone = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps or REPS):
                fn()
            b.record()
            torch.cuda.synchronize(dev)
            queued[name].append(a.elapsed_time(b) / (reps or REPS))
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            alone[name].append((time.perf_counter() - t) * 1e3)
    spread = lambda v: dict(median=round(float(np.median(v)), 4), low=round(min(v), 4), high=round(max(v), 4))
    return {k: dict(queued_ms=spread(queued[k]), alone_ms=spread(alone[k])) for k in calls}


def room_response(taps):
    rng = np.random.default_rng(taps)
    return (rng.normal(0.0, 1.0, taps) * np.exp(-np.arange(taps) / (0.2 * taps))).astype(np.float32)


def main():
    import torch
    import nvspeechplayer_amd as eng
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--families", default="resample,filter,adpcm,convolution,spectrogram", help="comma-separated: which rows to time")
    ap.add_argument("--long", action="store_true", help="also 64 rows through a 65536-tap response")
    ap.add_argument("--short", action="store_true", help="also 16384 rows x 256 samples through the resampler, 22050 -> 16000")
    ap.add_argument("--exports-only", action="store_true", help="the whole-row exports alone: an A/B of two builds of the library (SPEECHPLAYER_LIB)")
    args = ap.parse_args()
    families = args.families.split(",")
    bp = eng.BatchPlayer(22050)
    dev = bp.device
    rng = np.random.default_rng(1)
    result = {}
    for rows in (1024, 1):
        x = torch.from_numpy(rng.uniform(-1.0, 1.0, (rows, SAMPLES)).astype(np.float32)).to("cuda:%d" % dev)
        signal = (x, np.full(rows, SAMPLES, np.int64))
        room, mel = room_response(4096), eng.melFilterbank(22050, 1024, 80)
        # family -> (its stage's maker, its push's name, the whole-row export's name and call); a stage is made for the families asked for alone.
        # lpc: order 16, 512 / 256, lpc + error -- a row's 32 steps are one workgroup of 64; pitch: 1024 + 368 lags / 256 at 22050 Hz, f0 +
        # aperiodicity -- two workgroups of 16 steps
        every = {"resample": (lambda: bp.resampleStage(rows, 22050, 16000), "resample stage push", "resampledTensor(signal=)", lambda: bp.resampledTensor(16000, signal=signal)),
                 "filter": (lambda: bp.filterStage(rows, TELEPHONE), "filter stage push", "filteredTensor(signal=)", lambda: bp.filteredTensor(TELEPHONE, signal=signal)),
                 "adpcm": (lambda: bp.codeStage(rows, "adpcm"), "adpcm stage push", "codedTensor(adpcm, signal=)", lambda: bp.codedTensor("adpcm", signal=signal)),
                 "convolution": (lambda: bp.convolveStage(rows, room, tail=False), "convolution stage push, 4096 taps", "convolvedTensor(4096 taps, tail=False, signal=)",
                                 lambda: bp.convolvedTensor(room, tail=False, signal=signal)),
                 "spectrogram": (lambda: bp.spectrogramStage(rows, 1024, 256, bank=mel, log="db"), "spectrogram stage push, 1024 / 256, 80 mel, db",
                                 "spectrogramTensor(1024 / 256, 80 mel, db, signal=)", lambda: bp.spectrogramTensor(1024, 256, bank=mel, log="db", signal=signal)),
                 "lpc": (lambda: bp.lpcStage(rows), "lpc stage push, order 16, 512 / 256", "lpcTensor(order 16, 512 / 256, signal=)", lambda: bp.lpcTensor(signal=signal)),
                 "pitch": (lambda: bp.pitchStage(rows, 22050), "pitch stage push, 1024 / 256, lags 44 .. 368", "pitchTensor(1024 / 256, lags 44 .. 368, signal=)",
                           lambda: bp.pitchTensor(signal=signal, sampleRate=22050))}
        stages, calls = [], {}
        for family in families:
            make, push_name, export_name, export = every[family]
            if not args.exports_only:
                stages.append(make())
                calls[push_name] = (lambda s: lambda: s.push(signal))(stages[-1])
            calls[export_name] = export
        result["%d rows x %d float32" % (rows, SAMPLES)] = measure(calls, dev)
        for s in stages:
            s.close()
    if args.long:      # the history copy at its largest: 65535 float32 per row and push beside 8192 x 65536 taps of arithmetic per row
        rows = 64
        x = torch.from_numpy(rng.uniform(-1.0, 1.0, (rows, SAMPLES)).astype(np.float32)).to("cuda:%d" % dev)
        signal = (x, np.full(rows, SAMPLES, np.int64))
        room = room_response(65536)
        con = bp.convolveStage(rows, room, tail=False)
        calls = {"convolution stage push, 65536 taps": lambda: con.push(signal),
                 "convolvedTensor(65536 taps, tail=False, signal=)": lambda: bp.convolvedTensor(room, tail=False, signal=signal)}
        result["%d rows x %d float32, 65536 taps" % (rows, SAMPLES)] = measure(calls, dev, reps=4)
        con.close()
    if args.short:      # the resampler's history copy at its largest share: 2 Z - 1 = 17 float32 of history a row beside 256 samples of chunk
        rows, samples = 16384, 256
        x = torch.from_numpy(rng.uniform(-1.0, 1.0, (rows, samples)).astype(np.float32)).to("cuda:%d" % dev)
        signal = (x, np.full(rows, samples, np.int64))
        res = bp.resampleStage(rows, 22050, 16000)
        calls = {"resample stage push": lambda: res.push(signal), "resampledTensor(signal=)": lambda: bp.resampledTensor(16000, signal=signal)}
        result["%d rows x %d float32" % (rows, samples)] = measure(calls, dev)
        res.close()
    bp.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
