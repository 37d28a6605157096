"""Every batch path and the live handles at every sample rate, on utterances whose formants and bandwidths reach every class of the
coefficient code (needs a GPU).

At 22.05 kHz speech keeps exp(-pi bw / sr) unreduced below bw = 2433 Hz and cos(2 pi (-f) / sr) in quadrants 0 and -1 below
f = 8269 Hz, so batches of ordinary formants never reach the general class of the direct stages, fast_exp with k != 0, fast_cos beyond
quadrant -1, or the 0.499 / 0.501 margins of fade_classes and klatt_seeds.  edge_batch gives frequencies and bandwidths as fractions
of the sample rate, so every rate sees every class: formants within 0.3 % of sr / 8 and 3 sr / 8 (the quadrant boundaries) and exactly
on the margins, above Nyquist and negative; bandwidths on both sides of the exp margin; a few utterances beyond the direct stages'
eligibility bounds.  Each path is forced with the options the ABI has and kernelInfo() confirms it ran.  MODE_EXACT: all paths give
the same bytes; every path and mode against the oracle at the usual bar; lengths and index marks exactly.
"""
import numpy as np
import pytest

from tests import oracle
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 16000, 22050, 44100, 48000)
N_UTT = 7 * 64 + 37          # seven full wavefronts and a ragged eighth
THREADS = 16

# (name, options, what kernelInfo() must show)
PATHS = (
    ("lane kernel", dict(layout=0), None),
    ("stages, frame state machine", dict(layout=1, tracks=0, direct=0), None),
    ("flat stages on tracks", dict(layout=1, tracks=1, direct=0), lambda i: i["tracked_utterances"] > 0),
    ("direct stages, one workgroup per CU", dict(tracks=0, direct=2, direct_lean=0),
     lambda i: i["direct_utterances"] > 0 and i["stage_parallel_chunk"] == 16),
    ("direct stages, two workgroups per CU", dict(tracks=0, direct=2, direct_lean=1),
     lambda i: i["direct_utterances"] > 0 and i["stage_parallel_chunk"] == 8),
    ("lane-pipelined kernel", dict(layout=2), lambda i: i["lane_pipelined_utterances"] > 0),
    ("engine's choice", dict(layout=-1), None),
)


def edge_batch(rng, sr, n_utt):
    """Ragged utterances (timing as random_batch in tests/test_gpu_parity.py) whose frequencies and bandwidths are fractions of sr.
    Formants over (0, 0.45 sr), a share within 0.3 % of sr / 8 and 3 sr / 8, some exactly on the class margins (0.12475, 0.12525,
    0.37475, 0.37525 sr), some above Nyquist (to 0.9 sr), some negative (to -0.3 sr); N0 = 0 Hz in some frames.  Bandwidths over
    (0, 0.2 sr), a share at 0.1101 sr and 0.1104 sr (x log2e of exp's argument at 0.4991 and 0.5004: the margin) and beyond 0.33 sr
    (k = -2), 0 in some frames.  Quiet nasal-free utterances mixed with noisy and nasal ones; fades longer than their frame, 1-sample
    fades, M = 0 frames and NULL frames; vibrato; index marks.  One utterance in 40 has a frame beyond the direct stages' bounds
    (|f| > 9900 sr / 2 pi or bw > 690 sr / pi): the device library's exp / cos and the planner's fallbacks."""
    margins = np.array([0.12475, 0.12525, 0.37475, 0.37525])

    def freq(n):
        kind = rng.integers(0, 20, n)
        f = rng.uniform(0.0, 0.45, n)
        near = rng.choice([0.125, 0.375], n) * (1.0 + rng.uniform(-0.003, 0.003, n))
        f = np.where(kind < 4, near, f)
        f = np.where(kind == 4, rng.choice(margins, n), f)
        f = np.where((kind == 5) | (kind == 6), rng.uniform(0.5, 0.9, n), f)
        f = np.where(kind == 7, rng.uniform(-0.3, 0.0, n), f)
        return f * sr

    def bandwidth(n):
        kind = rng.integers(0, 20, n)
        b = rng.uniform(0.0, 0.2, n)
        b = np.where(kind < 3, rng.choice([0.1101, 0.1104], n), b)
        b = np.where(kind == 3, rng.uniform(0.33, 0.5, n), b)
        b = np.where((kind == 4) & (rng.random(n) < 0.5), 0.0, b)
        return b * sr

    frames, mins, fades, idx, nul, start, seeds = [], [], [], [], [], [0], []
    for u in range(n_utt):
        n = int(rng.integers(1, 9))
        quiet = rng.random() < 0.35
        nasal = rng.random() < 0.5
        beyond = u % 40 == 17
        for k in range(n):
            f = np.zeros(47)
            f[0] = rng.uniform(40, 400); f[46] = f[0] * rng.uniform(0.6, 1.6)
            if rng.random() < 0.3:
                f[1] = rng.uniform(0, 0.2); f[2] = rng.uniform(0, 8)                 # vibrato
            f[5] = rng.uniform(0, 1)
            if not quiet:
                f[3] = rng.uniform(0, 0.5) * (rng.random() < 0.5); f[4] = rng.uniform(0, 1)
                f[6] = rng.uniform(0, 1) * (rng.random() < 0.5); f[24] = rng.uniform(0, 1) * (rng.random() < 0.6)
            f[7:13] = freq(6)
            f[13] = freq(1)[0] * (rng.random() < 0.7); f[14] = freq(1)[0]          # N0 = 0 Hz in some frames
            f[15:23] = bandwidth(8)
            f[23] = rng.uniform(0, 1) * (nasal and rng.random() < 0.7)
            if not nasal:
                f[21] = max(f[21], 1.0)                                               # a nasal-free N0 bandwidth (klatt_plan.h)
            f[25:31] = freq(6); f[31:37] = bandwidth(6); f[37:43] = rng.uniform(0, 1, 6)
            f[43] = rng.uniform(0, 1); f[44] = rng.uniform(0, 1.5); f[45] = rng.uniform(0.2, 2.5)
            if beyond and k == n // 2:
                if rng.random() < 0.5:
                    f[7 + int(rng.integers(0, 6))] = rng.choice([-1, 1]) * rng.uniform(1600.0, 3000.0) * sr
                else:
                    f[15 + int(rng.integers(0, 6))] = rng.uniform(230.0, 400.0) * sr
            is_null = rng.random() < 0.2 and not (beyond and k == n // 2)
            frames.append(f); nul.append(is_null)
            mode = rng.integers(0, 5)
            if mode == 0: m, fd = int(rng.integers(0, 4)), int(rng.integers(0, 4))
            elif mode == 1: m, fd = int(rng.integers(1, 300)), int(rng.integers(300, 900))       # fade longer than the frame
            else: m, fd = int(rng.integers(50, 2500)), int(rng.integers(0, 700))
            if not is_null and m == 0 and u % 8 != 3:
                m = 1                   # M = 0 on a real frame divides by zero (reference src/frame.cpp:98; a NaN pitch from there on): one utterance in 8
            mins.append(m); fades.append(fd)
            idx.append(int(rng.integers(0, 5000)) if rng.random() < 0.3 else -1)
        start.append(start[-1] + n); seeds.append(int(rng.integers(0, 2 ** 31)))
    return dict(frames=np.array(frames), min=np.array(mins, np.uint32), fade=np.array(fades, np.uint32),
                index=np.array(idx, np.int32), isnull=np.array(nul, np.uint8), frame_start=np.array(start, np.int64),
                seeds=np.array(seeds, np.uint32))


def _set(bp, b):
    bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])


@pytest.mark.parametrize("sr", RATES)
def test_batch_paths_at_every_rate(sr):
    """edge_batch at `sr` through every batch path, both arithmetic modes: lengths and index marks equal the oracle's; MODE_EXACT's
    PCM is the same bytes on every path and within the usual bar of the oracle; MODE_FAST's within the usual bar on every path."""
    import nvspeechplayer_amd as eng
    rng = np.random.default_rng(sr)
    batch = edge_batch(rng, sr, N_UTT)
    exp, exp_start, total = oracle.batch_synthesize(sr, batch, threads=THREADS)
    marks = oracle.batch_last_index(sr, batch, threads=THREADS).tolist()
    assert sum(1 for x in marks if x != -1) > N_UTT // 2
    exact = {}
    for mode in (0, 1):
        for name, opts, check in PATHS:
            bp = eng.BatchPlayer(sr, mode=mode, layout=opts.get("layout"))
            for k, v in opts.items():
                if k != "layout":
                    bp.setOption(k, v)
            _set(bp, batch)
            info = bp.kernelInfo()
            assert check is None or check(info), (sr, mode, name, info)
            assert bp.totalSamples == total
            bp.synthesize()
            got, got_start = bp.readAll()
            assert np.array_equal(got_start, exp_start), (sr, mode, name)
            assert [bp.getLastIndex(u) for u in range(N_UTT)] == marks, (sr, mode, name)
            bp.close()
            flips = 0
            for u in range(N_UTT):
                flips += compare(got[got_start[u]:got_start[u + 1]], exp[exp_start[u]:exp_start[u + 1]], "%d Hz mode %d %s utt %d" % (sr, mode, name, u))
            print("%d Hz mode %d %-38s %d samples, %d one-LSB differences from the oracle; direct %d tracked %d lane-pipelined %d" % (
                sr, mode, name, total, flips, info["direct_utterances"], info["tracked_utterances"], info["lane_pipelined_utterances"]))
            if mode == 0:
                exact[name] = got.copy()
    first = PATHS[0][0]
    for name in exact:
        d = np.flatnonzero(exact[name] != exact[first])
        assert len(d) == 0, "%d Hz MODE_EXACT: %s and %s differ in %d samples (utterances %s)" % (
            sr, name, first, len(d), sorted(set((np.searchsorted(exp_start, d, side="right") - 1).tolist()))[:10])
    _exact_pcm[sr] = (batch, exact[first], exp_start)


_exact_pcm = {}      # rate -> (edge batch, its MODE_EXACT PCM, starts): what test_live_handles_at_every_rate compares with


def _live(sr, batch, utts, live_mode):
    """The utterances `utts` of `batch` as live handles created under live_mode, pulled together through synthesizeMany against
    oracle players: per pull, lengths and index marks exactly.  Returns each handle's PCM and its oracle's."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    assert L.speechPlayer_setGlobalOption(b"live_mode", live_mode) == 0
    fs = batch["frame_start"]
    players = [eng.SpeechPlayer(sr, noiseSeed=int(batch["seeds"][u])) for u in utts]
    oracles = [oracle.OraclePlayer(sr, seed=int(batch["seeds"][u])) for u in utts]
    for p, o, u in zip(players, oracles, utts):
        for j in range(int(fs[u]), int(fs[u + 1])):
            fr = None if batch["isnull"][j] else batch["frames"][j]
            p.queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), int(batch["min"][j]), int(batch["fade"][j]), int(batch["index"][j]))
            o.queue(fr, int(batch["min"][j]), int(batch["fade"][j]), int(batch["index"][j]))
    got = [[] for _ in utts]
    want = [[] for _ in utts]
    done = [False] * len(utts)
    pulls = 0
    while not all(done):
        n = (5000, 33, 8192)[pulls % 3]
        pulls += 1
        bufs = eng.SpeechPlayer.synthesizeMany(players, n)
        for k, b in enumerate(bufs):
            e = oracles[k].synthesize(n)
            g = np.zeros(0, np.int16) if b is None else np.frombuffer(b, dtype=np.int16)[:b.length].copy()
            assert len(g) == len(e) and players[k].getLastIndex() == oracles[k].last_index(), (sr, live_mode, k, pulls)
            got[k].append(g); want[k].append(e)
            done[k] = done[k] or len(g) < n
        assert pulls < 1000
    for p in players:
        p.close()
    return [np.concatenate(g) for g in got], [np.concatenate(e) for e in want]


@pytest.mark.parametrize("sr", RATES)
def test_live_handles_at_every_rate(sr):
    """32 edge utterances of test_batch_paths_at_every_rate's batch as live handles pulled together, under live_mode 0 (MODE_EXACT)
    and 1 (MODE_FAST): call lengths and index marks equal the oracle's, PCM within the usual bar; under live_mode 0 the PCM is the
    batch's MODE_EXACT bytes."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    if sr in _exact_pcm:
        batch, exact, start = _exact_pcm[sr]
    else:
        import nvspeechplayer_amd as eng
        batch = edge_batch(np.random.default_rng(sr), sr, N_UTT)
        bp = eng.BatchPlayer(sr)
        _set(bp, batch)
        bp.synthesize()
        exact, start = bp.readAll()
        bp.close()
    utts = [u for u in range(N_UTT) if u % 15 == 2][:32]
    assert len(utts) == 32 and any(u % 40 == 17 for u in utts)          # one beyond the direct stages' bounds among them
    try:
        for live_mode in (0, 1):
            pcm, want = _live(sr, batch, utts, live_mode)
            for k, u in enumerate(utts):
                compare(pcm[k], want[k], "%d Hz live_mode %d utt %d" % (sr, live_mode, u))
                if live_mode == 0:
                    assert np.array_equal(pcm[k], exact[start[u]:start[u + 1]]), (sr, u)
    finally:
        L.speechPlayer_setGlobalOption(b"live_mode", 0)
