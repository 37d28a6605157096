"""What tests/test_stage_frames_host.py and tests/test_gpu_stage_frames.py share (no GPU): the geometries of the LPC and the pitch stage,
the input generator and the chunk plans.

A row's input is a function of the row, of the segment (the row's life between two ends) and of the sample's index n in that segment
alone, so the host test can judge the very streams the GPU test pushes without a GPU.  Row i is, by i mod 3:
  0   a harmonic tone (fundamental and two overtones) of `period` samples plus low noise, with a stretch of EXACT zeros longer than a frame
      plus two hops from sample `frame` of the segment on -- silent steps (LPC: 0 stages; pitch: unvoiced) beside the voiced ones;
  1   noise alone: unvoiced steps, every LPC stage run;
  2   the tone plus low noise throughout.
An int16 chunk is round(12000 v), a float32 chunk v itself."""
import functools

import numpy as np

F32 = np.float32
LPC_ALL, PITCH_ALL = 31, 63
# order, nWin, hop, phase, what, with a lag window
LPC_GEOMETRY = [(4, 33, 8, 0, LPC_ALL, False),            # an odd window; 375 steps in a 3000-sample push: groups of 64 straddle rows
                (16, 512, 160, 0, 2 | 8, True),          # lpc + error, behind a lag window
                (32, 700, 1000, 300, LPC_ALL, False),    # a hop above the frame: samples are skipped; four lag blocks of 8 and one lag more
                (9, 64, 64, 63, 1 | 16, False)]          # autocorr + stages; a short second lag block (lags 8 and 9)
# W, lagMin, lagMax, hop, phase, what
PITCH_GEOMETRY = [(32, 2, 65, 8, 0, PITCH_ALL),          # R = 4, two scan blocks; groups of 16 straddle rows
                  (160, 44, 300, 80, 5, 1 | 16 | 2),     # f0 + voiced + period; R = 6
                  (128, 20, 256, 700, 750, PITCH_ALL),   # R = 4 at its boundary; a hop above the frame
                  (64, 10, 257, 64, 0, 1)]               # f0; R = 6 at its boundary
PITCH_RATE, PITCH_THRESHOLD = 16000, 0.15
PUSHES = 7
LONGEST = 3000


def lpc_frame(g):
    """(before, after) of an LPC geometry's frame."""
    return g[1] // 2, g[1] - 1 - g[1] // 2


def pitch_frame(g):
    n = g[0] + g[2]
    return n // 2, n - 1 - n // 2


def lpc_period(g):
    return 100.3


def pitch_period(g):
    """A period inside the geometry's lags: near 100 samples where they hold it."""
    return 100.3 if g[1] < 90 and g[2] > 120 else 0.61 * g[2]


def lag_window(order):
    return np.exp(-0.5 * (2.0 * np.pi * 60.0 * np.arange(order + 1) / 16000.0) ** 2) * np.where(np.arange(order + 1) == 0, 1.0 + 2.0 ** -30, 1.0)


def plan(n, H, hop, seed):
    """Seven pushes: per push the rows' chunk lengths, drawn unsorted from {0, 1, H - 1, H, H + 1, hop, 1023, 3000}, and their end flags --
    rows end at different pushes and go on as fresh rows, the last push ends all."""
    rng = np.random.default_rng(seed)
    pool = [0, 1, H - 1, H, H + 1, hop, 1023, LONGEST]
    lens = [[int(pool[rng.integers(0, len(pool))]) for _ in range(n)] for _ in range(PUSHES)]
    end = np.zeros((PUSHES, n), np.uint8)
    for i in range(n):
        end[2 + (i + seed) % (PUSHES - 3), i] = 1
    end[-1, :] = 1
    return lens, end


@functools.lru_cache(maxsize=None)
def _segment(i, segment, period, frame, hop, seed):
    """Row i's segment as float64 in -1 .. 1: PUSHES x LONGEST samples, more than any plan consumes."""
    rng = np.random.default_rng([seed, i, segment])
    n = np.arange(PUSHES * LONGEST, dtype=np.float64)
    w = 2.0 * np.pi / period
    tone = 0.5 * np.sin(w * n + 0.3 * i) + 0.2 * np.sin(2.0 * w * n + 1.1) + 0.1 * np.sin(3.0 * w * n + 2.3)
    noise = rng.normal(0.0, 1.0, len(n))
    if i % 3 == 1:
        return np.clip(0.2 * noise, -1.0, 1.0)
    v = tone + 0.004 * noise
    if i % 3 == 0:
        v[frame:2 * frame + 2 * hop + 1] = 0.0
    return v


def chunk(i, segment, start, length, npt, period, frame, hop, seed):
    """Samples start .. start + length - 1 of row i's segment, as int16 or float32."""
    v = _segment(i, segment, float(period), int(frame), int(hop), int(seed))[start:start + length]
    assert len(v) == length
    return np.round(12000.0 * v).astype(np.int16) if npt == np.int16 else v.astype(F32)


def x_of(row):
    """The reader's conversion: an int16 s is (float)s / 32767.0f, a float32 as it is."""
    return row.astype(F32) / F32(32767.0) if row.dtype == np.int16 else row.astype(F32)


def pushes(n, lens, end, period, frame, hop, seed):
    """The plan's chunks: per push the rows (int16 and float32 pushes alternate, as (k + seed) mod 2 says), each row reading on in its
    segment from where its last chunk stopped."""
    at, segment = [0] * n, [0] * n
    out = []
    for k, (ls, e) in enumerate(zip(lens, end)):
        npt = (np.int16, F32)[(k + seed) % 2]
        rows = []
        for i in range(n):
            rows.append(chunk(i, segment[i], at[i], ls[i], npt, period, frame, hop, seed))
            at[i] += ls[i]
            if e[i]:
                at[i], segment[i] = 0, segment[i] + 1
        out.append(rows)
    return out


def streams(n, lens, end, period, frame, hop, seed):
    """Per row its segments' whole inputs as the reader sees them (float32), in order: what the statements are taken of."""
    rows = [[[]] for _ in range(n)]
    for chunks, e in zip(pushes(n, lens, end, period, frame, hop, seed), end):
        for i in range(n):
            rows[i][-1].append(x_of(chunks[i]))
            if e[i]:
                rows[i].append([])
    return [[np.concatenate(s) if s else np.zeros(0, F32) for s in row[:-1]] for row in rows]


def lpc_case(g, n):
    """An LPC geometry on n rows: (lens, end, period, frame, hop, seed)."""
    order, nWin, hop = g[0], g[1], g[2]
    seed = 100 * LPC_GEOMETRY.index(g) + n
    return plan(n, nWin - 1, hop, seed) + (lpc_period(g), nWin, hop, seed)


def pitch_case(g, n):
    W, lagMax, hop = g[0], g[2], g[3]
    seed = 1000 + 100 * PITCH_GEOMETRY.index(g) + n
    return plan(n, W + lagMax - 1, hop, seed) + (pitch_period(g), W + lagMax, hop, seed)
