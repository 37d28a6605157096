"""What tests/test_export_rates_host.py and tests/test_gpu_export_rates.py share: the batch that holds the response, stems and source
exports (csrc/klatt_response.h, klatt_stems.h, klatt_source.h) at every sample rate, in two parts whose frequencies and bandwidths are
fractions of the rate.  No GPU.

coefficient_parts (csrc/klatt_device.h) picks between three bodies by wave-uniform votes: every lane's exp argument unreduced (k = 0)
and every cos argument in quadrant 0; the same with every cos argument in quadrant -1; else the general fast_exp / fast_cos.

  edge part   edge_batch of tests/test_gpu_rates.py, 96 utterances drawn from default_rng(sr): every class of exp and cos, the margins,
              formants above Nyquist and negative, bandwidths of 0, N0 at 0 Hz, two utterances beyond the documented range.  Its
              wavefronts are mixed: the general body, and the votes that fail.
  pure part   PURE_ROWS deterministic utterances (the same fractions of the rate at every rate) that make the votes SUCCEED, and
              fail by one lane.  In klatt_stems a wavefront is 64 export rows, longest first (a stable sort); the rows' lengths do not
              increase with their number, so an export of rows 0 .. PURE_ROWS - 1 has
                rows   0 ..  63   64 *low* utterances: all 14 frequencies in (0, 0.124 sr), all bandwidths in (0, 0.109 sr)
                rows  64 .. 127   64 *upper* utterances: all 14 frequencies in (0.126 sr, 0.374 sr), the same bandwidths
                rows 128 .. 191   63 low ones and, at lane ODD_LANE, a copy of its left neighbour with cf3 of its second frame at
                                  0.12525 sr (quadrant -1 in one lane)
                rows 192 .. 196   a ragged wavefront of four low ones and a copy of row 193 with cb2 of its second frame at 0.1104 sr
                                  (k = -1 in one lane)
              In klatt_response a wavefront is four consecutive steps of one utterance by its 14 resonators: every stretch of a low or
              upper utterance but its sample 0 (cur(0) is the all-zero frame) is class-pure, and the odd ones break four steps' votes
              from inside.  Rows 2, 66 and 130 speak the frame list of the row before them under another seed.
              Every utterance: frame A (a fade of 40 out of silence, held to sample 120), frame B (a fade of 150 that all rows of the
              batch walk together -- the stems kernel's branch-free fade blocks -- then held), and for two rows in three a frame C whose
              fade length differs from row to row (lanes fading beside steady ones: the general step); the last hold sets the length,
              1500 samples down to 520.  Even rows have no noise gain, odd rows have turbulence, aspiration and frication.  No vibrato
              (the edge part has it)."""
import functools

import numpy as np

from tests.test_gpu_rates import RATES, edge_batch      # (numpy, the oracle and the scenarios only: nothing there needs a GPU to import)

__all__ = ["RATES", "edge_batch", "edge_part", "pure_part", "parts", "restated_subset", "bins", "classes", "expand"]

LOG2E = 1.4426950408889634074          # klatt::kLog2e
TWO_OVER_PI = 0.63661977236758134308   # klatt::kTwoOverPi
RES_F = (13, 14, 12, 11, 10, 9, 8, 7, 25, 26, 27, 28, 29, 30)      # N0, NP, c6 .. c1, p1 .. p6 (csrc/klatt_response.h: kRespResF / kRespResB)
RES_B = (21, 22, 20, 19, 18, 17, 16, 15, 31, 32, 33, 34, 35, 36)
EDGE_ROWS = 96
LOW, UPPER, THIRD, RAGGED = 0, 64, 128, 192          # the first row of each wavefront of the stems export of the pure part
ODD_LANE = 37
ODD_F, ODD_BW = THIRD + ODD_LANE, RAGGED + 2          # the two odd ones out; each is a copy of the row before it
PURE_ROWS = RAGGED + 5
SHARED = (LOW + 2, UPPER + 2, THIRD + 2)             # rows that speak the list of the (noisy) row before them
ODD_F_FRACTION, ODD_BW_FRACTION = 0.12525, 0.1104
RESTATED_MOST = 60000
BIN_FRACTIONS = (0.0, 0.0198, 0.0454, 0.1343, 0.5)


def bins(sr):
    """Five bins (an odd count: float32 blocks that are not 16-byte aligned), the fractions of 22 050 Hz's 0, 437.5, 1000, 2961.3, Nyquist."""
    return np.array(BIN_FRACTIONS) * sr


def classes(f, bw, sr):
    """-> (k, n): the reduction class of exp's argument (-pi / sr) bw and the quadrant of cos's argument (2 pi / sr) (-f), formed as
    coefficient_parts forms them, by the predicates of klatt_math.h as tests/test_device_math.py states them."""
    ex = (-np.pi / sr) * np.asarray(bw, dtype=np.float64)
    th = ((np.pi * 2) / sr) * -np.asarray(f, dtype=np.float64)
    return np.rint(ex * LOG2E), np.rint(th * TWO_OVER_PI)


def in_range(frames, sr):
    """Per frame: all 28 frequencies and bandwidths inside the range in which the host states the device's bits (|pi bw / sr| <= 700,
    |2 pi f / sr| <= 1e4)."""
    f, bw = frames[:, list(RES_F)], frames[:, list(RES_B)]
    return (np.abs(np.pi * bw / sr) <= 700.0).all(axis=1) & (np.abs(2 * np.pi * f / sr) <= 1.0e4).all(axis=1)


def _frame(rng, sr, lo, hi, noisy):
    f = np.zeros(47)
    f[0] = rng.uniform(80.0, 300.0); f[46] = f[0] * rng.uniform(0.8, 1.25)
    f[4] = rng.uniform(0.3, 0.7); f[5] = rng.uniform(0.4, 1.0)
    noise = rng.uniform(0.0, 1.0, 3)                                   # (drawn for every row: a row's frequencies do not depend on its noise)
    if noisy:
        f[3], f[6], f[24] = 0.3 * noise[0], 0.05 + 0.4 * noise[1], 0.1 + 0.7 * noise[2]
    f[7:15] = rng.uniform(lo, hi, 8) * sr                              # cf1 .. cf6, cfN0 (never 0: the anti-resonator divides), cfNP
    f[15:23] = rng.uniform(0.02, 0.108, 8) * sr
    f[23] = rng.uniform(0.0, 0.3)
    f[25:31] = rng.uniform(lo, hi, 6) * sr
    f[31:37] = rng.uniform(0.02, 0.108, 6) * sr
    f[37:43] = rng.uniform(0.0, 1.0, 6)
    f[43] = rng.uniform(0.0, 1.0); f[44] = rng.uniform(0.3, 1.5); f[45] = rng.uniform(0.2, 1.0)
    return f


def _length(mins, fades):
    m, f = np.asarray(mins, dtype=np.int64), np.maximum(np.asarray(fades, dtype=np.int64), 1)
    return int((np.maximum(m, f + 1) + 1).sum())


@functools.lru_cache(maxsize=None)
def pure_part(sr):
    """-> dict(lists: the distinct frame lists as a batch dict, list_of [PURE_ROWS], seeds [PURE_ROWS], kind: 'low' / 'upper' /
    'odd f' / 'odd bw' per row, original: {odd row: the row it copies}, odd: {odd row: (frame of its list, parameter)})."""
    rng = np.random.default_rng(7)                                     # the same fractions of the rate at every rate
    frames, mins, fades, start, list_of, kind = [], [], [], [0], [], []
    lists = {}                                                         # row -> its list
    for row in range(PURE_ROWS):
        upper = UPPER <= row < THIRD
        lo, hi = (0.1265, 0.3735) if upper else (0.002, 0.1235)
        want = 1500 - 5 * row
        own = [_frame(rng, sr, lo, hi, noisy=row % 2 == 1) for _ in range(3)]
        if row in SHARED:
            list_of.append(lists[row - 1]); kind.append(kind[-1])
            continue
        if row in (ODD_F, ODD_BW):
            a, e = start[lists[row - 1]], start[lists[row - 1] + 1]
            fr = [x.copy() for x in frames[a:e]]
            if row == ODD_F:
                fr[1][9] = ODD_F_FRACTION * sr                          # cf3
            else:
                fr[1][16] = ODD_BW_FRACTION * sr                        # cb2
            m, fd = mins[a:e], fades[a:e]
            kind.append("odd f" if row == ODD_F else "odd bw")
        else:
            if row % 3 != 0 or row + 1 in (ODD_F, ODD_BW):             # (an odd one's list has a frame after the changed one)
                fr, m, fd = own, [120, 200, 0], [40, 150, 30 + (row * 7) % 90]
            else:
                fr, m, fd = own[:2], [120, 0], [40, 150]
            m[-1] = want - _length(m[:-1], fd[:-1]) - 1                # (a copy is as long as the row it copies)
            assert _length(m, fd) == want and all(hold >= fade + 16 for hold, fade in zip(m, fd))
            kind.append("upper" if upper else "low")
        lists[row] = len(start) - 1
        list_of.append(lists[row])
        frames += fr; mins += list(m); fades += list(fd); start.append(len(mins))
    n = len(mins)
    batch = dict(frames=np.array(frames), min=np.array(mins, np.uint32), fade=np.array(fades, np.uint32), index=np.full(n, -1, np.int32),
                 isnull=np.zeros(n, np.uint8), frame_start=np.array(start, np.int64))
    return dict(lists=batch, list_of=np.array(list_of, np.int64), seeds=np.arange(1000, 1000 + PURE_ROWS, dtype=np.uint32) - np.isin(np.arange(PURE_ROWS), (ODD_F, ODD_BW)),
                kind=kind, original={ODD_F: ODD_F - 1, ODD_BW: ODD_BW - 1}, odd={ODD_F: (1, 9), ODD_BW: (1, 16)})


@functools.lru_cache(maxsize=None)
def edge_part(sr):
    return edge_batch(np.random.default_rng(sr), sr, EDGE_ROWS)


def expand(lists, list_of, seeds):
    """Frame lists and the list of every utterance -> the batch dict of tests/scenarios.py, a list of its own per utterance."""
    fs = lists["frame_start"]
    pick = np.concatenate([np.arange(fs[l], fs[l + 1]) for l in list_of]) if len(list_of) else np.zeros(0, np.int64)
    start = np.concatenate([[0], np.cumsum([fs[l + 1] - fs[l] for l in list_of])]).astype(np.int64)
    out = {k: np.ascontiguousarray(lists[k][pick]) for k in ("frames", "min", "fade", "index", "isnull")}
    out["frame_start"] = start
    out["seeds"] = np.asarray(seeds, dtype=np.uint32)
    return out


@functools.lru_cache(maxsize=None)
def parts(sr):
    """Both parts as one batch, the pure part first: -> dict(lists, list_of, seeds: what setUtterancesShared takes; batch: the same
    utterances with a list each, what the oracle and the restatements take; kind per utterance ('edge' for the edge part); pure, edge:
    the utterance numbers of the parts)."""
    p, e = pure_part(sr), edge_part(sr)
    pl = p["lists"]
    n_lists, n_frames = len(pl["frame_start"]) - 1, len(pl["min"])
    lists = {k: np.concatenate([pl[k], e[k]]) for k in ("frames", "min", "fade", "index", "isnull")}
    lists["frame_start"] = np.concatenate([pl["frame_start"], e["frame_start"][1:] + n_frames]).astype(np.int64)
    list_of = np.concatenate([p["list_of"], n_lists + np.arange(EDGE_ROWS)]).astype(np.int64)
    seeds = np.concatenate([p["seeds"], e["seeds"]]).astype(np.uint32)
    return dict(lists=lists, list_of=list_of, seeds=seeds, batch=expand(lists, list_of, seeds), kind=p["kind"] + ["edge"] * EDGE_ROWS,
                pure=np.arange(PURE_ROWS), edge=PURE_ROWS + np.arange(EDGE_ROWS))


def lengths(batch):
    fs = batch["frame_start"]
    per = np.maximum(batch["min"].astype(np.int64), np.maximum(batch["fade"].astype(np.int64), 1) + 1) + 1
    c = np.concatenate([[0], np.cumsum(per)])
    return c[fs[1:]] - c[fs[:-1]]


def utterance_frames(batch, u):
    """The real frames of utterance u."""
    a, e = int(batch["frame_start"][u]), int(batch["frame_start"][u + 1])
    return batch["frames"][a:e][~batch["isnull"][a:e].astype(bool)]


# Utterances left out of the subset by number, per rate: the source comparison has a tie there (tests/test_export_rates_host.py).
TIED = {}


@functools.lru_cache(maxsize=None)
def restated_subset(sr):
    """The utterances, in ascending number, that the plain-Python restatements (`stems`, `source`) walk; together they stay under
    RESTATED_MOST samples.  First the pure part's witnesses (a low row and the row that shares its list, an upper row, both odd ones
    with the rows they copy); then the first edge utterance whose in-range frames reach exp's k = -2 and the first that reaches cos's
    quadrant -4; then the edge utterances in ascending number while the total stays under RESTATED_MOST.  Only utterances whose
    frames are all inside the documented range: those are compared bit for bit."""
    p = parts(sr)
    b, lens = p["batch"], lengths(p["batch"])
    chosen = [LOW + 1, LOW + 2, UPPER, ODD_F - 1, ODD_F, ODD_BW - 1, ODD_BW]
    edge = [int(u) for u in p["edge"] if in_range(utterance_frames(b, u), sr).all() and int(u) not in TIED.get(sr, ())]

    def reaches(u, which, value):
        fr = utterance_frames(b, u)
        return len(fr) > 0 and bool((classes(fr[:, list(RES_F)], fr[:, list(RES_B)], sr)[which] == value).any())

    for which, value in ((0, -2), (1, -4)):
        chosen.append(next(u for u in edge if reaches(u, which, value) and lens[u] < 8000))
    total = int(lens[sorted(set(chosen))].sum())
    for u in edge:
        if u not in chosen and total + lens[u] < RESTATED_MOST:
            chosen.append(u); total += int(lens[u])
    chosen = sorted(set(chosen))
    assert int(lens[chosen].sum()) < RESTATED_MOST
    return chosen
