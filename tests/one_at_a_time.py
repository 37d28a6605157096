"""One-parameter-at-a-time batches: utterances in which exactly ONE of the 47 parameters differs between two frames, so that a
failure names a parameter and a path (tests/test_one_at_a_time_host.py, tests/test_gpu_one_at_a_time.py).

A base frame B in which every branch contributes (voicing, vibrato, turbulence, aspiration, both nasal resonators, frication
through all six parallel resonators and the bypass), and changed(p): B with parameter p alone altered.  Three MANNERS of
putting the change into a frame list of (frame | None, minSamples, fadeSamples), Z a NULL frame, B' = changed(p):
    move    (B,600,200) (B',600,173) (B,400,100) (Z,100,100)    p moves inside two fades: it is in those fades' masks
    jump    (B,500,120) (Z,300,150) (B',700,300) (Z,100,100)    p never moves inside a fade: it jumps on the first row of the
                                                                fade out of silence, whose mask holds the gain alone
    edges   move with fade lengths in turn from EDGE_FADES and the first frame lengthened by 0..63 samples: fades start and end
            on every residue of the 16-sample hand-over and the 32-sample PCM tile
Three VARIANTS of the base: noisy (all 47 parameters), quiet (no turbulence, aspiration, frication: the parameters that still reach
the output), quiet_nasal_free (caNP = 0 as well).
Three COMPOSITIONS of a 64-lane wavefront, written for "sort" = 0 (lanes packed densely in the given order):
    pure      64 utterances of one case, seeds of their own: time-aligned lanes
    intruder  63 utterances that move cf1 (a usual kind in every flat stage) and one of case p at lane p % 64
    ragged    64 different edges cases: no two lanes share their timing
"""
import numpy as np

from tests import oracle
from tests.test_track_planning import PAIRS, RES_B, RES_F

SR = 22050
LANES = 64
NAMES = (["voicePitch", "vibratoPitchOffset", "vibratoSpeed", "voiceTurbulenceAmplitude", "glottalOpenQuotient", "voiceAmplitude",
          "aspirationAmplitude"] + ["cf%d" % i for i in range(1, 7)] + ["cfN0", "cfNP"] + ["cb%d" % i for i in range(1, 7)] +
         ["cbN0", "cbNP", "caNP", "fricationAmplitude"] + ["pf%d" % i for i in range(1, 7)] + ["pb%d" % i for i in range(1, 7)] +
         ["pa%d" % i for i in range(1, 7)] + ["parallelBypass", "preFormantGain", "outputGain", "endVoicePitch"])
assert len(NAMES) == 47

BASE = np.zeros(47)
BASE[0], BASE[46] = 120.0, 110.0
BASE[1], BASE[2], BASE[3], BASE[4], BASE[5], BASE[6] = 0.1, 5.0, 0.2, 0.5, 1.0, 0.2
BASE[7:13] = (700, 1200, 2600, 3300, 3750, 4900)
BASE[13], BASE[14] = 450, 270
BASE[15:21] = (90, 100, 150, 250, 200, 1000)
BASE[21], BASE[22], BASE[23], BASE[24] = 100, 100, 0.5, 0.3
BASE[25:31] = (720, 1250, 2500, 3400, 3800, 4800)
BASE[31:37] = (80, 110, 160, 240, 210, 900)
BASE[37:43] = (0.5, 0.45, 0.4, 0.35, 0.3, 0.25)
BASE[43], BASE[44], BASE[45] = 0.3, 1.0, 0.6
BASE.setflags(write=False)

FREQS = tuple(range(7, 15)) + tuple(range(25, 31))
BANDWIDTHS = tuple(range(15, 23)) + tuple(range(31, 37))
NOISE_GAINS = (3, 6, 24)
QUIET_PARAMS = (0, 1, 2, 4, 5) + tuple(range(7, 24)) + (44, 45, 46)
# variant -> (the parameters used, those set to 0 in every frame)
# (tests/test_one_at_a_time_host.py holds every case to its floor of audibility: one change rule serves all three variants.
# glottalOpenQuotient gates the turbulence only, so in the quiet variants it moves without being heard: kept, as a kind that moves)
VARIANTS = {
    "noisy": (tuple(range(47)), ()),
    "quiet": (QUIET_PARAMS, NOISE_GAINS),
    "quiet_nasal_free": (tuple(p for p in QUIET_PARAMS if p not in (13, 14, 21, 22, 23)), NOISE_GAINS + (23,)),
}
# variants of other modules, same form (tests/dead_terms.py: the dead variants).  A table of its own: list(VARIANTS) parametrises tests.
MORE_VARIANTS = {}
MANNERS = ("move", "jump", "edges")
EDGE_FADES = (1, 2, 15, 16, 17, 31, 32, 33)
USUAL = 7       # cf1: the parameter the intruder composition's 63 other lanes move


def _spec(variant):
    return VARIANTS[variant] if variant in VARIANTS else MORE_VARIANTS[variant]


def params(variant):
    return _spec(variant)[0]


def base(variant="noisy"):
    f = BASE.copy()
    f[list(_spec(variant)[1])] = 0.0
    return f


def changed(p, variant="noisy"):
    """base(variant) with parameter p alone altered."""
    f = base(variant)
    assert p in params(variant), (p, variant)
    if p in FREQS or p in BANDWIDTHS:
        f[p] *= 1.15
    elif p in (0, 46):
        f[p] *= 1.2
    elif p == 1:
        f[p] = 0.25
    elif p == 2:
        f[p] = 7.0
    elif p == 4:
        f[p] = 0.7
    elif p == 43:
        f[p] = 0.6
    else:
        f[p] *= 0.6
    assert np.count_nonzero(f != base(variant)) == 1
    return f


def case(p, manner, variant="noisy", edge=0, unchanged=False):
    """The frame list [(frame | None, minSamples, fadeSamples)] of parameter p in a manner; edge (edges only): 0..63, the first
    frame's extra samples and where in EDGE_FADES its fades start.  unchanged: the same list with B' = B."""
    b = base(variant)
    c = b if unchanged else changed(p, variant)
    if manner == "jump":
        return [(b, 500, 120), (None, 300, 150), (c, 700, 300), (None, 100, 100)]
    out = [(b, 600, 200), (c, 600, 173), (b, 400, 100), (None, 100, 100)]
    if manner == "edges":
        assert 0 <= edge < LANES
        out = [(fr, m + (edge if j == 0 else 0), EDGE_FADES[(edge + j) % len(EDGE_FADES)]) for j, (fr, m, _) in enumerate(out)]
    else:
        assert manner == "move", manner
    return out


def kind_bits(p):
    """The entry kinds parameter p belongs to, as bits of a track mask (tests/test_track_planning.py's table): none for the pitches,
    two for preFormantGain."""
    m = 0
    for r in range(14):
        if p in (RES_F[r], RES_B[r]):
            m |= 1 << r
    for e, pair in enumerate(PAIRS):
        if p in pair:
            m |= 1 << (14 + e)
    return m


def one_per_kind(variant="noisy"):
    """One parameter of the variant per entry kind it reaches (frequencies and bandwidths, first and second members of the pairs in
    turn), then the two pitches."""
    out, seen = [], 0
    for i, kinds in enumerate([(RES_F[r], RES_B[r]) for r in range(14)] + [tuple(x for x in pair if x >= 0) for pair in PAIRS]):
        cand = [p for p in kinds if p in params(variant) and not (kind_bits(p) & seen)]
        if cand:
            out.append(cand[i % len(cand)])
            seen |= kind_bits(out[-1])
    return out + [0, 46]


class Corpus:
    """Utterances as one batch (the dict tests/oracle.batch_synthesize and BatchPlayer.setUtterances take) and, per utterance,
    what it is: .what[u] = (parameter, manner, composition, wavefront, lane)."""

    def __init__(self, variant):
        self.variant, self.what, self.cases, self.seeds = variant, [], [], []

    def add(self, frames, seed, p, manner, composition, lane):
        wave = len(self.what) // LANES
        assert lane == len(self.what) % LANES
        self.what.append((p, manner, composition, wave, lane))
        self.cases.append(frames); self.seeds.append(seed)

    def finish(self, whole_wavefronts=True):
        assert len(self.what) % LANES == 0 or not whole_wavefronts
        z = np.zeros(47)
        flat = [x for c in self.cases for x in c]
        self.batch = dict(frames=np.array([z if fr is None else fr for fr, _, _ in flat]), min=np.array([m for _, m, _ in flat], np.uint32),
                          fade=np.array([f for _, _, f in flat], np.uint32), index=np.full(len(flat), -1, np.int32),
                          isnull=np.array([fr is None for fr, _, _ in flat], np.uint8),
                          frame_start=np.concatenate([[0], np.cumsum([len(c) for c in self.cases])]).astype(np.int64),
                          seeds=np.array(self.seeds, np.uint32))
        return self

    def __len__(self):
        return len(self.what)

    def tiled(self, k):
        """This corpus k times in order (whole wavefronts: under "sort" = 0 every wavefront keeps its composition) -- a batch large enough
        for the flat launch with two workgroups per CU; .what counts the wavefronts on.  The oracle synthesizes nothing twice."""
        assert len(self) % LANES == 0
        c = Corpus(self.variant)
        for _ in range(k):
            for (p, manner, composition, _, lane), frames, seed in zip(self.what, self.cases, self.seeds):
                c.add(frames, seed, p, manner, composition, lane)
        return c.finish()

    def oracle(self, threads=8):
        """(pcm, start, total) of tests/oracle.batch_synthesize; every distinct (frame list, seed) is synthesized once."""
        b, first, of = self.batch, {}, []
        for u in range(len(self)):
            a, e = b["frame_start"][u], b["frame_start"][u + 1]
            key = (b["frames"][a:e].tobytes(), b["min"][a:e].tobytes(), b["fade"][a:e].tobytes(), b["isnull"][a:e].tobytes(), int(b["seeds"][u]))
            of.append(first.setdefault(key, u))
        uniq = sorted(set(of))
        rows = np.concatenate([np.arange(b["frame_start"][u], b["frame_start"][u + 1]) for u in uniq])
        sub = {k: b[k][rows] for k in ("frames", "min", "fade", "index", "isnull")}
        sub["frame_start"] = np.concatenate([[0], np.cumsum([b["frame_start"][u + 1] - b["frame_start"][u] for u in uniq])]).astype(np.int64)
        sub["seeds"] = b["seeds"][uniq]
        pcm, start, _ = oracle.batch_synthesize(SR, sub, threads=threads)
        at = {u: i for i, u in enumerate(uniq)}
        lens = np.array([start[at[v] + 1] - start[at[v]] for v in of], np.int64)
        full_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        full = np.empty(int(full_start[-1]), np.int16)
        for u, v in enumerate(of):
            full[full_start[u]:full_start[u + 1]] = pcm[start[at[v]]:start[at[v] + 1]]
        return full, full_start, int(full_start[-1])

    def describe(self, u):
        p, manner, composition, wave, lane = self.what[u]
        return "%s: parameter %d (%s), manner %s, composition %s, wavefront %d lane %d (utterance %d)" % (
            self.variant, p, NAMES[p], manner, composition, wave, lane, u)

    def first_difference(self, got, want, start, tolerance=0):
        """None, or a message that names the first utterance in which got and want differ by more than `tolerance` and where."""
        d = np.abs(got.astype(np.int32) - want.astype(np.int32)) > tolerance
        if not d.any():
            return None
        i = int(np.argmax(d))
        u = int(np.searchsorted(start, i, side="right")) - 1
        a, e = int(start[u]), int(start[u + 1])
        return "%s: first difference at sample %d (%d against %d), %d samples of it differ, %d utterances of %d" % (
            self.describe(u), i - a, int(got[i]), int(want[i]), int(np.count_nonzero(d[a:e])),
            int(np.count_nonzero(np.add.reduceat(d, start[:-1]) > 0)), len(self))


def _seed(*key):
    """a seed of its own for every (composition, manner, parameter, lane)"""
    h = 0x9E3779B9
    for k in key:
        h = ((h ^ int(k)) * 0x85EBCA6B + 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 15
    return h


def add_pure(c, p, manner):
    for lane in range(LANES):
        c.add(case(p, manner, c.variant), _seed(1, MANNERS.index(manner), p, lane), p, manner, "pure", lane)


def add_intruder(c, p, manner):
    """(the 63 other lanes carry the same seeds in every wavefront of a manner: Corpus.oracle synthesizes them once)"""
    for lane in range(LANES):
        if lane == p % LANES:
            c.add(case(p, manner, c.variant), _seed(3, MANNERS.index(manner), p), p, manner, "intruder", lane)
        else:
            c.add(case(USUAL, manner, c.variant), _seed(2, MANNERS.index(manner), lane), USUAL, manner, "intruder", lane)


def add_ragged(c, turn):
    """64 edges cases, every lane with an offset of its own; `turn` shifts which parameter meets which offset."""
    ps = params(c.variant)
    for lane in range(LANES):
        p, edge = ps[(lane + 17 * turn) % len(ps)], (37 * lane + 11 * turn) % LANES
        c.add(case(p, "edges", c.variant, edge), _seed(4, turn, lane), p, "edges", "ragged", lane)


def batch_corpus(variant):
    """Every (parameter, manner) of the variant in at least one composition: `move` pure and as an intruder for every parameter,
    `jump` as an intruder for every parameter and pure for one parameter per entry kind, `edges` in ragged wavefronts (every
    parameter at least twice)."""
    c = Corpus(variant)
    for p in params(variant):
        add_pure(c, p, "move")
    for p in one_per_kind(variant):
        add_pure(c, p, "jump")
    for manner in ("move", "jump"):
        for p in params(variant):
            add_intruder(c, p, manner)
    for turn in range(-(-2 * len(params(variant)) // LANES)):
        add_ragged(c, turn)
    return c.finish()


def live_corpus(variant="noisy"):
    """One move, one jump and one edges case per entry kind, and of the two pitches: what the live handles are given (one handle per
    utterance, composition "live"), as a batch as well."""
    c = Corpus(variant)
    for i, p in enumerate(one_per_kind(variant)):
        for manner in MANNERS:
            c.add(case(p, manner, variant, edge=(5 * i + 3) % LANES), _seed(5, MANNERS.index(manner), p), p, manner, "live", len(c) % LANES)
    return c.finish(whole_wavefronts=False)
