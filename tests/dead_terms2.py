"""Batches for the flat stages' second set of dead terms (option "dead_terms"; csrc/klatt_consts.h, UTT2_*): utterances in which the
nasal pair or parallel resonators 2..6 contribute nothing in every frame, so that their wavefronts run the source stage without the pair,
the final stage without parallel 5 (and 6), the parallel stage without its four resonators (tests/test_dead_terms2_host.py,
tests/test_gpu_dead_terms2.py).  Built with the recipe of tests/dead_terms.py on tests/one_at_a_time.py's noisy base, in 64-lane
wavefronts of at most 192 utterances a corpus, at most 4000 samples and 8 frames each.

    ZEROED[name] = the parameters that are +0.0 in every frame
        nasal    caNP and the turbulence (the body without the pair is built without turbulence)     drops: nasal
        p5       pa5                                                                                  parallel5
        p56      pa5, pa6                                                                             parallel5, parallel56
        p1to4    pa1 .. pa4                                                                           parallel1to4
        all2     all of those and the aspiration                                                      all four
    near misses, which drop none of the four: nasal_alone (caNP alone: the turbulence is present), p6 (pa6 alone), p2to4 (pa1 present)
    CASES (cf1 moves; values altered as in tests/dead_terms.py): negzero -- every one of those gains -0.0, as dead as +0.0;
        cbN0_low (cbN0 = 0.999), pb5_low (pb5 = 0.999), one_frame (pa3 = 1e-300 in ONE frame): present by the rule, nothing of theirs goes;
        asp_far (caNP = 0 with aspirationAmplitude = 1e31, beyond the 1e30 that keeps a noisy list's source, and so N0 / NP, bounded): the pair stays;
        asp_edge (aspirationAmplitude = 1e30, the bound itself): the pair goes

dropped(zeroed sets of the lanes) is the rule: a term goes when it is dead in every lane, among the bodies the engine is built with
(BUILT_MASK = KLATT_DEAD_TERMS of csrc/klatt_systolic.h).
"""
import numpy as np

from tests import dead_terms as dt
from tests import one_at_a_time as oat

SR, LANES = oat.SR, oat.LANES
TERMS2 = ("nasal", "parallel5", "parallel56", "parallel1to4")
PREFIX = "stages_without_"
TURB, ASP, CA_NP, CB_N0, PA1, PA2, PA3, PA4, PA5, PA6, PB5 = 3, 6, 23, 21, 37, 38, 39, 40, 41, 42, 35
assert [oat.NAMES[p] for p in (CA_NP, CB_N0, PA3, PA5, PA6, PB5)] == ["caNP", "cbN0", "pa3", "pa5", "pa6", "pb5"]
BUILT_MASK = 123      # KLATT_DEAD_TERMS: 1 | 2 the first set's bodies; 8 nasal, 16 parallel 5, 32 parallel 5 and 6, 64 parallel 1..4

ZEROED = {
    "nasal": (TURB, CA_NP), "p5": (PA5,), "p56": (PA5, PA6), "p1to4": (PA1, PA2, PA3, PA4),
    "all2": (TURB, ASP, CA_NP, PA1, PA2, PA3, PA4, PA5, PA6),
    "nasal_alone": (CA_NP,), "p6": (PA6,), "p2to4": (PA2, PA3, PA4),
}
DEAD_VARIANTS = ("nasal", "p5", "p56", "p1to4", "all2")
NEAR_VARIANTS = ("nasal_alone", "p6", "p2to4")
PRESENT = dt.PRESENT


def variant(name):
    return "dead2_" + name


for _name, _z in ZEROED.items():
    oat.MORE_VARIANTS[variant(_name)] = (tuple(p for p in range(47) if p not in _z), tuple(_z))


def dropped(zeroed_sets, built=BUILT_MASK):
    """(second set's terms, first set's terms) a wavefront drops whose lanes have these parameters zero in every frame (a lane without a
    frame: all of range(47)): csrc/klatt_batchplan.h's dead2_wave_counts and dead_wave_counts, restated."""
    dead = set(range(47))
    for z in zeroed_sets:
        dead &= set(z)
    no5, no56 = PA5 in dead, PA5 in dead and PA6 in dead
    fin = 2 if (built & 32 and no56) else (1 if (built & 16 and no5) else 0)
    two = []
    if built & 8 and TURB in dead and CA_NP in dead:
        two.append("nasal")
    if fin >= 1:
        two.append("parallel5")
    if fin >= 2:
        two.append("parallel56")
    if built & 64 and all(p in dead for p in (PA1, PA2, PA3, PA4)):
        two.append("parallel1to4")
    one = []
    if built & 1 and PA1 in dead:
        one.append("parallel1")
    body = 2 if (built & 4 and TURB in dead and ASP in dead) else (1 if (built & 2 and TURB in dead) else 0)
    if body >= 1:
        one.append("turbulence")
    if body >= 2:
        one.append("aspiration")
    return tuple(two), tuple(one)


def counts_of(waves):
    """kernelInfo()'s seven counts for wavefronts given as lists of the lanes' zeroed sets."""
    out = {PREFIX + t: 0 for t in TERMS2}
    out.update({"waves_without_" + t: 0 for t in dt.TERMS})
    for lanes in waves:
        two, one = dropped(lanes)
        for t in two:
            out[PREFIX + t] += 1
        for t in one:
            out["waves_without_" + t] += 1
    return out


def zeroed_of(kind):
    return () if kind == PRESENT else ZEROED[kind]


def _seed(*key):
    return oat._seed(78, *key)


def oat_corpus(name):
    """ONE PARAMETER AT A TIME in the variant, three wavefronts: lane l moves parameter ps[l % len(ps)] (every parameter of the variant,
    the columns its dead bodies step over -- cfN0, cbN0, cfNP, cbNP; pf_k, pb_k -- included), then the same as a jump, then `edges` with 64
    timings.  Every lane is of the variant.  Returns (Corpus, per wavefront the lanes' zeroed sets)."""
    v, c = variant(name), oat.Corpus(variant(name))
    ps = oat.params(v)
    for wi, manner in enumerate(oat.MANNERS):
        for lane in range(LANES):
            p = ps[(lane + 23 * wi) % len(ps)] if manner == "edges" else ps[lane % len(ps)]
            c.add(oat.case(p, manner, v, (37 * lane + 11) % LANES if manner == "edges" else 0), _seed(1, wi, lane), p, manner, "pure " + name, lane)
    assert len(ps) <= LANES
    return c.finish(), [[ZEROED[name]] * LANES] * 3


def intruder_corpus(name):
    """63 lanes of the variant (move of cf1) and one, lane 37, of the unaltered base: everything present, the general bodies; then a whole
    wavefront of the variant beside it."""
    v, c = variant(name), oat.Corpus(variant(name))
    for lane in range(LANES):
        c.add(oat.case(oat.USUAL, "move", "noisy" if lane == 37 else v), _seed(2, lane), oat.USUAL, "move", "intruder", lane)
    for lane in range(LANES):
        c.add(oat.case(oat.USUAL, "jump", v), _seed(3, lane), oat.USUAL, "jump", "pure", lane)
    return c.finish(), [[() if lane == 37 else ZEROED[name] for lane in range(LANES)], [ZEROED[name]] * LANES]


# TWO at a time (tests/dead_terms.py, pairs): a stepped-over column q moving together with each parameter p of a kind BEHIND q's in the same
# stage's part of a track.  Kinds: N0 0 (two entries), NP 1 | 20..23 behind them in flat S0; parallel 5 12, parallel 6 13 | 15, 16 behind in
# the final stage; parallel 1..4 8..11 | 17 behind in the parallel stage.
def pairs(name):
    v = variant(name)
    z = ZEROED[name]
    out = []
    if CA_NP in z and TURB in z:
        out += [(q, p) for q in (13, 21, 14, 22) for p in (1, 2, 5, 6, 44) if p in oat.params(v)]
    if PA5 in z:
        qs = (29, 35) + ((30, 36) if PA6 in z else ())
        out += [(q, p) for q in qs for p in (30, 36, 42, 43, 45) if p in oat.params(v) and p not in qs]
    if all(p in z for p in (PA1, PA2, PA3, PA4)):
        out += [(q, p) for q in (25, 26, 27, 28, 31, 32, 33, 34) for p in (24, 44)]
    return out


def pair_case(name, q, p, manner, edge=0):
    v = variant(name)
    b, cq = oat.base(v), oat.changed(q, v)[q]
    out = []
    for fr, m, f in oat.case(p, manner, v, edge):
        if fr is not None and not np.array_equal(fr, b):
            fr = fr.copy()
            fr[q] = cq
        out.append((fr, m, f))
    return out


def pairs_corpus():
    """all2: every pair of its three lightened bodies, a wavefront moving and one jumping; p5: the final stage without parallel 5 alone,
    one wavefront, move and jump in turn."""
    c, waves = oat.Corpus("pairs2"), []
    ps = pairs("all2")
    assert 40 <= len(ps) <= LANES
    for wi, manner in enumerate(("move", "jump")):
        for lane in range(LANES):
            q, p = ps[lane % len(ps)]
            c.add(pair_case("all2", q, p, manner), _seed(4, wi, lane), p, manner, "all2: with %s" % oat.NAMES[q], lane)
        waves.append([ZEROED["all2"]] * LANES)
    ps = pairs("p5")
    for lane in range(LANES):
        q, p = ps[lane % len(ps)]
        c.add(pair_case("p5", q, p, "move" if (lane // len(ps)) % 2 == 0 else "jump"), _seed(5, lane), p, "move", "p5: with %s" % oat.NAMES[q], lane)
    waves.append([ZEROED["p5"]] * LANES)
    return c.finish(), waves


# MIXED SETS: wavefronts whose lanes have different dead sets drop only what is dead in every lane
MIXED = ("nasal|all2", "p5|p56", "p1to4|all2", "nasal|p56", "p6|all2", "nasal_alone|nasal", "all2@present0", "all2@present63", "p2to4|p1to4")


def _mixed_lanes(comp):
    if "|" in comp:
        a, b = comp.split("|")
        return [a if lane % 2 == 0 else b for lane in range(LANES)]
    return ["present" if lane == int(comp.split("@present")[1]) else "all2" for lane in range(LANES)]


def mixed_corpora():
    """MIXED in corpora of at most 192 utterances: [(Corpus, per wavefront the lanes' zeroed sets)].  Lane kinds: a variant, the unaltered
    base (everything present)."""
    out = []
    for at in range(0, len(MIXED), 3):
        c, waves = oat.Corpus("mixed sets 2"), []
        for ci, comp in enumerate(MIXED[at:at + 3]):
            kinds = _mixed_lanes(comp)
            # (pf2 moves: a kind of the parallel stage, which p1to4 steps over and the others read)
            for lane, kind in enumerate(kinds):
                frames = oat.case(26 if ci % 2 else oat.USUAL, "move", "noisy" if kind == "present" else variant(kind))
                c.add(frames, _seed(6, at + ci, lane), 26 if ci % 2 else oat.USUAL, "move", comp, lane)
            waves.append([() if k == "present" else ZEROED[k] for k in kinds])
        out.append((c.finish(), waves))
    return out


# cf1 moving with altered values (tests/dead_terms.py, frames_of): the edges of the rules
ALL2 = {p: 0.0 for p in ZEROED["all2"]}


def _with(d, more):
    out = dict(d)
    out.update(more)
    return out


CASES = {
    "negzero": (_with(ALL2, {p: -0.0 for p in (CA_NP, PA1, PA2, PA3, PA4, PA5, PA6)}), {}, ZEROED["all2"]),
    "cbN0_low": (_with(ALL2, {CB_N0: 0.999}), {}, tuple(p for p in ZEROED["all2"] if p != CA_NP)),
    "pb5_low": (_with(ALL2, {PB5: 0.999}), {}, tuple(p for p in ZEROED["all2"] if p != PA5)),
    "one_frame": (ALL2, {PA3: 1e-300}, tuple(p for p in ZEROED["all2"] if p != PA3)),
    "asp_far": (_with(ALL2, {ASP: 1e31}), {}, tuple(p for p in ZEROED["all2"] if p not in (ASP, CA_NP))),
    "asp_edge": (_with(ALL2, {ASP: 1e30}), {}, tuple(p for p in ZEROED["all2"] if p != ASP)),
}


def frames_of(case, manner, edge=0):
    everywhere, second, _ = CASES[case]
    out, seen = [], 0
    for fr, m, f in oat.case(oat.USUAL, manner, "noisy", edge):
        if fr is not None:
            fr = fr.copy()
            for p, v in everywhere.items():
                fr[p] = v
            if seen == 1:
                for p, v in second.items():
                    fr[p] = v
            seen += 1
        out.append((fr, m, f))
    return out


def case_corpus(case):
    """pure (move), pure (jump) and ragged (edges) wavefronts of the case; the lanes' dead parameters are CASES[case][2] (what the rule makes of them)."""
    c, ci = oat.Corpus("noisy"), list(CASES).index(case)
    for wi, manner in enumerate(oat.MANNERS):
        for lane in range(LANES):
            c.add(frames_of(case, manner, (37 * lane + 11) % LANES if manner == "edges" else 0), _seed(7, ci, wi, lane), oat.USUAL, manner, case, lane)
    return c.finish(), [[CASES[case][2]] * LANES] * 3


def sparse_corpus(kinds):
    c = oat.Corpus("noisy")
    for k, kind in enumerate(kinds):
        c.add(oat.case(oat.USUAL, "move" if k % 2 == 0 else "jump", "noisy" if kind == PRESENT else variant(kind)), _seed(8, k), oat.USUAL, "move", "sparse", k)
    return c.finish(whole_wavefronts=False), [[zeroed_of(k) for k in kinds]]


CORPORA = ["oat:" + n for n in DEAD_VARIANTS + NEAR_VARIANTS] + ["intruder:" + n for n in ("all2", "nasal", "p5")] + ["pairs"] + \
          ["mixed:%d" % i for i in range(3)] + ["case:" + n for n in CASES]


def build(name):
    """(Corpus, per wavefront the lanes' zeroed sets) of CORPORA's name."""
    kind, _, arg = name.partition(":")
    if kind == "oat":
        return oat_corpus(arg)
    if kind == "intruder":
        return intruder_corpus(arg)
    if kind == "pairs":
        return pairs_corpus()
    if kind == "mixed":
        return mixed_corpora()[int(arg)]
    return case_corpus(arg)
