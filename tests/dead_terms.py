"""Batches for the flat stages' dead terms (option "dead_terms"): utterances in which voice turbulence, aspiration or the first
parallel resonator contribute nothing in every frame, so that their wavefronts run stage bodies without those terms
(tests/test_dead_terms_host.py, tests/test_gpu_dead_terms.py).

The base frame and the frame lists are those of tests/one_at_a_time.py -- `move`, `jump` and `edges` of cf1, a kind that moves in
the fades, so that rows are loaded past the kinds the bodies leave out -- with the frames ALTERED for a case:

    dead cases         p1          pa1 = 0
                       turb        voiceTurbulenceAmplitude = 0
                       turb_asp    voiceTurbulenceAmplitude = aspirationAmplitude = 0
                       all         all three
    edge cases         pa1_negzero   pa1 = -0.0: zero of either sign is dead (the term is +-0 onto +0)
                       voiceless     turb_asp with voiceAmplitude = 0: voice * 0 is -0 for half the glottal cycle, the sum 0.0 + -0 must stay +0
    near misses        pb1_low       pa1 = 0 with pb1 = 0.999: the resonator might not stay finite by the rule, so it is present
                       asp_negzero   turbulence 0, aspiration -0.0: not +0.0 bit for bit, the generator stays
                       one_frame     pa1 = 0 except 1e-300 in ONE frame in the middle of the list

EXPECT[case] = the terms whose bodies a wavefront of the case alone must drop, of ("parallel1", "turbulence", "aspiration").
Compositions of a 64-lane wavefront for "sort" = 0 (lanes packed densely in the given order), as in tests/one_at_a_time.py:
    pure      64 utterances of the case (move), seeds of their own
    intruder  63 utterances of the case and one of the unaltered base, in which every term is present: the general bodies
    ragged    64 edges timings of the case

Those corpora move cf1 alone, a kind of flat S1, whose body is the same with and without dead terms.  ONE PARAMETER AT A TIME in the
bodies that differ (flat S0 without turbulence, flat S3 without parallel 1) are the dead VARIANTS of tests/one_at_a_time.py's noisy base:
    p1      pa1 = +0.0 in every frame            46 parameters     every wavefront drops parallel1
    turb    voiceTurbulenceAmplitude = +0.0      46                turbulence
    all     both and aspirationAmplitude         44                both (aspiration: EXPECT has it, BUILT decides the count)
each with tests/one_at_a_time.batch_corpus's recipe (variant_corpus: move pure and as an intruder for every parameter, jump as an intruder
for every parameter and pure for one per kind, edges ragged; the intruders' 63 other lanes move cf1 in the same variant, so the wavefront
stays dead and the lone lane's kind takes it off the usual instantiation).  pf1 / pb1 in p1 and all, and glottalOpenQuotient in turb and
all (INAUDIBLE), move kinds 8 and 21 -- columns the dead bodies step over -- and must not be heard.
PAIRS (pairs_corpus): each of those inaudible parameters moving together with each parameter of a kind behind it in the same flat stage
-- the dead body finds the latter's rows only by counting the moving column it steps over, which no case with ONE moving kind can show.
MIXED SETS (mixed_corpus): whole wavefronts whose lanes have different dead sets -- p1|all, turb|all and p1|turb alternating; all with
one lane that has every term present at lane 0, at lane 63, and as the utterance that ends first; all with one utterance of zero frames
and with one of a single NULL frame (no frame sets a bit; WITHOUT_A_FRAME: four timings) -- each with the move lists of cf1 and of
pf2, and MIXED[composition] the terms the wavefront drops: those dead in every lane.
"""
import numpy as np

from tests import one_at_a_time as oat

SR = oat.SR
LANES = oat.LANES
TERMS = ("parallel1", "turbulence", "aspiration")
PA1, PB1, TURB, ASP, VOICE_AMP = 37, 31, 3, 6, 5
assert (oat.NAMES[PA1], oat.NAMES[PB1], oat.NAMES[TURB], oat.NAMES[ASP], oat.NAMES[VOICE_AMP]) == (
    "pa1", "pb1", "voiceTurbulenceAmplitude", "aspirationAmplitude", "voiceAmplitude")

# case -> ({parameter: value in every frame}, {parameter: value in the list's second frame alone}, the terms that are dead)
CASES = {
    "p1": ({PA1: 0.0}, {}, ("parallel1",)),
    "turb": ({TURB: 0.0}, {}, ("turbulence",)),
    "turb_asp": ({TURB: 0.0, ASP: 0.0}, {}, ("turbulence", "aspiration")),
    "all": ({PA1: 0.0, TURB: 0.0, ASP: 0.0}, {}, TERMS),
    "pa1_negzero": ({PA1: -0.0}, {}, ("parallel1",)),
    "voiceless": ({TURB: 0.0, ASP: 0.0, VOICE_AMP: 0.0}, {}, ("turbulence", "aspiration")),
    "pb1_low": ({PA1: 0.0, PB1: 0.999}, {}, ()),
    "asp_negzero": ({TURB: 0.0, ASP: -0.0}, {}, ("turbulence",)),
    "one_frame": ({PA1: 0.0}, {PA1: 1e-300}, ()),
}
DEAD_CASES = ("p1", "turb", "turb_asp", "all")
EDGE_CASES = ("pa1_negzero", "voiceless")
NEAR_MISSES = ("pb1_low", "asp_negzero", "one_frame")
EXPECT = {name: spec[2] for name, spec in CASES.items()}
PRESENT = "present"      # the unaltered base: every term contributes


def frames_of(case, manner, edge=0):
    """[(frame | None, minSamples, fadeSamples)]: tests/one_at_a_time.py's list of cf1 in the manner, its frames altered for the case."""
    everywhere, second, _ = ({}, {}, ()) if case == PRESENT else CASES[case]
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


def _seed(*key):
    return oat._seed(77, *key)


def corpus(case, compositions=("pure", "intruder", "ragged")):
    """The case's wavefronts as a tests/one_at_a_time.Corpus (what[u] = (parameter, manner, composition, wavefront, lane)), at most 192
    utterances of at most 4000 samples, and per wavefront whether every lane of it is of the case."""
    c, ci = oat.Corpus("noisy"), list(CASES).index(case)
    whole = []
    for comp in compositions:
        for lane in range(LANES):
            if comp == "pure":
                c.add(frames_of(case, "move"), _seed(ci, 1, lane), oat.USUAL, "move", comp, lane)
            elif comp == "intruder":
                c.add(frames_of(PRESENT if lane == 37 else case, "move"), _seed(ci, 2, lane), oat.USUAL, "move", comp, lane)
            else:
                c.add(frames_of(case, "edges", (37 * lane + 11) % LANES), _seed(ci, 3, lane), oat.USUAL, "edges", comp, lane)
        whole.append(comp != "intruder")
    c.finish()
    assert len(c) <= 192 and int(np.diff(c.batch["frame_start"]).max()) <= 8
    return c, whole


# The bodies the engine is built with (KLATT_DEAD_TERMS in csrc/klatt_systolic.h): the source stage without the aspiration generator is
# written and was measured, but it takes the kernel above its register budget for a gain inside the spread (profiles/dead_terms.txt),
# so a wavefront whose aspiration is dead keeps the generator -- its count stays 0 -- and is held to the same bytes all the same.
BUILT = ("parallel1", "turbulence")


def waves(n, dead):
    """kernelInfo()'s three counts when n wavefronts have the terms `dead` dead in all their lanes."""
    return {"waves_without_" + t: (n if t in dead and t in BUILT else 0) for t in TERMS}


def expected_waves(case, whole):
    """kernelInfo()'s counts for the corpus under "sort" = 0 and "dead_terms" = 1: per term the wavefronts all of whose lanes are of the case."""
    return waves(sum(whole), EXPECT[case])


# ---- one parameter at a time in the dead bodies ----------------------------------------------------------------------------------------
# variant -> the parameters that are +0.0 in every frame of tests/one_at_a_time.py's noisy base; what a wavefront of it alone drops is
# EXPECT[variant] (the cases of the same names above zero the same parameters)
VARIANTS = {"p1": (PA1,), "turb": (TURB,), "all": (TURB, ASP, PA1)}
PF1, PF2, OPEN_QUOTIENT = 25, 26, 4
assert (oat.NAMES[PF1], oat.NAMES[PF2], oat.NAMES[OPEN_QUOTIENT]) == ("pf1", "pf2", "glottalOpenQuotient")
# (variant, parameter) that moves without being heard: pf1 / pb1 shape parallel resonator 1, whose gain pa1 is 0 (entry kind 8); the open
# quotient gates the turbulence alone, which is 0 (kind 21).  The dead bodies step over these kinds' entries while they move.
SKIPPED_KIND = {PF1: 8, PB1: 8, OPEN_QUOTIENT: 21}
INAUDIBLE = {("p1", PF1), ("p1", PB1), ("all", PF1), ("all", PB1), ("turb", OPEN_QUOTIENT), ("all", OPEN_QUOTIENT)}


def variant(name):
    """The dead variant's name in tests/one_at_a_time.py (MORE_VARIANTS): oat.case, oat.changed, oat.batch_corpus take it."""
    return "dead_" + name


for _name, _zeroed in VARIANTS.items():
    assert set(CASES[_name][0]) == set(_zeroed) and not any(CASES[_name][0].values())
    oat.MORE_VARIANTS[variant(_name)] = (tuple(p for p in range(47) if p not in _zeroed), tuple(_zeroed))


def variant_corpus(name):
    """tests/one_at_a_time.batch_corpus of the dead variant: every lane of every wavefront is of the variant (the intruders' 63 other lanes
    move cf1 in the same variant), so under "sort" = 0 EVERY wavefront drops EXPECT[name]."""
    return oat.batch_corpus(variant(name))


# TWO at a time: where exactly one kind moves, every kind behind a stepped-over column stands still and is found by counting the kinds that
# do NOT move -- a body that miscounts a MOVING column it steps over reads the right rows all the same.  So each inaudible parameter q moves
# together with each parameter p whose kind lies behind q's in the same stage's part of a track: the body must count q's moving column
# to find p's.  q adds nothing to the PCM: the oracle's PCM of the pair is that of p alone, bit for bit (tests/test_dead_terms_host.py).
BEHIND = {8: (9, 10, 11, 17, 18, 19), 21: (22, 23)}      # flat S3's kinds behind parallel 1's, flat S0's behind the turbulence's


def pairs(name):
    """[(q, p)] of the variant: q inaudible in it, p a parameter of it with a kind behind q's."""
    behind = {q: sum(1 << k for k in BEHIND[SKIPPED_KIND[q]]) for v, q in sorted(INAUDIBLE) if v == name}
    return [(q, p) for q in behind for p in oat.params(variant(name)) if oat.kind_bits(p) & behind[q]]


def pair_case(name, q, p, manner, edge=0):
    """tests/one_at_a_time.case of p in the variant, with q changed as well wherever p is."""
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
    """Per variant a pure wavefront (move) of every pair, then ragged wavefronts (edges, 64 timings) through its pairs in turn, as one
    Corpus: what[u] = (p, manner, "<variant>: <composition> with <q>", wavefront, lane); and the variant of every wavefront."""
    c, of = oat.Corpus("pairs"), []
    for vi, name in enumerate(VARIANTS):
        ps = pairs(name)
        for q, p in ps:
            for lane in range(LANES):
                c.add(pair_case(name, q, p, "move"), _seed(300 + vi, q, p, lane), p, "move", "%s: pure with %s" % (name, oat.NAMES[q]), lane)
            of.append(name)
        for turn in range(-(-len(ps) // LANES)):
            for lane in range(LANES):
                q, p = ps[(lane + 17 * turn) % len(ps)]
                c.add(pair_case(name, q, p, "edges", (37 * lane + 11 * turn) % LANES), _seed(310 + vi, turn, lane), p, "edges",
                      "%s: ragged with %s" % (name, oat.NAMES[q]), lane)
            of.append(name)
    return c.finish(), of


def pairs_waves(of, sets=1):
    """kernelInfo()'s counts for pairs_corpus's wavefronts, `sets` times over, under "sort" = 0 and "dead_terms" = 1."""
    return {"waves_without_" + t: sets * sum(1 for name in of if t in EXPECT[name] and t in BUILT) for t in TERMS}


# The mixed-sets corpus: compositions of a 64-lane wavefront whose lanes have DIFFERENT dead sets, and per composition the terms the
# wavefront must drop.  The rule (dropped_by below): a term goes when no lane has it present -- the intersection of the lanes' dead
# sets, an utterance without a frame that is not NULL having every term dead -- among the terms the engine has bodies for (BUILT).
# Written out here, and held to the rule by tests/test_dead_terms_host.py:
MIXED = {
    "p1|all": ("parallel1",),               # p1 lanes alternating with all lanes
    "turb|all": ("turbulence",),
    "p1|turb": (),
    "present@0": (),                        # all, lane 0 with every term present
    "present@63": (),
    "present_ends_first": (),               # all, lane 29 present and without the list's last frame: the wavefront's shortest utterance
    "no_frames": ("parallel1", "turbulence"),       # all, lane 17 an utterance of zero frames (with pf2: of two NULL frames)
    "null_only": ("parallel1", "turbulence"),       # all, lane 40 an utterance of one NULL frame
}
MIXED_MOVED = (oat.USUAL, PF2)       # every composition once with the move list of cf1 (flat S1) and once with that of pf2 (flat S3)
MIXED_WAVES = {"waves_without_parallel1": 6, "waves_without_turbulence": 6, "waves_without_aspiration": 0}      # of the 16 wavefronts
NO_FRAMES, NULL_ONLY = "no_frames", "null_only"      # lane kinds beside the variants and PRESENT
# The utterances that set no bit, per wavefront of their composition (MIXED_MOVED): four timings, so that each is shared by as many
# utterances as the corpus is repeated.  (Quiet utterances stay on the flat stages, in their lanes, only while fewer than 32 of the batch
# share their timing -- csrc/klatt_batchplan.h, reroute_lonely_quiet -- so the utterance of zero frames is there once.)
WITHOUT_A_FRAME = {NO_FRAMES: ([], [(None, 64, 33), (None, 50, 20)]), NULL_ONLY: ([(None, 100, 100)], [(None, 90, 45)])}


def mixed_lanes(composition):
    """What each of the 64 lanes of a composition is: a variant, PRESENT, NO_FRAMES or NULL_ONLY; and the lane (or None) that lacks its
    list's last frame."""
    if "|" in composition:
        a, b = composition.split("|")
        return [a if lane % 2 == 0 else b for lane in range(LANES)], None
    odd, at, short = {"present@0": (PRESENT, 0, None), "present@63": (PRESENT, 63, None), "present_ends_first": (PRESENT, 29, 29),
                      "no_frames": (NO_FRAMES, 17, None), "null_only": (NULL_ONLY, 40, None)}[composition]
    return [odd if lane == at else "all" for lane in range(LANES)], short


def dropped_by(lanes):
    """The rule: the terms of BUILT that are dead in every lane."""
    dead = {PRESENT: (), NO_FRAMES: TERMS, NULL_ONLY: TERMS}
    return tuple(t for t in TERMS if t in BUILT and all(t in (dead[x] if x in dead else EXPECT[x]) for x in lanes))


def mixed_corpus():
    """The 16 wavefronts of MIXED x MIXED_MOVED as a tests/one_at_a_time.Corpus (what[u] = (parameter, "move", composition, wavefront,
    lane), seeds of their own), and the composition of every wavefront."""
    c, of = oat.Corpus("mixed sets"), []
    for ci, composition in enumerate(MIXED):
        lanes, short = mixed_lanes(composition)
        for p in MIXED_MOVED:
            for lane, kind in enumerate(lanes):
                if kind in (NO_FRAMES, NULL_ONLY):
                    frames = list(WITHOUT_A_FRAME[kind][MIXED_MOVED.index(p)])
                else:
                    frames = oat.case(p, "move", "noisy" if kind == PRESENT else variant(kind))
                    if lane == short:
                        frames = frames[:-1]
                c.add(frames, _seed(200 + ci, p, lane), p, "move", composition, lane)
            of.append(composition)
    return c.finish(), of


def mixed_waves(of, sets=1):
    """kernelInfo()'s counts for wavefronts of the compositions `of`, `sets` times over, under "sort" = 0 and "dead_terms" = 1."""
    return {"waves_without_" + t: sets * sum(1 for comp in of if t in MIXED[comp]) for t in TERMS}


def shared_lists(c):
    """A corpus as setUtterancesShared takes it: its distinct frame lists as a batch dict, and the list of every utterance."""
    first, list_of, lists = {}, [], oat.Corpus(c.variant)
    b = c.batch
    for u in range(len(c)):
        a, e = b["frame_start"][u], b["frame_start"][u + 1]
        key = (b["frames"][a:e].tobytes(), b["min"][a:e].tobytes(), b["fade"][a:e].tobytes(), b["isnull"][a:e].tobytes())
        if key not in first:
            first[key] = len(lists)
            lists.add(c.cases[u], 0, c.what[u][0], c.what[u][1], c.what[u][2], len(lists) % LANES)
        list_of.append(first[key])
    return lists.finish(whole_wavefronts=False).batch, np.array(list_of, np.uint32)
