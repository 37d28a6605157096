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
