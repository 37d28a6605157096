"""The flat stages' second set of dead terms on the host, no GPU needed: the second word of "present" facts of a frame and its way to the
utterances (tests/native/check_dead_terms2.cpp, a stand-alone program under AddressSanitizer + UBSan), and the corpora of
tests/dead_terms2.py: their sizes, that every lane is what its wavefront's expectation says, and that a column a lightened body steps
over is not heard in the oracle while the term it belongs to is heard when present."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dead_terms2 as d2
from tests import one_at_a_time as oat
from tests.test_one_at_a_time_host import MIN_SAMPLES, pcm_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCHES = 22     # the branches tests/native/check_dead_terms2.cpp counts; one reached zero times fails the program itself


def test_present2_facts_under_sanitizers(tmp_path):
    """shape_present2 / present2_of (csrc/klatt_plan.h) on hand-written frames, each side of every rule (caNP = -0.0 dead, cbN0 = 0.999
    present, aspirationAmplitude 1e30 dead and beyond it present, pa5 = -0.0 dead, pb5 = 0.999 present, pa3 = 1e-300 in one frame of a list present); NULL frames ignored; the word through
    classify_list, the re-routing of lonely quiet lists, mark_tracked, route_direct, restore_rerouted and pack_lanes, which it does not
    change; dead2_wave_counts on a width-4 order for every value of the built mask.  Nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_dead_terms2")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_dead_terms2.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out
    taken = [int(n) for n in re.findall(r": (\d+)$", out, flags=re.M)]
    assert len(taken) == BRANCHES and min(taken) > 0, out


def test_built_mask_is_the_kernel_constant():
    src = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_systolic.h")).read()
    assert int(re.search(r"#define KLATT_DEAD_TERMS (\d+)", src).group(1)) == d2.BUILT_MASK


def zero_in_every_frame(b, u):
    rows = [k for k in range(b["frame_start"][u], b["frame_start"][u + 1]) if not b["isnull"][k]]
    return {p for p in range(47) if all(b["frames"][k, p] == 0 for k in rows)}      # (zero of either sign)


@pytest.mark.parametrize("name", d2.CORPORA)
def test_corpora_are_what_they_say(name):
    """At most 192 utterances in whole 64-lane wavefronts, at most 8 frames and 4000 samples each; every lane has exactly the zeroed
    parameters its wavefront's expectation is computed from (the cases that sit on the present side of a rule excepted: there the rule
    decides, tests/native/check_dead_terms2.cpp)."""
    c, waves = d2.build(name)
    b = c.batch
    assert len(c) <= 192 and len(c) % d2.LANES == 0 and len(waves) == len(c) // d2.LANES
    assert int(np.diff(b["frame_start"]).max()) <= 8
    lengths = [int(np.sum(np.maximum(b["min"][a:e], b["fade"][a:e] + 1) + 1)) for a, e in zip(b["frame_start"][:-1], b["frame_start"][1:])]
    assert max(lengths) <= 4000
    candidates = set(d2.ZEROED["all2"])
    for u in range(len(c)):
        said = set(waves[u // d2.LANES][u % d2.LANES])
        have = zero_in_every_frame(b, u) & candidates
        if name in ("case:cbN0_low", "case:pb5_low", "case:asp_far"):
            assert said < have and len(have - said) == 1      # the gain is zero, the rule keeps the term
        else:
            assert said == have, (name, u, said, have)


def test_moved_parameters_cover_the_variants():
    """oat_corpus moves and jumps every parameter of its variant, the stepped-over columns included."""
    for name in d2.DEAD_VARIANTS:
        c, _ = d2.oat_corpus(name)
        for manner in ("move", "jump", "edges"):
            assert {w[0] for w in c.what if w[1] == manner} == set(oat.params(d2.variant(name))), (name, manner)
    assert {q for q, _ in d2.pairs("all2")} == {13, 14, 21, 22, 29, 30, 35, 36, 25, 26, 27, 28, 31, 32, 33, 34}
    assert {q for q, _ in d2.pairs("p5")} == {29, 35}


STEPPED_OVER = {"nasal": (13, 14, 21, 22), "p5": (29, 35), "p56": (29, 30, 35, 36), "p1to4": (25, 26, 27, 28, 31, 32, 33, 34)}
TERM_GAINS = {"nasal": (d2.CA_NP,), "p5": (d2.PA5,), "p56": (d2.PA6,), "p1to4": (d2.PA2, d2.PA3, d2.PA4)}


@pytest.mark.parametrize("name", list(STEPPED_OVER))
def test_stepped_over_columns_are_silent_and_the_terms_are_heard(name):
    """Conditions on the inputs, from the oracle alone.  A column the lightened body steps over changes NO sample of the variant's PCM (the
    body must not hear it); each gain the variant zeroes is heard in more samples than tests/test_one_at_a_time_host.py's floor when it is
    present -- a body that dropped a term that IS present would fail the GPU tests."""
    v = d2.variant(name)
    for manner in ("move", "jump"):
        still = pcm_of(oat.case(oat.USUAL, manner, v, unchanged=True), seed=5)
        for q in STEPPED_OVER[name]:
            moved = pcm_of(oat.case(q, manner, v), seed=5)
            assert np.array_equal(moved, still), (name, manner, oat.NAMES[q])
        for g in TERM_GAINS[name]:
            present = [(None if fr is None else np.where(np.arange(47) == g, oat.BASE[g], fr), m, f) for fr, m, f in oat.case(oat.USUAL, manner, v, unchanged=True)]
            d = np.abs(pcm_of(present, seed=5).astype(np.int32) - still.astype(np.int32))
            n = int(np.count_nonzero(d > 1))
            print("%s %s: %s present differs in %d samples by more than 1 LSB" % (name, manner, oat.NAMES[g], n))
            assert n > MIN_SAMPLES, (name, manner, oat.NAMES[g], n)
