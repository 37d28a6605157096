"""The flat stages' dead terms on the host, no GPU needed: the three "present" facts of a frame and their way into UttDesc.flags
(tests/native/check_dead_terms.cpp, a stand-alone program under AddressSanitizer + UBSan), and that tests/test_gpu_dead_terms.py can
fail: each term the stage bodies leave out is audible in the oracle's PCM when it is present."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dead_terms as dt
from tests import one_at_a_time as oat
from tests.test_one_at_a_time_host import MIN_SAMPLES, pcm_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD_TERMS_BRANCHES = 16     # the branches tests/native/check_dead_terms.cpp counts; one reached zero times fails the program itself


def test_present_facts_under_sanitizers(tmp_path):
    """shape_flags (csrc/klatt_plan.h) on hand-written frames, each side of every rule; the OR over a list with NULL frames and one
    offending frame in the middle; the bits through classify_list, the re-routing of lonely quiet lists, mark_tracked, route_direct and
    restore_rerouted into what every utterance carries (csrc/klatt_batchplan.h).  Nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_dead_terms")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_dead_terms.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out
    taken = [int(n) for n in re.findall(r": (\d+)$", out, flags=re.M)]
    assert len(taken) == DEAD_TERMS_BRANCHES and min(taken) > 0, out


@pytest.mark.parametrize("case", dt.DEAD_CASES)
def test_each_dead_term_is_audible_when_present(case):
    """A condition on the inputs, not a measurement of the engine: the oracle's PCM of the unaltered base (pa1 = 0.5, turbulence and
    aspiration 0.2) differs from the case's by more than 1 LSB on more samples than tests/test_one_at_a_time_host.py's floor, in both
    manners -- a stage body that dropped a term that IS present would be heard."""
    for manner in ("move", "jump"):
        present = pcm_of(dt.frames_of(dt.PRESENT, manner), seed=5)
        dead = pcm_of(dt.frames_of(case, manner), seed=5)
        assert len(present) == len(dead)
        d = np.abs(present.astype(np.int32) - dead.astype(np.int32))
        n = int(np.count_nonzero(d > 1))
        print("%s %s: %d samples differ by more than 1 LSB (largest difference %d LSB)" % (case, manner, n, int(d.max())))
        assert n > MIN_SAMPLES, (case, manner, n)


def test_cases_are_what_they_say():
    """Every case alters the base in the parameters it names and nowhere else; one_frame's offending value sits in one frame, in the
    middle of the list; the corpus of a case holds whole wavefronts of at most 4000 samples per utterance."""
    for case, (everywhere, second, _) in dt.CASES.items():
        for manner in ("move", "jump"):
            got = [fr for fr, _, _ in dt.frames_of(case, manner) if fr is not None]
            ref = [fr for fr, _, _ in oat.case(oat.USUAL, manner, "noisy") if fr is not None]
            for j, (g, r) in enumerate(zip(got, ref)):
                want = r.copy()
                for p, v in everywhere.items():
                    want[p] = v
                if j == 1:
                    for p, v in second.items():
                        want[p] = v
                assert np.array_equal(g.view(np.uint64), want.view(np.uint64)), (case, manner, j)
        c, whole = dt.corpus(case)
        assert len(c) == 192 and whole == [True, False, True]
        b = c.batch
        lengths = [int(np.sum(np.maximum(b["min"][a:e], b["fade"][a:e] + 1) + 1)) for a, e in zip(b["frame_start"][:-1], b["frame_start"][1:])]
        assert max(lengths) <= 4000
    assert set(dt.DEAD_CASES + dt.EDGE_CASES + dt.NEAR_MISSES) == set(dt.CASES)
    assert all(not dt.EXPECT[c] or c == "asp_negzero" for c in dt.NEAR_MISSES) and dt.EXPECT["asp_negzero"] == ("turbulence",)
