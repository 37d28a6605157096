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
from tests.test_one_at_a_time_host import MAX_PEAK, MIN_SAMPLES, check_audible, check_corpus_shape, check_masks_and_kinds, pcm_of, plan_kinds

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


# ---- one parameter at a time in the dead bodies (tests/dead_terms.py: VARIANTS, the mixed sets) -----------------------------------------

def lengths_of(b):
    return np.array([int(np.sum(np.maximum(b["min"][a:e], b["fade"][a:e] + 1) + 1)) for a, e in zip(b["frame_start"][:-1], b["frame_start"][1:])])


def dead_in(b, u):
    """The terms no frame of utterance u has, from its frames alone: the gain +0.0 bit for bit in every frame that is not NULL (pa1: zero)."""
    rows = [k for k in range(b["frame_start"][u], b["frame_start"][u + 1]) if not b["isnull"][k]]
    col = {"parallel1": dt.PA1, "turbulence": dt.TURB, "aspiration": dt.ASP}
    return {t for t in dt.TERMS if all(b["frames"][k, col[t]].view(np.uint64) == 0 for k in rows)}


@pytest.mark.parametrize("name", list(dt.VARIANTS))
def test_dead_variant_cases_are_audible_but_for_the_skipped_columns(name):
    """tests/test_one_at_a_time_host.py's condition for the dead variants: every parameter, move and jump, is heard in more than 25 samples
    by more than 1 LSB and nothing peaks at 16 000 -- but pf1 and pb1 where pa1 = 0 (kind 8 moves) and glottalOpenQuotient where the
    turbulence is 0 (kind 21 moves), which must differ in NO sample: columns that move, are stepped over, and must not be heard.
    Measured (conditions on the inputs, no tolerance of the engine's):   weakest move   weakest jump   peak (edges cases included)
                                                                  p1     pb6, 108       pb6, 94        4882
                                                                  turb   pb6, 103       pb6, 89        4635
                                                                  all    pb6, 104       pb6, 83        4709"""
    inaudible = {p for v, p in dt.INAUDIBLE if v == name}
    assert inaudible == {"p1": {dt.PF1, dt.PB1}, "turb": {dt.OPEN_QUOTIENT}, "all": {dt.PF1, dt.PB1, dt.OPEN_QUOTIENT}}[name]
    assert inaudible <= set(oat.params(dt.variant(name))) and not set(dt.VARIANTS[name]) & set(oat.params(dt.variant(name)))
    weakest, peak = check_audible(dt.variant(name), inaudible)
    assert all(n > MIN_SAMPLES for _, n in weakest.values()) and peak < MAX_PEAK, (weakest, peak)


@pytest.mark.parametrize("name", list(dt.VARIANTS))
def test_dead_variant_corpus_and_the_kinds_it_skips(name):
    """The variant's corpus holds every (parameter, manner) as tests/one_at_a_time.batch_corpus does, in whole wavefronts of lists of at most
    8 frames and 4000 samples; every frame has the variant's gains at +0.0 and no other of the three; and the planner sees every case
    as what it is -- the SKIPPED entries really move: where pf1 / pb1 move under pa1 = 0 the moving fades' masks hold bit 8 and the
    utterance's kinds word kind 8, likewise bit 21 for glottalOpenQuotient under turbulence 0; every other case exactly kind_bits(p)."""
    v = dt.variant(name)
    c = check_corpus_shape(v)
    b = c.batch
    assert len(c) % oat.LANES == 0 and int(np.diff(b["frame_start"]).max()) <= 8 and int(lengths_of(b).max()) <= 4000
    want = set(dt.EXPECT[name])
    assert all(dead_in(b, u) == want for u in range(len(c)))
    mask, kinds = check_masks_and_kinds(c, v)       # move: [gain, kind_bits(p), kind_bits(p), gain]; the word: kind_bits(p) | gain
    gain = oat.kind_bits(44)
    assert {p: oat.kind_bits(p) for p in dt.SKIPPED_KIND} == {dt.PF1: 1 << 8, dt.PB1: 1 << 8, dt.OPEN_QUOTIENT: 1 << 21}
    skipped = {(p, m): 0 for v_, p in dt.INAUDIBLE if v_ == name for m in oat.MANNERS}
    for u in range(len(c)):
        p, manner = c.what[u][:2]
        if (p, manner) not in skipped:
            continue
        bit = 1 << dt.SKIPPED_KIND[p]
        m = [int(x) for x in mask[b["frame_start"][u]:b["frame_start"][u + 1]]]
        assert int(kinds[u]) == bit | gain, c.describe(u)
        assert m == ([gain] * 4 if manner == "jump" else [gain, bit, bit, gain]), c.describe(u)
        skipped[(p, manner)] += 1
    assert skipped and min(skipped.values()) > 0, skipped


def test_pairs_move_a_skipped_column_with_every_kind_behind_it():
    """tests/dead_terms.pairs_corpus: in every variant each inaudible parameter q (kind 8 under pa1 = 0, kind 21 under turbulence 0) moves
    in the SAME fades as each parameter p of a kind behind it in its flat stage -- written out here -- so the dead body finds p's rows
    only by counting q's moving column.  The planner shows both kinds in the moving fades' masks; the oracle's PCM of the pair is that
    of p alone in every sample (q adds nothing), which the one-at-a-time test holds to its floor of audibility."""
    s3 = (24, 26, 27, 28, 32, 33, 34, 38, 39, 40, 44)      # fricationAmplitude, pf2..4, pb2..4, pa2..4, preFormantGain: kinds 17, 9..11, 18, 19
    assert dt.pairs("p1") == [(q, p) for q in (dt.PF1, dt.PB1) for p in s3]
    assert dt.pairs("turb") == [(dt.OPEN_QUOTIENT, p) for p in (5, 6, 44)]      # voiceAmplitude, aspirationAmplitude: kind 22; the gain: 23
    assert dt.pairs("all") == [(dt.OPEN_QUOTIENT, p) for p in (5, 44)] + [(q, p) for q in (dt.PF1, dt.PB1) for p in s3]
    for name in dt.VARIANTS:
        for q, p in dt.pairs(name):
            behind = dt.BEHIND[dt.SKIPPED_KIND[q]]
            assert (name, q) in dt.INAUDIBLE and (name, p) not in dt.INAUDIBLE and min(behind) > dt.SKIPPED_KIND[q]
            assert any(oat.kind_bits(p) >> k & 1 for k in behind), (name, q, p)
            for manner in ("move", "jump"):
                assert np.array_equal(pcm_of(dt.pair_case(name, q, p, manner), seed=9), pcm_of(oat.case(p, manner, dt.variant(name)), seed=9)), (name, q, p, manner)
    c, of = dt.pairs_corpus()
    b = c.batch
    assert of == ["p1"] * 23 + ["turb"] * 4 + ["all"] * 25 and len(c) == len(of) * oat.LANES
    assert dt.pairs_waves(of) == {"waves_without_parallel1": 48, "waves_without_turbulence": 29, "waves_without_aspiration": 0}
    assert int(np.diff(b["frame_start"]).max()) <= 8 and int(lengths_of(b).max()) <= 4000
    assert all(dead_in(b, u) == set(dt.EXPECT[of[u // oat.LANES]]) for u in range(len(c)))
    mask, tracked, kinds = plan_kinds(b)
    assert tracked.all()
    gain, seen = oat.kind_bits(44), set()
    for u in range(len(c)):
        p, manner, comp = c.what[u][:3]
        q = oat.NAMES.index(comp.split(" with ")[1])
        both = oat.kind_bits(p) | oat.kind_bits(q)
        assert oat.kind_bits(q) == 1 << dt.SKIPPED_KIND[q] and oat.kind_bits(p) & ~oat.kind_bits(q)
        assert [int(x) for x in mask[b["frame_start"][u]:b["frame_start"][u + 1]]] == [gain, both, both, gain], c.describe(u)
        assert int(kinds[u]) == both | gain, c.describe(u)
        seen.add((of[u // oat.LANES], q, p, manner))
    assert seen == {(name, q, p, manner) for name in dt.VARIANTS for q, p in dt.pairs(name) for manner in ("move", "edges")}
    for w in range(len(of)):
        timing = {(b["min"][b["frame_start"][u]:b["frame_start"][u + 1]].tobytes(), b["fade"][b["frame_start"][u]:b["frame_start"][u + 1]].tobytes()) for u in range(w * oat.LANES, (w + 1) * oat.LANES)}
        assert len(timing) == (oat.LANES if "ragged" in c.what[w * oat.LANES][2] else 1)


def test_mixed_sets_corpus_is_what_its_table_says():
    """Every composition's dropped terms, written out in tests/dead_terms.MIXED, are what the rule gives (the terms dead in every lane, among
    those the engine has bodies for) -- from the lanes' names and, independently, from the frames the corpus holds; the counts of
    kernelInfo() written out in MIXED_WAVES are the table's; the utterance that must end first does, and the ones without a frame
    have none."""
    assert dt.MIXED == {"p1|all": ("parallel1",), "turb|all": ("turbulence",), "p1|turb": (), "present@0": (), "present@63": (),
                        "present_ends_first": (), "no_frames": ("parallel1", "turbulence"), "null_only": ("parallel1", "turbulence")}
    assert dt.MIXED_WAVES == {"waves_without_parallel1": 6, "waves_without_turbulence": 6, "waves_without_aspiration": 0}
    c, of = dt.mixed_corpus()
    b = c.batch
    assert len(c) == 16 * oat.LANES and of == [comp for comp in dt.MIXED for _ in dt.MIXED_MOVED]
    assert dt.mixed_waves(of) == dt.MIXED_WAVES and dt.mixed_waves(of, 3) == {k: 3 * n for k, n in dt.MIXED_WAVES.items()}
    lens = lengths_of(b)
    assert int(np.diff(b["frame_start"]).max()) <= 8 and int(lens.max()) <= 4000
    for w, comp in enumerate(of):
        lanes, short = dt.mixed_lanes(comp)
        assert dt.dropped_by(lanes) == dt.MIXED[comp], comp
        us = range(w * oat.LANES, (w + 1) * oat.LANES)
        assert all(c.what[u][2:] == (comp, w, u % oat.LANES) and c.what[u][0] == dt.MIXED_MOVED[w % 2] for u in us)
        common = set(dt.TERMS)
        for u in us:
            common &= dead_in(b, u)
        assert tuple(t for t in dt.TERMS if t in common and t in dt.BUILT) == dt.MIXED[comp], comp
        # lanes with different dead sets, none of them empty, in the alternating compositions
        if "|" in comp:
            assert {frozenset(dead_in(b, u)) for u in us} == {frozenset(dt.EXPECT[x]) for x in comp.split("|")}
        wl = lens[w * oat.LANES:(w + 1) * oat.LANES]
        n = np.diff(b["frame_start"])[w * oat.LANES:(w + 1) * oat.LANES]
        if comp == "present_ends_first":
            assert short == 29 and wl[29] == wl.min() and np.count_nonzero(wl == wl.min()) == 1 and not dead_in(b, w * oat.LANES + 29)
        elif comp in ("no_frames", "null_only"):
            at = 17 if comp == "no_frames" else 40
            k = b["frame_start"][w * oat.LANES + at]
            assert n[at] == {"no_frames": (0, 2), "null_only": (1, 1)}[comp][w % 2] and b["isnull"][k:k + n[at]].all() and (np.delete(n, at) == 4).all()
            assert (wl[at] == 0) == (comp == "no_frames" and w % 2 == 0)
        else:
            assert len(set(wl)) == 1 and (n == 4).all()
    # setUtterancesShared's form of it: the same utterances from distinct lists
    lists, list_of = dt.shared_lists(c)
    assert len(list_of) == len(c) and len(lists["frame_start"]) - 1 == int(list_of.max()) + 1 < len(c)
    # the utterances without a frame have four timings of their own: as many share one as the corpus is repeated
    quiet = [u for u in range(len(c)) if dead_in(b, u) == set(dt.TERMS) and c.what[u][2] in ("no_frames", "null_only") and b["isnull"][b["frame_start"][u]:b["frame_start"][u + 1]].all()]
    assert len(quiet) == 4 and len({(b["min"][b["frame_start"][u]:b["frame_start"][u + 1]].tobytes(), b["fade"][b["frame_start"][u]:b["frame_start"][u + 1]].tobytes()) for u in quiet}) == 4
    for u in (0, 65, 17 + 12 * oat.LANES, 40 + 15 * oat.LANES, len(c) - 1):
        a, e, la, le = b["frame_start"][u], b["frame_start"][u + 1], lists["frame_start"][list_of[u]], lists["frame_start"][list_of[u] + 1]
        assert np.array_equal(b["frames"][a:e], lists["frames"][la:le]) and np.array_equal(b["min"][a:e], lists["min"][la:le])
        assert np.array_equal(b["fade"][a:e], lists["fade"][la:le]) and np.array_equal(b["isnull"][a:e], lists["isnull"][la:le])
