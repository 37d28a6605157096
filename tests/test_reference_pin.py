"""Pin the CPU oracle to the COMPILED reference, call by call, on everything the kernels' special paths exist for.

oracle/klatt_oracle.c is a restatement of the reference by the hands that wrote the kernels; the GPU parity tests compare the
kernels with it.  Here it is compared with the reference itself -- the checkout's three .cpp files compiled in place into
oracle/_ref/libspeechPlayer_ref.so (oracle/Makefile, target `ref`; tests/reference.py) -- with the same noise stream, on

  * all scenarios of tests/scenarios.py, call by call (PCM, call lengths, getLastIndex after every call),
  * the GPU tests' random batches (seeds 1, 2, 11, 12, 21, 22; plain and wild), utterance by utterance,
  * 400 plain + 400 extreme fuzzed call sequences (scenarios.fuzz_sequence): purge anywhere, pulls of 1 .. 8192 samples, frames
    queued onto drained handles, six sample rates; the extreme ones with negative bandwidths, overflowing coefficients, +-inf,
    clipping gains, formants beyond Nyquist and the anti-resonator's zero / denormal frequencies.

Zero tolerance: both sides are IEEE double with glibc's libm, contraction off, the same operation order.  A difference is a
finding in the oracle.

What the library answered is committed as digests (tests/golden/reference.json, written by tests/golden/make_golden.py), so the
pin holds in a checkout with no reference beside it: test_oracle_reproduces_the_recorded_reference always runs; the tests that
call the library skip when neither oracle/_ref/ nor the checkout is there.
"""
import ctypes
import functools
import hashlib
import json
import os
import threading

import numpy as np
import pytest

from tests import oracle, reference, scenarios
from tests.test_oracle_pin import CFG0_FIRST, CFG0_MINMAX, CFG0_SHA1, IPA_COUNTS, IPA_SHA1_10

needs_reference = pytest.mark.skipif(not reference.available(),
                                     reason="no compiled reference (oracle/_ref/libspeechPlayer_ref.so) and no reference checkout to build it from")

GROUPS = ("scenarios", "fuzz_plain", "fuzz_extreme") + tuple("batch_%d" % s for s, _ in scenarios.REFERENCE_BATCHES)


@functools.lru_cache(maxsize=None)
def recorded():
    with open(os.path.join(scenarios.GOLDEN, "reference.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def sequences(group):
    if group == "scenarios":
        return scenarios.build_scenarios(scenarios.Ref())
    if group.startswith("fuzz_"):
        return [scenarios.fuzz_sequence(s, group == "fuzz_extreme") for s in range(scenarios.N_FUZZ)]
    seed = int(group.split("_")[1])
    return scenarios.batch_scenarios(seed, dict(scenarios.REFERENCE_BATCHES)[seed])


@functools.lru_cache(maxsize=None)
def played(group):
    """Every sequence of a group on the oracle and, where there is one, on the compiled reference (in a thread of its own: the two
    libraries share nothing).  -> dict: per sequence the oracle's and the reference's (sha1 of the PCM, calls, marks, sequence digest),
    the first difference between the two per sequence that has one, for the fuzz groups whether the sequence is admitted
    (scenarios.admitted, on the oracle), and the samples compared."""
    scns = sequences(group)
    with_ref = reference.available()
    ref_out = [None] * len(scns)

    def run_reference():
        for i, scn in enumerate(scns):
            ref_out[i] = reference.play_reference(scn)
    th = None
    if with_ref:
        reference.lib()
        th = threading.Thread(target=run_reference)
        th.start()

    def summary(pcm, marks):
        flat = np.concatenate(pcm) if pcm else np.zeros(0, np.int16)
        return (hashlib.sha1(flat.tobytes()).hexdigest(), [int(len(x)) for x in pcm], [int(m) for m in marks],
                scenarios.sequence_digest(pcm, marks))
    res = dict(oracle=[], reference=[], differences=[], admitted=[], samples=0)
    ora_out = []
    for scn in scns:
        if group.startswith("fuzz_"):
            ok, pcm, marks = scenarios.admitted(scn, oracle.OraclePlayer)
            res["admitted"].append(ok)
        else:
            pcm, marks = scenarios.play_oracle(scn)
        res["oracle"].append(summary(pcm, marks))
        res["samples"] += sum(len(x) for x in pcm)
        ora_out.append((pcm, marks) if with_ref else None)
    if th is not None:
        th.join()
        for scn, (op, om), got in zip(scns, ora_out, ref_out):
            assert got is not None, "the reference thread stopped at %s" % scn.name
            rp, rm = got
            res["reference"].append(summary(rp, rm))
            for c, (a, b) in enumerate(zip(op, rp)):
                if len(a) != len(b) or om[c] != rm[c] or not np.array_equal(a, b):
                    n = min(len(a), len(b))
                    bad = np.flatnonzero(a[:n] != b[:n])
                    res["differences"].append("%s call %d: oracle %d samples mark %d, reference %d samples mark %d, first differing sample %s"
                                              % (scn.name, c, len(a), om[c], len(b), rm[c], int(bad[0]) if len(bad) else None))
                    break
    return res


def check_inputs(group):
    """The generators are seeded numpy draws: a numpy that draws differently gives other inputs, which is no fault of the oracle."""
    rec = recorded()
    if group.startswith("fuzz_"):
        want = rec["fuzz"][group[5:]]["input"]
    elif group.startswith("batch_"):
        want = rec["batches"][group[6:]]["input"]
    else:
        return
    assert scenarios.input_digest(sequences(group)) == want, (
        "%s: the generated inputs are not the recorded ones (fixture written with numpy %s, this is %s): "
        "regenerate tests/golden/reference.json with tests/golden/make_golden.py" % (group, rec["numpy"], np.__version__))


def check_against_recorded(group, side):
    rec = recorded()
    got = played(group)[side]
    names = [s.name for s in sequences(group)]
    if group == "scenarios":
        assert sorted(names) == sorted(rec["scenarios"]), "the scenario list changed: regenerate reference.json with make_golden.py"
        bad = [n for n, g in zip(names, got)
               if (g[0], g[1], g[2]) != (rec["scenarios"][n]["sha1"], rec["scenarios"][n]["calls"], rec["scenarios"][n]["marks"])]
    elif group.startswith("fuzz_"):
        want = rec["fuzz"][group[5:]]["sha1"]
        assert len(want) == len(got)
        bad = [n for n, g, w in zip(names, got, want) if g[3] != w]      # (the name carries the seed: replay it to localise)
    else:
        bad = [] if scenarios.group_digest([g[3] for g in got]) == rec["batches"][group[6:]]["sha1"] else [group]
    assert not bad, "%s differs from what the compiled reference answered (tests/golden/reference.json) on %d: %s" % (side, len(bad), bad[:10])


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_reproduces_the_recorded_reference(group):
    """Needs no reference: the oracle gives, sequence by sequence, the digests the compiled reference's answers were recorded with."""
    check_inputs(group)
    check_against_recorded(group, "oracle")


def test_reference_json_agrees_with_expected_json():
    """The scenarios' expected.json (written from the oracle) and reference.json (written from the compiled reference) say the same."""
    with open(os.path.join(scenarios.GOLDEN, "expected.json")) as f:
        exp = json.load(f)
    rec = recorded()["scenarios"]
    assert sorted(exp) == sorted(rec)
    for name, e in exp.items():
        assert (e["sha1"], e["calls"], e["marks"]) == (rec[name]["sha1"], rec[name]["calls"], rec[name]["marks"]), name


def test_sequence_tracer_gives_the_call_lengths():
    """scenarios.trace_sequence -- the sample counter of the frame state machine alone, by which the GPU tests show that every
    kind of purge occurs -- gives every call length of every fuzzed sequence, and every kind of purge occurs among them."""
    total = dict.fromkeys(scenarios.PURGE_KINDS, 0)
    for group in ("fuzz_plain", "fuzz_extreme"):
        for scn, got in zip(sequences(group), played(group)["oracle"]):
            calls, kinds = scenarios.trace_sequence(scn)
            assert calls == got[1], scn.name
            for k, v in kinds.items():
                total[k] += v
    print("purges by kind over %d sequences: %s" % (2 * scenarios.N_FUZZ, total))
    assert all(total.values()), total


def test_admitted_shares():
    """Which sequences the GPU tests hold to the parity bar is decided here, on the CPU (scenarios.admitted): every plain one, and
    all but at most 15 % of the extreme ones.  Measured: 0 of 400 plain, 40 of 400 extreme left out."""
    plain, extreme = played("fuzz_plain")["admitted"], played("fuzz_extreme")["admitted"]
    print("left out: %d of %d plain, %d of %d extreme" % (plain.count(False), len(plain), extreme.count(False), len(extreme)))
    assert all(plain)
    assert extreme.count(False) <= 0.15 * len(extreme)
    kinds = set().union(*(s.kinds for s, ok in zip(sequences("fuzz_extreme"), extreme) if ok))
    assert kinds == set(scenarios.EXTREME_KINDS), kinds          # every extreme kind is among the admitted


@needs_reference
def test_restated_noise_is_the_oracles():
    """oracle/ref_noise.cpp restates klatt_noise31 (the oracle is not linked into the reference library)."""
    R, O = reference.lib(), oracle.lib()
    rng = np.random.default_rng(5)
    for seed, k in zip(rng.integers(0, 2 ** 32, 2000), rng.integers(0, 2 ** 32, 2000)):
        assert R.ref_noise31(int(seed), int(k)) == O.klatt_noise31(int(seed), int(k))
    for seed, k in ((0, 0), (0, 2 ** 32 - 1), (2 ** 32 - 1, 0), (2 ** 32 - 1, 2 ** 32 - 1), (1, 1)):
        assert R.ref_noise31(seed, k) == O.klatt_noise31(seed, k)


@needs_reference
def test_known_answers_come_out_of_this_build():
    """The values tests/test_oracle_pin.py holds (recorded from a compiled reference with glibc rand() after srand(1)) from THIS
    build of the reference in libc noise mode: cfg0, and the eight sampleIpa.txt lines in one process in order."""
    ref = scenarios.Ref()
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(1)
    p = reference.RefPlayer(22050, noise=reference.NOISE_LIBC)
    p.queue(scenarios.vowel_frame(ref, "a", 120.0), scenarios.ms(1000), scenarios.ms(50))
    first, second = p.synthesize(22050), p.synthesize(22050)
    p.close()
    assert len(first) == 22050 and len(second) == 1
    assert first[:20].tolist() == CFG0_FIRST
    assert (int(first.min()), int(first.max())) == CFG0_MINMAX
    assert hashlib.sha1(first.tobytes()).hexdigest() == CFG0_SHA1
    libc.srand(1)
    for line in range(8):
        p = reference.RefPlayer(22050, noise=reference.NOISE_LIBC)
        for fr, m, f in ref.ipa_case(ref.find_ipa(line, speed=1.0, clause=0, pitch=100.0, infl=0.5)):
            p.queue(fr, m, f)
        pcm = p.drain()
        p.close()
        assert len(pcm) == IPA_COUNTS[line]
        assert hashlib.sha1(pcm.tobytes()).hexdigest()[:10] == IPA_SHA1_10[line], "line %d" % line


@needs_reference
@pytest.mark.parametrize("group", GROUPS)
def test_reference_reproduces_its_record(group):
    """Guards a stale fixture: the library built here answers what reference.json holds."""
    check_inputs(group)
    check_against_recorded(group, "reference")


@needs_reference
@pytest.mark.parametrize("group", GROUPS)
def test_oracle_equals_reference_call_by_call(group):
    """PCM, call length and getLastIndex of every call of every sequence: oracle == compiled reference."""
    res = played(group)
    print("%s: %d sequences, %d samples on each side, %d sequences differ" % (group, len(sequences(group)), res["samples"], len(res["differences"])))
    assert not res["differences"], res["differences"][:10]
