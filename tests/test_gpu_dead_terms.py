"""The flat stages' bodies without dead terms (option "dead_terms", csrc/klatt_systolic.h) against the oracle and against the general
bodies, on the batches of tests/dead_terms.py.  Needs a GPU.

Per case: MODE_EXACT equals the oracle with 0 differing samples and equals the same batch under "dead_terms" = 0 byte for byte, index
marks included; MODE_FAST stays within tests/test_gpu_parity.py's bar; and kernelInfo() counts the wavefronts that dropped each term
-- as many as the case has wavefronts all of whose lanes are dead, none in a near miss, none under "dead_terms" = 0 -- so that a body
that silently never runs fails.  pa1 = -0.0 and voiceAmplitude = 0 sit on the dead side of their rules (zero of either sign; the
sum 0.0 + voice kept as an add) and are held to the same bytes.

Those cases move cf1, a kind of flat S1.  The dead VARIANTS of the one-parameter-at-a-time corpus, the pairs and the mixed sets
(tests/dead_terms.py) move every kind of the bodies that differ, in both flat launches -- as they are (one workgroup per CU) and
repeated in order past the CUs (two per CU: the instantiation bench.py times) -- and hold one player launched again and again, and
the shared lists, to the same bytes and counts.
"""
import numpy as np
import pytest

from tests import dead_terms as dt
from tests import oracle
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu

FLAT = dict(tracks=1, direct=0)
_built = {}


def built(case):
    """(corpus, whole wavefronts, the oracle's pcm, start): once per module run."""
    if case not in _built:
        c, whole = dt.corpus(case)
        exp, exp_start, _ = c.oracle(threads=8)
        exp.setflags(write=False)
        _built[case] = (c, whole, exp, exp_start)
    return _built[case]


def run(b, mode, dead_terms, sort=0, marks=False):
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(dt.SR, mode=mode)
    for k, v in FLAT.items():
        bp.setOption(k, v)
    bp.setOption("sort", sort)
    bp.setOption("dead_terms", dead_terms)
    bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
    bp.synthesize()
    pcm, start = bp.readAll()
    info = bp.kernelInfo()
    last = [bp.getLastIndex(u) for u in range(len(b["seeds"]))] if marks else None
    bp.close()
    return pcm.copy(), start, info, last


def counts(info):
    return {k: v for k, v in info.items() if k.startswith("waves_without_")}


@pytest.mark.parametrize("case", list(dt.CASES))
def test_case_against_oracle_and_general_bodies(case):
    c, whole, exp, exp_start = built(case)
    b = dict(c.batch)
    b["index"] = np.arange(len(b["index"]), dtype=np.int32) % 1000      # index marks of their own, so that getLastIndex says something
    got, start, info, last = run(b, 0, 1, marks=True)
    ref, ref_start, ref_info, ref_last = run(b, 0, 0, marks=True)
    print("%s: %d utterances, %d samples; dead_terms 1 %s; dead_terms 0 %s" % (case, len(c), len(exp), counts(info), counts(ref_info)))
    assert info["tracked_utterances"] == len(c) == ref_info["tracked_utterances"], info
    assert info["scratch_bytes"] == 0, info
    assert np.array_equal(start, exp_start) and np.array_equal(ref_start, exp_start)
    diff = c.first_difference(got, exp, start)
    assert diff is None, "dead_terms 1 against the oracle: %s" % diff
    diff = c.first_difference(got, ref, start)
    assert diff is None and got.tobytes() == ref.tobytes(), "dead_terms 1 against dead_terms 0: %s" % diff
    assert last == ref_last
    assert counts(info) == dt.expected_waves(case, whole), (case, counts(info))
    assert not any(counts(ref_info).values()), counts(ref_info)
    # sorted lanes (the engine's default packing): same bytes, whatever wavefronts the sort made
    srt, srt_start, _, _ = run(b, 0, 1, sort=1)
    assert np.array_equal(srt_start, start) and srt.tobytes() == got.tobytes()
    fast, fast_start, fast_info, _ = run(b, 1, 1)
    assert np.array_equal(fast_start, exp_start)
    flips = compare(fast, exp, "%s, MODE_FAST" % case)
    assert counts(fast_info) == dt.expected_waves(case, whole), (case, counts(fast_info))
    print("%s MODE_FAST: %d one-LSB differences from the oracle" % (case, flips))


# ---- one parameter at a time in the dead bodies, in both flat launches (tests/dead_terms.py: VARIANTS, the mixed sets) ------------------

OAT_CORPORA = list(dt.VARIANTS) + ["pairs", "mixed"]
_oat, _untiled = {}, {}


def oat_built(name):
    """(corpus, kernelInfo()'s counts under "sort" = 0 and "dead_terms" = 1, the oracle's pcm, start): once per module run."""
    if name not in _oat:
        if name == "mixed":
            c, of = dt.mixed_corpus()
            want = dt.mixed_waves(of)
            assert want == dt.MIXED_WAVES
        elif name == "pairs":
            c, of = dt.pairs_corpus()
            want = dt.pairs_waves(of)
        else:
            c = dt.variant_corpus(name)
            want = dt.waves(len(c) // dt.LANES, dt.EXPECT[name])      # every lane of every wavefront is of the variant
        exp, exp_start, _ = c.oracle(threads=8)
        exp.setflags(write=False)
        _oat[name] = (c, want, exp, exp_start)
    return _oat[name]


def marked(c):
    b = dict(c.batch)
    b["index"] = np.arange(len(b["index"]), dtype=np.int32) % 1000      # index marks of their own, so that getLastIndex says something
    return b


def untiled(name):
    """The corpus as it is, MODE_EXACT, "dead_terms" = 1, lanes in the given order: (pcm, start, kernelInfo(), last index marks), run once."""
    if name not in _untiled:
        got, start, info, last = run(marked(oat_built(name)[0]), 0, 1, marks=True)
        got.setflags(write=False)
        _untiled[name] = (got, start, info, last)
    return _untiled[name]


def tiles_past(n, cus):
    """The smallest k for which n * k utterances no longer fit one workgroup per CU (plan_group, csrc/klatt_engine.hip)."""
    k = 1
    while n * k // dt.LANES + 1 <= cus:
        k += 1
    return k


@pytest.mark.parametrize("launch", ["one_per_cu", "two_per_cu"])
@pytest.mark.parametrize("name", OAT_CORPORA)
def test_one_parameter_at_a_time_in_the_dead_bodies(name, launch):
    """Every parameter of a dead variant moving or jumping alone (then the pairs: a stepped-over column moving together with each kind
    behind it; and the mixed sets) on the flat stages, lanes in the given order, in
    BOTH flat launches: as it is -- one workgroup per CU -- and repeated k times in order until the batch no longer
    fits (kernelInfo(): wavefronts // 4 + 1 against cus), which is the instantiation with two workgroups per CU that bench.py times.
    MODE_EXACT under "dead_terms" = 1: 0 samples from the oracle, tile by tile; the untiled run's bytes, tile by tile; the bytes and index
    marks of "dead_terms" = 0; the same bytes with sorted lanes.  MODE_FAST: tests/test_gpu_parity.py's bar.  The counts of wavefronts that
    dropped a term are the expected ones exactly (k times over), and zero under "dead_terms" = 0."""
    c0, want0, exp, exp_start = oat_built(name)
    base, base_start, base_info, base_last = untiled(name)
    cus = base_info["cus"]
    assert base_info["wavefronts"] // 4 + 1 <= cus, base_info
    k = tiles_past(len(c0), cus) if launch == "two_per_cu" else 1
    # (the utterances without a frame of the mixed sets stay on the flat stages while fewer than 32 share their timing: csrc/klatt_batchplan.h, kRunMin)
    assert name != "mixed" or k < 32, (k, cus)
    c, want = (c0.tiled(k), {t: k * n for t, n in want0.items()}) if k > 1 else (c0, want0)
    b = marked(c)
    got, start, info, last = run(b, 0, 1, marks=True) if k > 1 else (base, base_start, base_info, base_last)
    print("%s %s: %d x %d utterances, %d samples; %d wavefronts on %d CUs, hand-overs of %d samples, %d VGPRs (untiled: %d); %s" % (
        name, launch, k, len(c0), len(got), info["wavefronts"], cus, info["stage_parallel_chunk"], info["vgprs"], base_info["vgprs"], counts(info)))
    assert (info["wavefronts"] // 4 + 1 > cus) == (launch == "two_per_cu"), info
    assert info["tracked_utterances"] == len(c) and info["scratch_bytes"] == 0, info
    want_start = np.concatenate([[0], np.cumsum(np.tile(np.diff(exp_start), k))]).astype(np.int64)
    assert np.array_equal(start, want_start)
    n = len(exp)
    for t in range(k):
        tile = got[t * n:(t + 1) * n]
        diff = c0.first_difference(tile, exp, exp_start)
        assert diff is None, "%s, tile %d of %d, dead_terms 1 against the oracle: %s" % (launch, t, k, diff)
        diff = c0.first_difference(tile, base, exp_start)
        assert diff is None and tile.tobytes() == base.tobytes(), "%s, tile %d of %d against the untiled run: %s" % (launch, t, k, diff)
    assert counts(info) == want, (name, launch, counts(info), want)
    ref, ref_start, ref_info, ref_last = run(b, 0, 0, marks=True)
    assert ref_info["tracked_utterances"] == len(c) and ref_info["wavefronts"] == info["wavefronts"], ref_info
    diff = c.first_difference(got, ref, start)
    assert diff is None and np.array_equal(ref_start, start) and got.tobytes() == ref.tobytes(), "dead_terms 1 against dead_terms 0: %s" % diff
    assert last == ref_last
    assert not any(counts(ref_info).values()), counts(ref_info)
    del ref
    srt, srt_start, srt_info, _ = run(b, 0, 1, sort=1)
    assert np.array_equal(srt_start, start) and srt.tobytes() == got.tobytes(), c.first_difference(srt, got, start)
    assert srt_info["tracked_utterances"] == len(c), srt_info
    del srt
    fast, fast_start, fast_info, _ = run(b, 1, 1)
    assert np.array_equal(fast_start, start)
    want_pcm = np.tile(exp, k) if k > 1 else exp
    try:
        flips = compare(fast, want_pcm, "%s %s, MODE_FAST" % (name, launch))
    except AssertionError as e:
        beyond = int(np.abs(fast.astype(np.int32) - want_pcm.astype(np.int32)).max()) > 1
        raise AssertionError("%s -- %s" % (e, c.first_difference(fast, want_pcm, start, 1 if beyond else 0)))
    assert counts(fast_info) == want and (fast_info["wavefronts"] // 4 + 1 > cus) == (launch == "two_per_cu"), fast_info
    print("%s %s MODE_FAST: %d one-LSB differences from the oracle, %d VGPRs" % (name, launch, flips, fast_info["vgprs"]))


@pytest.mark.parametrize("sort", [0, 1])
def test_every_launch_reads_the_option(sort):
    """One player, the mixed sets set once, launched under "dead_terms" 1, 0, 1, 0: the same bytes (the oracle's) every time, the counts
    the plan's, zero, the plan's, zero.  Before the first launch kernelInfo() reports what the plan says the stages will decide
    (dead_wave_counts, csrc/klatt_batchplan.h, from the bits in UttDesc.flags); the first launch counted the same on the device.  In the
    given order that is tests/dead_terms.MIXED_WAVES; with sorted lanes whatever wavefronts the sort made."""
    import nvspeechplayer_amd as eng
    c, want, exp, exp_start = oat_built("mixed")
    b = c.batch
    bp = eng.BatchPlayer(dt.SR, mode=0)
    try:
        for k, v in FLAT.items():
            bp.setOption(k, v)
        bp.setOption("sort", sort)
        bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
        plan = counts(bp.kernelInfo())
        if sort == 0:
            assert plan == want == dt.MIXED_WAVES, plan
        for launch, dead_terms in enumerate((1, 0, 1, 0)):
            bp.setOption("dead_terms", dead_terms)
            bp.synthesize()
            pcm, start = bp.readAll()
            info = bp.kernelInfo()
            assert info["tracked_utterances"] == len(c), info
            assert counts(info) == (plan if dead_terms else dt.waves(0, ())), (launch, dead_terms, counts(info), plan)
            assert np.array_equal(start, exp_start)
            diff = c.first_difference(pcm, exp, start)
            assert diff is None, "launch %d, dead_terms %d: %s" % (launch, dead_terms, diff)
        print("sort %d: plan %s" % (sort, plan))
    finally:
        bp.close()


def test_shared_lists_carry_their_bits():
    """The mixed sets through setUtterancesShared -- their distinct lists and a list per utterance: the bits reach UttDesc.flags through
    classify_list per LIST there -- give the bytes and the counts of setUtterances."""
    import nvspeechplayer_amd as eng
    c, want, exp, exp_start = oat_built("mixed")
    base, base_start, _, _ = untiled("mixed")
    lists, list_of = dt.shared_lists(c)
    bp = eng.BatchPlayer(dt.SR, mode=0)
    try:
        for k, v in FLAT.items():
            bp.setOption(k, v)
        bp.setOption("sort", 0)
        bp.setUtterancesShared(lists["frame_start"], lists["frames"], lists["min"], lists["fade"], list_of, lists["index"], lists["isnull"], c.batch["seeds"])
        assert counts(bp.kernelInfo()) == want
        for dead_terms in (1, 0):
            bp.setOption("dead_terms", dead_terms)
            bp.synthesize()
            pcm, start = bp.readAll()
            info = bp.kernelInfo()
            assert info["tracked_utterances"] == len(c) and info["scratch_bytes"] == 0, info
            assert counts(info) == (want if dead_terms else dt.waves(0, ())), (dead_terms, counts(info))
            assert np.array_equal(start, base_start)
            diff = c.first_difference(pcm, base, start)
            assert diff is None and pcm.tobytes() == base.tobytes(), "%d lists, dead_terms %d, against setUtterances: %s" % (len(list_of), dead_terms, diff)
            assert c.first_difference(pcm, exp, start) is None
    finally:
        bp.close()


def sparse_batch(cases):
    """One utterance per entry of `cases` (move lists, seeds of their own): fewer than a wavefront, which the packing completes with replica lanes."""
    from tests import one_at_a_time as oat
    c = oat.Corpus("noisy")
    for k, case in enumerate(cases):
        c.add(dt.frames_of(case, "move" if k % 2 == 0 else "jump"), dt._seed(99, k), oat.USUAL, "move", "sparse", k)
    return c.finish(whole_wavefronts=False)


@pytest.mark.parametrize("sort", [0, 1])
def test_sparse_wavefront_replica_lanes_carry_their_bits(sort):
    """Five utterances in one wavefront: its other lanes are replicas, which carry their utterance's bits.  All five dead: the wavefront
    drops every term; one of the five with everything present: it drops none."""
    for cases, dead in ((["all"] * 5, True), (["all", "all", dt.PRESENT, "all", "all"], False)):
        c = sparse_batch(cases)
        exp, exp_start, _ = c.oracle(threads=4)
        got, start, info, _ = run(c.batch, 0, 1, sort=sort)
        ref, _, ref_info, _ = run(c.batch, 0, 0, sort=sort)
        assert info["tracked_utterances"] == 5, info
        assert np.array_equal(start, exp_start)
        diff = c.first_difference(got, exp, start)
        assert diff is None, diff
        assert got.tobytes() == ref.tobytes()
        assert counts(info) == dt.waves(1, dt.TERMS if dead else ()), counts(info)
        assert not any(counts(ref_info).values())


def test_ipa_text_batch():
    """From IPA text through setIpa, lanes in the given order: a wavefront of `hælou` -- h has aspiration -- drops turbulence and parallel 1,
    which no phoneme of the producer's table sets; in a wavefront of a sentence without h all three terms are dead (tests/dead_terms.py,
    BUILT: which of them the engine has bodies for)."""
    import nvspeechplayer_amd as eng
    # (no h and no voiceless stop, behind which the producer inserts a puff of aspiration; z and v: frication, so the utterance is noisy and tracked)
    texts = ["hælou"] * dt.LANES + ["zu ɪz vɛri izi"] * dt.LANES
    seeds = np.arange(1, len(texts) + 1, dtype=np.uint32)
    pitch = np.linspace(90.0, 180.0, len(texts))
    out = {}
    for dead_terms in (1, 0):
        bp = eng.BatchPlayer(dt.SR, mode=0)
        for k, v in FLAT.items():
            bp.setOption(k, v)
        bp.setOption("sort", 0)
        bp.setOption("dead_terms", dead_terms)
        bp.setIpa(texts, basePitch=pitch, noiseSeed=seeds)
        bp.synthesize()
        pcm, start = bp.readAll()
        frames = [bp.frames(u) for u in (0, dt.LANES)] if dead_terms else None
        out[dead_terms] = (pcm.copy(), start, bp.kernelInfo(), frames, [bp.getLastIndex(u) for u in range(len(texts))])
        bp.close()
    got, start, info, frames, last = out[1]
    assert info["tracked_utterances"] == len(texts), info
    want = dt.waves(1, ("parallel1", "turbulence"))
    for k, v in dt.waves(1, dt.TERMS).items():
        want[k] += v
    assert counts(info) == want and want["waves_without_parallel1"] == 2, counts(info)
    assert not any(counts(out[0][2]).values())
    assert got.tobytes() == out[0][0].tobytes() and last == out[0][4]
    # the oracle on the frames as they are resident, for one utterance of each text
    for u, (fr, m, f, ix, nu) in zip((0, dt.LANES), frames):
        assert (fr[nu == 0][:, 6] != 0).any() == (u == 0) and not fr[:, 3].any() and not fr[:, 37].any()
        b = dict(frames=fr, min=m, fade=f, index=ix, isnull=nu, frame_start=np.array([0, len(m)], np.int64), seeds=seeds[u:u + 1])
        exp, exp_start, _ = oracle.batch_synthesize(dt.SR, b, threads=1)
        mine = got[start[u]:start[u + 1]]
        assert len(mine) == len(exp) and np.array_equal(mine, exp), (u, int(np.count_nonzero(mine != exp[:len(mine)])))
