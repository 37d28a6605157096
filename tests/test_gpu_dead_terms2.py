"""The flat stages' bodies without the second set of dead terms -- the source stage without the nasal pair, the final stage without
parallel 5 (and 6), the parallel stage without parallel 1..4 (option "dead_terms", csrc/klatt_systolic.h) -- against the oracle and
against the general bodies, on the batches of tests/dead_terms2.py.  Needs a GPU.

Per corpus and flat launch (as it is: one workgroup per CU; repeated in order past the CUs: two per CU, the instantiation bench.py
times): MODE_EXACT has 0 samples from the oracle and the bytes and index marks of "dead_terms" = 0; the same bytes with sorted lanes;
MODE_FAST stays within tests/test_gpu_parity.py's bar; kernelInfo()'s four new counts (stages_without_*) are exactly what the rule says
(tests/dead_terms2.dropped: a term goes when it is dead in every lane), zero under "dead_terms" = 0, and the three older counts
(waves_without_*) are what they were.
"""
import numpy as np
import pytest

from tests import dead_terms as dt
from tests import dead_terms2 as d2
from tests import oracle
from tests.test_gpu_dead_terms import FLAT, marked, run, tiles_past
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu

_built, _untiled = {}, {}


def built(name):
    """(corpus, the seven counts under "sort" = 0 and "dead_terms" = 1, the oracle's pcm, start): once per module run."""
    if name not in _built:
        c, waves = d2.build(name)
        assert len(c) <= 192 and int(np.diff(c.batch["frame_start"]).max()) <= 8
        exp, exp_start, _ = c.oracle(threads=8)
        assert int(np.diff(exp_start).max()) <= 4000
        exp.setflags(write=False)
        _built[name] = (c, d2.counts_of(waves), exp, exp_start)
    return _built[name]


def untiled(name):
    if name not in _untiled:
        got, start, info, last = run(marked(built(name)[0]), 0, 1, marks=True)
        got.setflags(write=False)
        _untiled[name] = (got, start, info, last)
    return _untiled[name]


def counts(info):
    return {k: v for k, v in info.items() if k.startswith(d2.PREFIX) or k.startswith("waves_without_")}


def test_the_counts_have_their_keys():
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(d2.SR)
    info = bp.kernelInfo()
    bp.close()
    assert sorted(k for k in info if k.startswith(d2.PREFIX)) == sorted(d2.PREFIX + t for t in d2.TERMS2)
    assert len([k for k in info if k.startswith("waves_without_")]) == 3


@pytest.mark.parametrize("launch", ["one_per_cu", "two_per_cu"])
@pytest.mark.parametrize("name", d2.CORPORA)
def test_corpus_in_both_flat_launches(name, launch):
    c0, want0, exp, exp_start = built(name)
    base, base_start, base_info, base_last = untiled(name)
    cus = base_info["cus"]
    assert base_info["wavefronts"] // 4 + 1 <= cus, base_info
    k = tiles_past(len(c0), cus) if launch == "two_per_cu" else 1
    c, want = (c0.tiled(k), {t: k * n for t, n in want0.items()}) if k > 1 else (c0, want0)
    b = marked(c)
    got, start, info, last = run(b, 0, 1, marks=True) if k > 1 else (base, base_start, base_info, base_last)
    print("%s %s: %d x %d utterances, %d samples; %d wavefronts on %d CUs, %d VGPRs; %s" % (
        name, launch, k, len(c0), len(got), info["wavefronts"], cus, info["vgprs"], counts(info)))
    assert (info["wavefronts"] // 4 + 1 > cus) == (launch == "two_per_cu"), info
    assert info["tracked_utterances"] == len(c) and info["scratch_bytes"] == 0, info
    want_start = np.concatenate([[0], np.cumsum(np.tile(np.diff(exp_start), k))]).astype(np.int64)
    assert np.array_equal(start, want_start)
    n = len(exp)
    for t in range(k):
        tile = got[t * n:(t + 1) * n]
        diff = c0.first_difference(tile, exp, exp_start)
        assert diff is None, "%s, tile %d of %d, dead_terms 1 against the oracle: %s" % (launch, t, k, diff)
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
    flips = compare(fast, np.tile(exp, k) if k > 1 else exp, "%s %s, MODE_FAST" % (name, launch))
    assert counts(fast_info) == want, fast_info
    print("%s %s MODE_FAST: %d one-LSB differences from the oracle" % (name, launch, flips))


def test_the_plan_reports_before_the_first_launch_and_every_launch_reads_the_option():
    """One player, the first mixed corpus set once: before the first launch kernelInfo() reports what the plan says (dead2_wave_counts,
    csrc/klatt_batchplan.h); launched under "dead_terms" 1, 0, 1 the stages count the same, zero, the same, with the oracle's bytes."""
    import nvspeechplayer_amd as eng
    c, want, exp, exp_start = built("mixed:0")
    b = c.batch
    bp = eng.BatchPlayer(d2.SR, mode=0)
    try:
        for k, v in FLAT.items():
            bp.setOption(k, v)
        bp.setOption("sort", 0)
        bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
        assert counts(bp.kernelInfo()) == want
        for launch, dead_terms in enumerate((1, 0, 1)):
            bp.setOption("dead_terms", dead_terms)
            bp.synthesize()
            pcm, start = bp.readAll()
            info = bp.kernelInfo()
            assert counts(info) == (want if dead_terms else {k: 0 for k in want}), (launch, counts(info))
            assert np.array_equal(start, exp_start) and c.first_difference(pcm, exp, start) is None
    finally:
        bp.close()


@pytest.mark.parametrize("sort", [0, 1])
def test_sparse_wavefront_replica_lanes_carry_their_bits(sort):
    """Five utterances in one wavefront, whose other lanes are replicas that carry their utterance's word: all five dead, the wavefront
    drops every term; one of the five with everything present, none."""
    for kinds in (["all2"] * 5, ["all2", "all2", d2.PRESENT, "all2", "all2"]):
        c, waves = d2.sparse_corpus(kinds)
        want = d2.counts_of(waves)
        assert (want[d2.PREFIX + "nasal"] == 1) == (d2.PRESENT not in kinds)
        exp, exp_start, _ = c.oracle(threads=4)
        got, start, info, _ = run(c.batch, 0, 1, sort=sort)
        ref, _, ref_info, _ = run(c.batch, 0, 0, sort=sort)
        assert info["tracked_utterances"] == 5, info
        assert np.array_equal(start, exp_start)
        assert c.first_difference(got, exp, start) is None
        assert got.tobytes() == ref.tobytes()
        assert counts(info) == want, counts(info)
        assert not any(counts(ref_info).values())


def test_ipa_text_batch():
    """From IPA text through setIpa, lanes in the given order: a wavefront of `hælou` drops the nasal pair and parallel 2..6 (and, as before,
    parallel 1 and the turbulence); a wavefront of a sentence with n and k drops none of the new four.  One utterance of each against the
    oracle on its resident frames."""
    import nvspeechplayer_amd as eng
    texts = ["hælou"] * d2.LANES + ["nou kin"] * d2.LANES
    seeds = np.arange(1, len(texts) + 1, dtype=np.uint32)
    pitch = np.linspace(90.0, 180.0, len(texts))
    out = {}
    for dead_terms in (1, 0):
        bp = eng.BatchPlayer(d2.SR, mode=0)
        for k, v in FLAT.items():
            bp.setOption(k, v)
        bp.setOption("sort", 0)
        bp.setOption("dead_terms", dead_terms)
        bp.setIpa(texts, basePitch=pitch, noiseSeed=seeds)
        bp.synthesize()
        pcm, start = bp.readAll()
        frames = [bp.frames(u) for u in (0, d2.LANES)] if dead_terms else None
        out[dead_terms] = (pcm.copy(), start, bp.kernelInfo(), frames, [bp.getLastIndex(u) for u in range(len(texts))])
        bp.close()
    got, start, info, frames, last = out[1]
    assert info["tracked_utterances"] == len(texts), info
    # what the resident frames say: hælou has no caNP and no pa2..pa6 anywhere; the other sentence has caNP (n) and pa2..pa6 (k)
    z = []
    for fr, m, f, ix, nu in frames:
        real = fr[nu == 0]
        z.append(tuple(p for p in range(47) if not real[:, p].any()))
    assert all(p in z[0] for p in d2.ZEROED["all2"] if p != d2.ASP)
    assert not any(p in z[1] for p in (d2.CA_NP, d2.PA2, d2.PA3, d2.PA4, d2.PA5, d2.PA6))
    want = d2.counts_of([[z[0]] * d2.LANES, [z[1]] * d2.LANES])
    assert all(want[d2.PREFIX + t] == 1 for t in d2.TERMS2 if d2.dropped([d2.ZEROED["all2"]])[0].count(t)), want
    assert counts(info) == want, (counts(info), want)
    assert not any(counts(out[0][2]).values())
    assert got.tobytes() == out[0][0].tobytes() and last == out[0][4]
    for u, (fr, m, f, ix, nu) in zip((0, d2.LANES), frames):
        b = dict(frames=fr, min=m, fade=f, index=ix, isnull=nu, frame_start=np.array([0, len(m)], np.int64), seeds=seeds[u:u + 1])
        exp, exp_start, _ = oracle.batch_synthesize(d2.SR, b, threads=1)
        mine = got[start[u]:start[u + 1]]
        assert len(mine) == len(exp) and np.array_equal(mine, exp), (u, int(np.count_nonzero(mine != exp[:len(mine)])))
