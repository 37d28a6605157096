"""The flat stages' bodies without dead terms (option "dead_terms", csrc/klatt_systolic.h) against the oracle and against the general
bodies, on the batches of tests/dead_terms.py.  Needs a GPU.

Per case: MODE_EXACT equals the oracle with 0 differing samples and equals the same batch under "dead_terms" = 0 byte for byte, index
marks included; MODE_FAST stays within tests/test_gpu_parity.py's bar; and kernelInfo() counts the wavefronts that dropped each term
-- as many as the case has wavefronts all of whose lanes are dead, none in a near miss, none under "dead_terms" = 0 -- so that a body
that silently never runs fails.  pa1 = -0.0 and voiceAmplitude = 0 sit on the dead side of their rules (zero of either sign; the
sum 0.0 + voice kept as an add) and are held to the same bytes.
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
