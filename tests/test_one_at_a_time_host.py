"""The one-parameter-at-a-time corpus (tests/one_at_a_time.py) on the host, no GPU needed: that it proves something -- every case
is audible in the oracle's PCM and nothing clips -- and that the planner sees in it what it is made of: per fade the mask of the one
kind that moves, per utterance the kinds word (speechPlayer_planTrackKinds), against tests/test_track_planning.py's table."""
import ctypes

import numpy as np
import pytest

from nvspeechplayer_amd import _native
from tests import one_at_a_time as oat
from tests import oracle
from tests.test_track_planning import PAIRS, RES_B, RES_F, expected

MIN_SAMPLES = 25        # samples that differ by more than 1 LSB between a case and the same list with B' = B
MAX_PEAK = 16000
# glottalOpenQuotient acts on the turbulence alone (reference src/speechWaveGenerator.cpp:76-82: it gates voiceTurbulenceAmplitude's noise):
# with the turbulence at 0 no value of it reaches the output.  The quiet variants keep it -- its kind still moves in the planner and
# in the kernels, and the PCM must not care -- and this test holds it to exactly that: not one sample may differ.
INAUDIBLE = {("quiet", 4), ("quiet_nasal_free", 4)}


def pcm_of(frames, seed=0):
    p = oracle.OraclePlayer(oat.SR, seed=seed)
    for fr, m, f in frames:
        p.queue(fr, m, f)
    out = p.drain()
    p.close()
    return out


@pytest.mark.parametrize("variant", list(oat.VARIANTS))
def test_every_case_is_audible_and_nothing_clips(variant):
    """For every parameter of the variant and both manners the oracle's PCM of the case differs from that of the same list with
    B' = B by more than 1 LSB in at least 25 samples (a condition on the inputs, not a measurement of the engine), and no case
    -- the edges cases included -- peaks at 16 000 or above (clipping would hide sensitivity and errors alike).
    Measured: noisy pb6 102 (move) / 95 (jump) samples, largest difference 3 / 4 LSB; quiet cb5 247 / 255, up to 15 LSB; quiet
    nasal-free vibratoSpeed 203 (jump); every other case more than 300.  INAUDIBLE: the one pair that cannot meet it."""
    check_audible(variant, {p for v, p in INAUDIBLE if v == variant})


def check_audible(variant, inaudible):
    """(the body of the test above, for any variant; `inaudible`: the parameters that must differ in NO sample)  Returns per manner the
    weakest audible parameter with its count, and the peak."""
    weakest, peak = {}, 0
    for manner in ("move", "jump"):
        plain = pcm_of(oat.case(oat.USUAL, manner, variant, unchanged=True))
        counts = {}
        for p in oat.params(variant):
            pcm = pcm_of(oat.case(p, manner, variant))
            assert len(pcm) == len(plain)
            d = np.abs(pcm.astype(np.int32) - plain.astype(np.int32))
            if p in inaudible:
                assert not d.any(), (variant, manner, oat.NAMES[p], int(np.count_nonzero(d)))
                continue
            counts[p] = (int(np.count_nonzero(d > 1)), int(d.max()))
            peak = max(peak, int(np.abs(pcm.astype(np.int32)).max()))
        p = min(counts, key=lambda p: counts[p])
        weakest[manner] = (oat.NAMES[p], counts[p][0])
        print("%s %s: weakest %s, %d samples differ by more than 1 LSB (largest difference %d LSB)" % (
            variant, manner, oat.NAMES[p], counts[p][0], counts[p][1]))
        weak = {oat.NAMES[p]: c for p, c in counts.items() if c[0] < MIN_SAMPLES}
        assert not weak, (variant, manner, weak)
    for edge in range(oat.LANES):
        for p in (oat.USUAL, 45, 5):
            if p in oat.params(variant):
                peak = max(peak, int(np.abs(pcm_of(oat.case(p, "edges", variant, edge)).astype(np.int32)).max()))
    print("%s: peak %d" % (variant, peak))
    assert peak < MAX_PEAK
    return weakest, peak


def test_corpus_holds_every_parameter_in_every_manner():
    """Every (parameter, manner) pair of a variant is in its batch corpus, `move` and `jump` both in a pure wavefront (jump: one
    parameter per entry kind) and as the one intruder among 63 lanes that move cf1; a ragged wavefront has 64 timings; and
    changed() alters one parameter."""
    assert oat.params("noisy") == tuple(range(47))
    assert oat.params("quiet") == (0, 1, 2, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 44, 45, 46)
    assert oat.params("quiet_nasal_free") == (0, 1, 2, 4, 5, 7, 8, 9, 10, 11, 12, 15, 16, 17, 18, 19, 20, 44, 45, 46)
    for variant in oat.VARIANTS:
        check_corpus_shape(variant)


def check_corpus_shape(variant):
    """(the body of the test above, for any variant)  Returns the corpus."""
    c = oat.batch_corpus(variant)
    ps = set(oat.params(variant))
    have = {(p, m, comp) for p, m, comp, _, _ in c.what}
    assert {p for p, m, comp in have if (m, comp) == ("move", "pure")} == ps
    assert {p for p, m, comp in have if (m, comp) == ("move", "intruder")} == ps
    assert {p for p, m, comp in have if (m, comp) == ("jump", "intruder")} == ps
    assert {p for p, m, comp in have if (m, comp) == ("edges", "ragged")} == ps
    kinds = 0
    for p in {p for p, m, comp in have if (m, comp) == ("jump", "pure")}:
        kinds |= oat.kind_bits(p)
    full = 0
    for p in ps:
        full |= oat.kind_bits(p)
    assert kinds == full and {0, 46} <= {p for p, m, comp in have if (m, comp) == ("jump", "pure")}
    b = c.batch
    for w in range(len(c) // oat.LANES):
        lanes = range(w * oat.LANES, (w + 1) * oat.LANES)
        timing = {(b["min"][b["frame_start"][u]:b["frame_start"][u + 1]].tobytes(), b["fade"][b["frame_start"][u]:b["frame_start"][u + 1]].tobytes()) for u in lanes}
        comp = c.what[w * oat.LANES][2]
        assert all(c.what[u][2] == comp and c.what[u][4] == u % oat.LANES for u in lanes)
        assert len(timing) == (oat.LANES if comp == "ragged" else 1)
        if comp == "intruder":
            odd = [u for u in lanes if c.what[u][0] != oat.USUAL]
            assert len(odd) <= 1 and all(c.what[u][4] == c.what[u][0] % oat.LANES for u in odd)
    for p in ps:
        assert np.count_nonzero(oat.changed(p, variant) != oat.base(variant)) == 1
    fades = {int(f) for u in range(len(c)) if c.what[u][1] == "edges" for f in b["fade"][b["frame_start"][u]:b["frame_start"][u + 1]]}
    assert fades == set(oat.EDGE_FADES)
    return c


def plan_kinds(b):
    L = _native.load()
    nu, nf = len(b["frame_start"]) - 1, len(b["fade"])
    off = np.zeros(nf, np.uint64); mask = np.zeros(nf, np.uint32); tracked = np.zeros(nu, np.uint8); kinds = np.full(nu, 0xFFFFFFFF, np.uint32)
    entries = ctypes.c_ulonglong(0)
    frames = np.ascontiguousarray(b["frames"], np.float64)
    n = L.speechPlayer_planTrackKinds(nu, b["frame_start"].ctypes.data, frames.ctypes.data, b["fade"].ctypes.data, b["isnull"].ctypes.data, None, 16384,
                                      off.ctypes.data, mask.ctypes.data, tracked.ctypes.data, ctypes.byref(entries), kinds.ctypes.data)
    assert n > 0, _native.last_error()
    # the view changes no planning: speechPlayer_planTracks answers the same
    off2 = np.zeros(nf, np.uint64); mask2 = np.zeros(nf, np.uint32); tracked2 = np.zeros(nu, np.uint8); entries2 = ctypes.c_ulonglong(0)
    n2 = L.speechPlayer_planTracks(nu, b["frame_start"].ctypes.data, frames.ctypes.data, b["fade"].ctypes.data, b["isnull"].ctypes.data, None, 16384,
                                   off2.ctypes.data, mask2.ctypes.data, tracked2.ctypes.data, ctypes.byref(entries2))
    assert n2 == n and entries2.value == entries.value and np.array_equal(off, off2) and np.array_equal(mask, mask2) and np.array_equal(tracked, tracked2)
    return mask, tracked, kinds


def walked_kinds(b, masks, keys):
    """The kinds word by the rule of plan_tracks (csrc/klatt_trackplan.h), from the fade end points tests/test_track_planning.expected walks: what a fade moves,
    and what the first sample of a later fade sets to other values than the fade before it ended on."""
    shape = [p for r in range(14) for p in (RES_F[r], RES_B[r])] + [23, 41, 42, 43, 45, 24, 44, 37, 38, 39, 40, 1, 2, 3, 4, 5, 6]
    out = []
    for u in range(len(b["frame_start"]) - 1):
        word = 0
        for k in range(b["frame_start"][u], b["frame_start"][u + 1]):
            word |= masks[k]
            if k > b["frame_start"][u]:
                ended, begins = np.frombuffer(keys[k - 1][1]), np.frombuffer(keys[k][0])
                for i in np.flatnonzero(ended != begins):
                    word |= oat.kind_bits(shape[i])
        out.append(word)
    return out


@pytest.mark.parametrize("variant", list(oat.VARIANTS))
def test_masks_and_kinds_word_of_every_case(variant):
    """Per-fade masks (speechPlayer_planTracks) and the per-utterance kinds word (speechPlayer_planTrackKinds: what the flat stages get
    in UttDesc.flags) of every case of the corpus, against the parameter -> kind table of tests/test_track_planning.py.
    move: the fade into B' and the fade back have exactly the kind(s) of p in their mask (none for the pitches).  jump: the fade out
    of silence has the gain kinds alone.  Either way the word holds the kinds of p and the gain kinds the silence fades move, and
    nothing else: in jump only its second term -- what a fade's first row re-sets -- can have put the kind of p there."""
    check_masks_and_kinds(oat.batch_corpus(variant), variant)
    # every one of the 24 kinds is some parameter's, and the noisy variant reaches them all
    if variant == "noisy":
        every = 0
        for p in range(1, 46):
            assert oat.kind_bits(p) != 0
            every |= oat.kind_bits(p)
        assert every == (1 << 24) - 1


def check_masks_and_kinds(c, variant):
    """(the body of the test above, for any variant's batch corpus)  Returns (mask per frame, kinds word per utterance)."""
    b = c.batch
    mask, tracked, kinds = plan_kinds(b)
    assert tracked.all()
    masks, keys = expected(b["frame_start"], b["frames"], b["fade"], b["isnull"])
    assert [int(m) for m in mask] == masks
    assert [int(k) for k in kinds] == walked_kinds(b, masks, keys)
    gain = oat.kind_bits(44)
    assert gain == (1 << 17) | (1 << 23) and oat.kind_bits(45) == 1 << 16 and oat.kind_bits(0) == 0 == oat.kind_bits(46)
    seen = set()
    for u in range(len(c)):
        p, manner = c.what[u][:2]
        m = [int(x) for x in mask[b["frame_start"][u]:b["frame_start"][u + 1]]]
        own = oat.kind_bits(p)
        assert len(m) == 4
        if manner == "jump":
            assert m == [gain, gain, gain, gain], c.describe(u)
        else:
            assert m == [gain, own, own, gain], c.describe(u)
        assert int(kinds[u]) == own | gain, c.describe(u)
        seen.add((p, manner))
    assert seen == {(p, manner) for p in oat.params(variant) for manner in oat.MANNERS}
    return mask, kinds


def test_kinds_word_of_utterances_that_get_no_tracks():
    """speechPlayer_planTrackKinds answers 0 for an utterance that is not tracked (not eligible, or over the budget), and takes a NULL kinds."""
    c = oat.Corpus("noisy")
    oat.add_pure(c, 9, "move")
    b = c.finish().batch
    L = _native.load()
    nu = len(c)
    el = (np.arange(nu) % 3 != 0).astype(np.uint8)
    kinds = np.full(nu, 0xFFFFFFFF, np.uint32); tracked = np.zeros(nu, np.uint8)
    frames = np.ascontiguousarray(b["frames"], np.float64)
    args = (nu, b["frame_start"].ctypes.data, frames.ctypes.data, b["fade"].ctypes.data, b["isnull"].ctypes.data)
    assert L.speechPlayer_planTrackKinds(*args, el.ctypes.data, 16384, None, None, tracked.ctypes.data, None, kinds.ctypes.data) > 0
    assert np.array_equal(tracked, el)
    assert np.array_equal(kinds, np.where(el != 0, oat.kind_bits(9) | oat.kind_bits(44), 0).astype(np.uint32))
    assert L.speechPlayer_planTrackKinds(*args, None, 0, None, None, tracked.ctypes.data, None, kinds.ctypes.data) == 0
    assert not tracked.any() and not kinds.any()
    assert L.speechPlayer_planTrackKinds(*args, None, 16384, None, None, None, None, None) > 0
    assert L.speechPlayer_planTrackKinds(2, None, None, None, None, None, 16384, None, None, None, None, None) == -1
