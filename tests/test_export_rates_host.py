"""The inputs of tests/test_gpu_export_rates.py and the host statements it compares the device with, at every sample rate
(tests/export_rates.py).  The batches hold what they claim -- the pure part's wavefronts are class-pure, the odd ones break them in one
lane, the edge part reaches every class -- and what the GPU tests take as the truth is held to something independent at the rate:
speechPlayer_resonatorCoefficients to the C library's formula in every class of exp and cos, speechPlayer_frameResponse to the closed
form within its forward error bound, the `stems` restatement to the oracle's PCM, and the source comparison to a tie-free subset.  No GPU."""
import hashlib

import numpy as np
import pytest

from tests import export_rates as X
from tests.export_rates import RATES, RES_B, RES_F
from tests.test_response_host import LEFT_OUT_MOST, bounded_response, within
from tests.test_source_host import PHASE, Sourced, source, ties
from tests.test_stems_host import OUTPUT, Stemmed, libm_coefficients, stems, to_pcm
from tests.test_timeline_host import utterance, walk

E_POLE = 2.0 ** -47


def test_the_edge_batch_is_what_it_was():
    """edge_batch is imported from tests/test_gpu_rates.py, not copied: the same function, the same draws.  The digest of its 22 050 Hz
    batch of 96, taken when this file was written."""
    b = X.edge_part(22050)
    h = hashlib.sha256()
    for k in ("frames", "min", "fade", "index", "isnull", "frame_start", "seeds"):
        h.update(np.ascontiguousarray(b[k]).tobytes())
    assert h.hexdigest() == EDGE_DIGEST_22050


EDGE_DIGEST_22050 = "263b2e1675e798966ed33893fa15db4e407f793f6b4ab821354f5b2a615ac0a7"


def pure_classes(sr, row):
    """The classes of every sample of pure row `row` but its first (cur(0) is the all-zero frame): (k [L - 1, 14], n [L - 1, 14], cur)."""
    b = X.parts(sr)["batch"]
    cur = walk(*utterance(b, row))[0]
    assert not cur[0].any() and len(cur) == X.lengths(b)[row]
    k, n = X.classes(cur[1:, list(RES_F)], cur[1:, list(RES_B)], sr)
    return k, n, cur


@pytest.mark.parametrize("sr", RATES)
def test_the_inputs_hold_what_they_claim(sr):
    """Pure part: on walk's frames, sample 0 aside, every low utterance has k = 0 and quadrant 0 in all 14 resonators on every sample
    (interpolation between two frames of a class stays in it), every upper one k = 0 and quadrant -1; the two odd ones leave their
    class in exactly one resonator, on the samples that their changed frame reaches, and are the only rows of their wavefronts that do;
    the rows' lengths do not increase (the stems kernel's stable sort by length leaves them where they are).  Edge part: its in-range
    frames reach exp's k = 0, -1, -2 and cos's quadrants -4 .. +1; a formant above Nyquist, a negative one, a bandwidth of 0, N0 at 0 Hz
    and an utterance beyond the documented range are there.  The restated subset has a witness of each."""
    p = X.parts(sr)
    b, kind = p["batch"], p["kind"]
    lens = X.lengths(b)
    pure = lens[:X.PURE_ROWS]
    assert (np.diff(pure) <= 0).all() and pure[0] == 1500 and pure[-1] >= 400 and len(set(pure[:64].tolist())) >= 60
    assert kind[X.LOW:X.UPPER] == ["low"] * 64 and kind[X.UPPER:X.THIRD] == ["upper"] * 64
    assert [r for r in range(X.THIRD, X.PURE_ROWS) if kind[r] != "low"] == [X.ODD_F, X.ODD_BW] and X.ODD_F % 64 == X.ODD_LANE
    assert X.PURE_ROWS % 64 != 0                                         # a ragged last wavefront
    for r in X.SHARED:
        assert p["list_of"][r] == p["list_of"][r - 1] and p["seeds"][r] != p["seeds"][r - 1]
    assert len(set(p["list_of"].tolist())) == len(p["list_of"]) - len(X.SHARED)
    fs = b["frame_start"]
    noisy = np.array([b["frames"][fs[r]:fs[r + 1]][:, [3, 6, 24]].any() for r in range(X.PURE_ROWS)])
    rows = np.array([r for r in range(X.PURE_ROWS) if r not in X.SHARED and r not in (X.ODD_F, X.ODD_BW)])
    assert np.array_equal(noisy[rows], rows % 2 == 1) and not b["frames"][:fs[X.PURE_ROWS], 1].any()
    assert set((fs[1:X.PURE_ROWS + 1] - fs[:X.PURE_ROWS]).tolist()) == {2, 3} and not b["isnull"][:fs[X.PURE_ROWS]].any()
    broken = {}
    for row in range(X.PURE_ROWS):
        k, n, cur = pure_classes(sr, row)
        want = -1.0 if kind[row] == "upper" else 0.0
        off = (k != 0) | (n != want)
        if off.any():
            broken[row] = off
    assert sorted(broken) == [X.ODD_F, X.ODD_BW]
    for row, (frame, param) in X.pure_part(sr)["odd"].items():
        off = broken[row]
        col = (RES_F.index(param) if param in RES_F else RES_B.index(param))
        assert off[:, col].any() and not np.delete(off, col, axis=1).any(), row
        k, n, cur = pure_classes(sr, row)
        assert (set(n[off[:, col], col].tolist()) == {-1.0}) if row == X.ODD_F else (set(k[off[:, col], col].tolist()) == {-1.0})
        # the copy differs from its original on a stretch that begins after frame A and ends before the utterance does
        orig = walk(*utterance(b, X.pure_part(sr)["original"][row]))[0]
        differ = np.flatnonzero((cur != orig).any(axis=1))
        assert len(cur) == len(orig) and 120 < differ[0] and differ[-1] < len(cur) - 16 and off[:, col].sum() < len(differ)
        assert p["seeds"][row] == p["seeds"][row - 1]
    # the edge part
    e = X.edge_part(sr)
    real = e["frames"][~e["isnull"].astype(bool)]
    inside = X.in_range(real, sr)
    k, n = X.classes(real[inside][:, list(RES_F)], real[inside][:, list(RES_B)], sr)
    assert {0.0, -1.0, -2.0} <= set(np.unique(k).tolist()) and {-4.0, -3.0, -2.0, -1.0, 0.0, 1.0} <= set(np.unique(n).tolist())
    f, bw = real[:, list(RES_F)], real[:, list(RES_B)]
    assert (f > sr / 2).any() and (f < 0).any() and (bw == 0).any() and (real[:, 13] == 0).any() and (real[:, 13] != 0).any()
    beyond = [u for u in range(X.EDGE_ROWS) if not X.in_range(X.utterance_frames(e, u), sr).all()]
    assert beyond == [17, 57]
    # the subset the restatements walk
    sub = X.restated_subset(sr)
    assert sub == sorted(set(sub)) and lens[sub].sum() < X.RESTATED_MOST and {kind[u] for u in sub} == {"low", "upper", "odd f", "odd bw", "edge"}
    fr = np.concatenate([X.utterance_frames(b, u) for u in sub if kind[u] == "edge"])
    assert X.in_range(fr, sr).all()
    k, n = X.classes(fr[:, list(RES_F)], fr[:, list(RES_B)], sr)
    assert (k == -2).any() and (n == -4).any()
    print("%d Hz: exp classes %s, cos quadrants %s; subset of %d utterances, %d samples" % (
        sr, sorted(set(np.unique(X.classes(f[inside], bw[inside], sr)[0]).astype(int).tolist())), sorted(set(np.unique(n).astype(int).tolist())), len(sub), lens[sub].sum()))


@pytest.mark.parametrize("sr", RATES)
def test_host_coefficients_against_the_c_library_in_every_class(sr):
    """speechPlayer_resonatorCoefficients against libm_coefficients (tests/test_stems_host.py) on every in-range (frequency, bandwidth)
    pair of both parts' real frames, all 14 resonators: exp's k = 0, -1, -2 and below, cos's quadrants -4 .. +1 and beyond, the margins.

    Pole resonators (and N0 at 0 Hz, which is not inverted): each of a, b, c within 2^-47 ABSOLUTE.  The arguments ex and th are
    formed by the same two operations on both sides, so no argument term enters.  Every bandwidth here is >= 0 (asserted), so
    rad = exp(ex) <= 1 and an ulp of it is at most 2^-53; klatt_math.h states <= 1 ulp for its exp over the whole validated range,
    whatever k (tests/test_device_math.py holds it to that per class), the C library's is within 1 ulp: |d rad| < 2 * 2^-53.  Its
    cos is within 1.5 ulp + 2^-90 in every quadrant, the C library's within 1 ulp, of a value <= 1: |d cs| < 2.5 * 2^-53 + 2^-90.
    b = rad cs 2 (|b| <= 2): 2 (|cs| d rad + rad d cs) < 9 * 2^-53, and the product's rounding on either side, 2^-54 each, doubled:
    < 11 * 2^-53.  c = -(rad rad) (|c| <= 1): 2 rad d rad < 4 * 2^-53 and two roundings of 2^-54: < 5 * 2^-53.  a = 1 - b - c
    (|1 - b| <= 3, |a| <= 4): d b + d c and two differences rounded on either side, half an ulp of a value below 4 each (2^-52):
    < (16 + 8) * 2^-53.  All below 64 * 2^-53 = 2^-47, in every class: nothing above depends on k or the quadrant.

    The anti-resonator with f != 0 inverts a: with E = 2^-47 and (a, b, c) the pole form by the C library,
      a' = 1 / a:     within E / (|a| (|a| - E)) (the reciprocals of two numbers E apart) + 2 * 2^-53 |a'| (the division, either side)
      b' = b (-a'):   within (|a'| + d a') E + |b| d a' + 2 * 2^-53 |b'|;   c' likewise.
    (Not relative to |b'|, as the 22 050 Hz test has it for formants below 5500 Hz: here b passes through zero at f = sr / 4.)"""
    from nvspeechplayer_amd.speechPlayer import resonatorCoefficients
    b = X.parts(sr)["lists"]
    real = b["frames"][~b["isnull"].astype(bool)]
    real = real[X.in_range(real, sr)]
    assert (real[:, list(RES_B)] >= 0).all() and len(real) > 800
    f, bw = real[:, list(RES_F)], real[:, list(RES_B)]
    # poles: resonators 1 .. 13, and N0 where its frequency is 0
    pf = np.concatenate([f[:, 1:].ravel(), f[f[:, 0] == 0, 0]])
    pbw = np.concatenate([bw[:, 1:].ravel(), bw[f[:, 0] == 0, 0]])
    got, want = resonatorCoefficients(pf, pbw, sr), libm_coefficients(pf, pbw, False, sr)
    worst = float(np.abs(got - want).max())
    assert np.all(np.isfinite(got)) and worst <= E_POLE, worst
    zero = f[:, 0] == 0
    assert zero.any() and np.array_equal(resonatorCoefficients(f[zero, 0], bw[zero, 0], sr, anti=True), resonatorCoefficients(f[zero, 0], bw[zero, 0], sr))
    # the anti-resonator
    af, abw = f[~zero, 0], bw[~zero, 0]
    got, want = resonatorCoefficients(af, abw, sr, anti=True), libm_coefficients(af, abw, True, sr)
    pole = libm_coefficients(af, abw, False, sr)
    a, bb, cc = np.abs(pole[:, 0]), np.abs(pole[:, 1]), np.abs(pole[:, 2])
    assert (a > 2 * E_POLE).all()
    inv = 1.0 / a
    d_inv = E_POLE / (a * (a - E_POLE)) + 2 * 2.0 ** -53 * inv
    tol = np.stack([d_inv, (inv + d_inv) * E_POLE + bb * d_inv + 2 * 2.0 ** -53 * np.abs(want[:, 1]),
                    (inv + d_inv) * E_POLE + cc * d_inv + 2 * 2.0 ** -53 * np.abs(want[:, 2])], axis=1)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= tol), float((np.abs(got - want) / tol).max())
    k, n = X.classes(pf, pbw, sr)
    print("%d Hz: %d pole pairs (k %d .. %d, quadrants %d .. %d), worst |difference| %.3g of %.3g allowed; %d anti-resonators, worst %.3g of their bound" % (
        sr, len(pf), k.min(), k.max(), n.min(), n.max(), worst, E_POLE, len(af), float((np.abs(got - want) / tol).max())))


@pytest.mark.parametrize("sr", RATES)
def test_frame_response_is_within_the_bound_of_the_restatement_at_the_rate(sr):
    """speechPlayer_frameResponse at the rate against bounded_response (tests/test_response_host.py) on the distinct real frames of both
    parts -- the out-of-range ones and the poles of bandwidth 0 among them -- at bins(sr), all eight kinds, gain off and on: no element
    misses its bound, and the bound says nothing (LEFT_OUT) for at most LEFT_OUT_MOST of them."""
    import nvspeechplayer_amd as eng
    b = X.parts(sr)["lists"]
    frames = b["frames"][~b["isnull"].astype(bool)].copy()
    frames[:, [0, 46]] = 0.0                                             # (the pitch does not enter the response)
    frames = np.unique(frames, axis=0)
    assert len(frames) > 800
    edge = X.edge_part(sr)
    edge = edge["frames"][~edge["isnull"].astype(bool)]
    for gain in (False, True):
        value, bound, rel = bounded_response(frames, sr, X.bins(sr), gain)
        got = eng.frameResponse(frames, sr, X.bins(sr), list(range(8)), gain=gain)
        miss, left_out, total = within(got, value, bound, rel)
        ev, eb, er = bounded_response(edge, sr, X.bins(sr), gain)
        e_left = int((~(er <= 1e-8)).sum())
        print("%d Hz, gain %d: %d distinct frames, %d of %d elements left out (share %.4f; the edge part's frames alone: %.4f), %d miss their bound" % (
            sr, gain, len(frames), left_out, total, left_out / total, e_left / er.size, miss))
        assert miss == 0 and left_out <= LEFT_OUT_MOST * total, (sr, gain, miss, left_out, total)


@pytest.mark.parametrize("sr", RATES)
def test_the_restatement_gives_the_oracles_pcm_on_every_sample_at_the_rate(sr):
    """`stems` with the C library's coefficients and P from source(), clipped and truncated, is the oracle's PCM on every sample of
    restated_subset(sr): what tests/test_gpu_export_rates.py compares the device's stems with bit for bit is right at this rate."""
    s = Stemmed(X.parts(sr)["batch"], sr)
    samples = 0
    for u in X.restated_subset(sr):
        cur = s.cur(u)
        st = stems(cur, source(cur, sr)[0][:, PHASE], s.seed(u), sr, libm_coefficients)
        want = s.pcm(u)
        assert len(st) == len(want), u
        differ = np.flatnonzero(to_pcm(st[:, OUTPUT]) != want)
        assert len(differ) == 0, (u, len(differ), int(differ[0]))
        samples += len(st)
    assert 50000 < samples < X.RESTATED_MOST


@pytest.mark.parametrize("sr", RATES)
def test_the_source_comparison_sets_nothing_aside(sr):
    """No sample of restated_subset(sr) is a tie (tests/test_source_host.py: ties): CYCLE, OPEN, the epochs' samples and the counts
    must be equal exactly, and check_batch stays as it is.  No rate's draw had a tie: export_rates.TIED is empty."""
    s = Sourced(X.parts(sr)["batch"], sr)
    vibrato = epochs = 0
    for u in X.restated_subset(sr):
        cur, cols, ep, xs = s.get(u)
        assert ties(cur, cols, xs) == (0, 0), (sr, u)
        vibrato += int((cur[:, 1] != 0).any()); epochs += len(ep)
    assert vibrato >= 3 and epochs > 100 and not X.TIED
