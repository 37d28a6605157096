"""The vocal-tract frequency response (include/speechPlayer_batch.h: speechPlayer_frameResponse; nvspeechplayer_amd.frameResponse;
csrc/klatt_response.h) on the host.

`closed_form` restates the header's definition in numpy -- complex128, the C library's exp and cos -- and `impulse_responses` restates
the reference's CascadeFormantGenerator::getNext / ParallelFormantGenerator::getNext (src/speechWaveGenerator.cpp:139-182) sample by
sample on a frozen frame.  The first test ties the two together (the DTFT of the impulse response is the closed form), the a == 0 rule and
the cfN0 == 0 FIR form included; the second holds speechPlayer_frameResponse to the closed form within `bounded_response`'s forward error
bound, which is built from the roundings the definition counts and never from the output under test.  tests/test_gpu_response.py holds the
device to both.  No GPU is needed here."""
import numpy as np
import pytest

from tests import scenarios

SR = 22050
U = 2.0 ** -53                       # the unit roundoff of binary64: one rounding is at most U relative, 1 ulp at most 2 U
RES_F = [13, 14, 12, 11, 10, 9, 8, 7, 25, 26, 27, 28, 29, 30]      # N0 (anti), NP, c6 .. c1, p1 .. p6 (reference :149-156, :173-178)
RES_B = [21, 22, 20, 19, 18, 17, 16, 15, 31, 32, 33, 34, 35, 36]
CANP, PA1, BYPASS, PREGAIN, OUTGAIN = 23, 37, 43, 44, 45
KINDS = ["cascade_re", "cascade_im", "cascade_mag", "cascade_db", "parallel_re", "parallel_im", "parallel_mag", "parallel_db"]
DB = 20.0 / np.log(10.0)             # 8.686: d(20 log10 m) = DB dm / m
LEFT_OUT = 1e-8                      # an element whose bound is beyond this (relative) says nothing and is left out ...
LEFT_OUT_MOST = 0.01                 # ... of at most this share of the elements


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def coefficients(frames, sr):
    """Resonator::setParams (reference :112-127) of the 14 resonators of frames [n, 47]: -> a, b, c, each [n, 14]."""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, 47)
    f, bw = frames[:, RES_F], frames[:, RES_B]
    r = np.exp(-np.pi / sr * bw)
    c = -(r * r)
    b = r * np.cos(np.pi * 2 / sr * -f) * 2.0
    a = 1.0 - b - c
    anti = np.zeros_like(a, dtype=bool)
    anti[:, 0] = f[:, 0] != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(anti, 1.0 / a, a)
    return inv, np.where(anti, b * -inv, b), np.where(anti, c * -inv, c)


def twiddles(freqs, sr):
    w = 2.0 * np.pi * np.asarray(freqs, dtype=np.float64) / sr
    return np.exp(-1j * w), np.exp(-2j * w)


def transfer_functions(frames, sr, freqs):
    """H_r of the 14 resonators at the bins: complex [n, 14, K].  N0 is the FIR a + b z1 + c z2; a pole resonator with a == 0 is silent."""
    a, b, c = (x[:, :, None] for x in coefficients(frames, sr))
    z1, z2 = twiddles(freqs, sr)
    with np.errstate(divide="ignore", invalid="ignore"):
        H = np.where(a == 0, 0.0, a / (1.0 - b * z1 - c * z2))
    H[:, 0] = (a + b * z1 + c * z2)[:, 0]
    return H


def closed_form(frames, sr, freqs, gain=False):
    """The definition: -> (C, P), complex [n, K]."""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, 47)
    H = transfer_functions(frames, sr, freqs)
    C = 0.5 * (1.0 + (H[:, 0] * H[:, 1] - 1.0) * frames[:, CANP, None])
    for r in range(2, 8):
        C = C * H[:, r]
    S = np.zeros_like(C)
    for k in range(6):
        S = S + (H[:, 8 + k] - 1.0) * frames[:, PA1 + k, None]
    P = 0.5 * (S + (1.0 - S) * frames[:, BYPASS, None])
    if gain:
        g = (frames[:, PREGAIN] * frames[:, OUTGAIN])[:, None]
        C, P = C * g, P * g
    return C, P


def kinds_of(C, P):
    """[n, 8, K]: the eight kinds of the header's table."""
    with np.errstate(divide="ignore"):
        rows = [f(x) for x in (C, P) for f in (np.real, np.imag, np.abs, lambda v: 20.0 * np.log10(np.abs(v)))]
    return np.stack(rows, axis=1)


def impulse_responses(frames, sr, n):
    """Resonator::resonate, CascadeFormantGenerator::getNext and ParallelFormantGenerator::getNext (reference :129-135, :147-158, :170-180)
    sample by sample on frozen frames [m, 47], fresh state, input = a unit impulse: -> (cascade [m, n], parallel [m, n])."""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, 47)
    m = len(frames)
    a, b, c = coefficients(frames, sr)
    p1, p2 = np.zeros((m, 14)), np.zeros((m, 14))

    def resonate(r, x):
        out = a[:, r] * x + b[:, r] * p1[:, r] + c[:, r] * p2[:, r]
        p2[:, r] = p1[:, r]
        p1[:, r] = x if r == 0 else out          # (the anti-resonator remembers its input: :133)
        return out

    ca, bypass = frames[:, CANP], frames[:, BYPASS]
    hc, hp = np.zeros((m, n)), np.zeros((m, n))
    for t in range(n):
        x = np.full(m, 1.0 if t == 0 else 0.0)
        i = x / 2.0
        out = i + (resonate(1, resonate(0, i)) - i) * ca
        for r in range(2, 8):
            out = resonate(r, out)
        hc[:, t] = out
        out = np.zeros(m)
        for k in range(6):
            out = out + (resonate(8 + k, i) - i) * frames[:, PA1 + k]
        hp[:, t] = out + (i - out) * bypass
    return hc, hp


# ---- the frames -----------------------------------------------------------------------------------------------------------------------
def random_frames(rng, n, floor=40.0):
    """Seeded frames with every bandwidth >= floor Hz (the impulse responses die out inside the window: see the DTFT test)."""
    f = np.zeros((n, 47))
    f[:, 7:13] = np.sort(rng.uniform(150, 5500, (n, 6)), axis=1)
    f[:, 13] = rng.uniform(100, 600, n) * (rng.random(n) < 0.6)
    f[:, 14] = rng.uniform(200, 500, n)
    f[:, 15:23] = rng.uniform(floor, 1000, (n, 8))
    f[:, CANP] = rng.uniform(0, 1, n) * (rng.random(n) < 0.6)
    f[:, 25:31] = np.sort(rng.uniform(150, 5500, (n, 6)), axis=1)
    f[:, 31:37] = rng.uniform(floor, 1000, (n, 6))
    f[:, 37:43] = rng.uniform(0, 1, (n, 6))
    f[:, BYPASS] = rng.uniform(0, 1.1, n)
    f[:, PREGAIN] = rng.uniform(0, 1.5, n)
    f[:, OUTGAIN] = rng.uniform(0.2, 2.5, n)
    f[:, 0] = rng.uniform(60, 300, n)
    return f


def edge_frames():
    """The all-zero frame (sample 0, silence: every a == 0); /a/ with cfN0 = 0 and caNP = 1 (the anti-resonator keeps the resonator's
    coefficients, in FIR form), once with its bandwidth and once with cbN0 = 0 as well (a = 0, b = 2, c = -1: the FIR 2 z1 - z2)."""
    ref = scenarios.Ref()
    fir = scenarios.vowel_frame(ref, "a", 120.0)
    fir[13], fir[21], fir[CANP] = 0.0, 90.0, 1.0
    bare = fir.copy()
    bare[21] = 0.0
    return np.stack([np.zeros(47), fir, bare])


def response_frames():
    """The 49 phoneme frames of tests/golden/ref_frames.npz, the edge frames, 24 seeded random frames."""
    return np.concatenate([scenarios.Ref().frames, edge_frames(), random_frames(np.random.default_rng(31), 24)])


# ---- the forward error bound ----------------------------------------------------------------------------------------------------------
def bounded_response(frames, sr, freqs, gain=False):
    """closed_form's eight kinds [n, 8, K] and, alongside, a bound [n, 8, K] on |the product's value - this value|, to first order in U,
    and that bound relative to the largest magnitude of the branch over the frame's bins (RE, IM, MAG) or to the magnitude itself (DB).
    Both sides round, so every rounding is counted twice (the factor 2 in front of U below); one rounding is U relative, 1 ulp is 2 U.

    Coefficients (klatt_math.h states 1 ulp for its exp, 1.5 ulp for its cos; the C library's are within 1 ulp; counted as 1 and 1.5):
      ex = (-pi / sr) bw and th = (2 pi / sr) (-f) carry 3 roundings (pi, the quotient, the product): 3 U relative on the argument,
      rad = exp(ex):        2 U + 3 U |ex| relative
      cs  = cos(th):        3 U |cs| + 3 U |th| absolute (|sin| <= 1)
      c   = -(rad rad):     |c| (2 rel(rad) + U)
      b   = rad cs 2:       |b| (rel(rad) + U) + 2 rad abs(cs)
      a   = 1 - b - c:      e_b + e_c + U |1 - b| + U |a|
      the anti-resonator with cfN0 != 0:  a' = 1 / a: e_a / a^2 + U |a'|;   c' = c (-a'): |c| e_a' + |a'| e_c + U |c'|;   b' likewise.
    Twiddles: w = 2 pi f / sr carries 2 roundings, so z1 = e^(-i w) is off by 2 U w in phase and 3 U in its two rounded components
      (1 ulp each: 2 sqrt(2) U), z2 by twice the phase.
    A pole resonator H = a / D, D = 1 - b z1 - c z2:
      e_D = e_b + e_c + |b| e_z1 + |c| e_z2 + 5 U (1 + |b| + |c|)     (re: two products, two differences: (2 + 3 |b| + 2 |c|) U; im: two
            products, one sum: (2 |b| + 2 |c|) U)
      rel(H) = e_a / |a| + e_D / |D| + 5 U      (the quotient: two squares and their sum 2 U, the division U, the product U; the
            restatement's complex division is counted the same).  e_D / |D| is where the condition (1 + |b| + |c|) / |D| enters.
    The FIR N0 = a + b z1 + c z2:   e = e_a + e_b + e_c + |b| e_z1 + |c| e_z2 + 5 U (|a| + |b| + |c|)
    A complex product x y, written out:   |x| e_y + |y| e_x + 3 U |x| |y|      (each component two products and a sum)
    Cascade:  T = N0 NP;   X = 0.5 (1 + (T - 1) caNP):  0.5 |caNP| e_T + U (2 |caNP| (|T| + 1) + 2 |X|)     (a difference, a product and a
              sum in the real part, a product in the imaginary part; the halving is exact)
              C = X H6 .. H1, relatively:  e_X prod |H_r| + |C| sum_r (rel(H_r) + 3 U);   exactly zero when a factor is silent.
    Parallel, absolutely:  term_k = (H_k - 1) pa_k:  |pa_k| (e_H + 2 U |H_k - 1|) + 2 U |term_k|     (per component a difference and a product)
              S = their sum from zero:  sum e_term + 2 U sum_k |S_k| over the partial sums
              P = 0.5 (S + (1 - S) bypass):  0.5 (1 + |bypass|) e_S + U (2 |bypass| (|S| + 1) + 2 |P|)
    gain:     times g = pre out: |g| e + 2 U |x g|
    Kinds:    RE, IM: e;   MAG: e + 2 U |x| (two squares, a sum and a root: 1.5 U; the restatement's hypot: 1 ulp);
              DB: DB e_mag / |x| + 4 ulp of the value (the logarithm and the product by 20, on both sides)."""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1, 47)
    freqs = np.asarray(freqs, dtype=np.float64)
    f, bw = frames[:, RES_F], frames[:, RES_B]
    with np.errstate(divide="ignore", invalid="ignore"):
        ex, th = -np.pi / sr * bw, np.pi * 2 / sr * -f
        rad, cs = np.exp(ex), np.cos(th)
        rel_rad = (2 + 3 * np.abs(ex)) * U
        abs_cs = 3 * U * (np.abs(cs) + np.abs(th))
        c = -(rad * rad); e_c = np.abs(c) * (2 * rel_rad + U)
        b = rad * cs * 2.0; e_b = np.abs(b) * (rel_rad + U) + 2 * rad * abs_cs
        a = 1.0 - b - c; e_a = e_b + e_c + U * np.abs(1.0 - b) + U * np.abs(a)
        anti = np.zeros_like(a, dtype=bool)
        anti[:, 0] = f[:, 0] != 0
        ai = 1.0 / a; e_ai = e_a / (a * a) + U * np.abs(ai)
        ci = c * -ai; e_ci = np.abs(c) * e_ai + np.abs(ai) * e_c + U * np.abs(ci)
        bi = b * -ai; e_bi = np.abs(b) * e_ai + np.abs(ai) * e_b + U * np.abs(bi)
        a, b, c = np.where(anti, ai, a), np.where(anti, bi, b), np.where(anti, ci, c)
        e_a, e_b, e_c = 2 * np.where(anti, e_ai, e_a), 2 * np.where(anti, e_bi, e_b), 2 * np.where(anti, e_ci, e_c)      # (both sides)
        a, b, c, e_a, e_b, e_c = (x[:, :, None] for x in (a, b, c, e_a, e_b, e_c))
        w = 2.0 * np.pi * freqs / sr
        z1, z2 = np.exp(-1j * w), np.exp(-2j * w)
        e_z1, e_z2 = 2 * (2 * np.abs(w) + 3) * U, 2 * (4 * np.abs(w) + 3) * U
        D = 1.0 - b * z1 - c * z2
        e_D = e_b + e_c + np.abs(b) * e_z1 + np.abs(c) * e_z2 + 2 * 5 * U * (1 + np.abs(b) + np.abs(c))
        silent = np.broadcast_to(a == 0, D.shape)
        H = np.where(silent, 0.0, a / D)
        e_H = np.where(silent, 0.0, np.abs(H) * (e_a / np.abs(a) + e_D / np.abs(D) + 2 * 5 * U))
        H[:, 0] = (a + b * z1 + c * z2)[:, 0]
        e_H[:, 0] = (e_a + e_b + e_c + np.abs(b) * e_z1 + np.abs(c) * e_z2 + 2 * 5 * U * (np.abs(a) + np.abs(b) + np.abs(c)))[:, 0]
        aH = np.abs(H)
        # cascade
        ca = frames[:, CANP, None]
        T = H[:, 0] * H[:, 1]
        e_T = aH[:, 0] * e_H[:, 1] + aH[:, 1] * e_H[:, 0] + 2 * 3 * U * aH[:, 0] * aH[:, 1]
        X = 0.5 * (1.0 + (T - 1.0) * ca)
        e_X = 0.5 * np.abs(ca) * e_T + 2 * U * (2 * np.abs(ca) * (np.abs(T) + 1) + 2 * np.abs(X))
        C, tail, rel = X, np.ones_like(aH[:, 0]), np.zeros_like(aH[:, 0])
        for r in range(2, 8):
            C = C * H[:, r]
            tail = tail * aH[:, r]
            rel = rel + np.where(aH[:, r] == 0, 0.0, e_H[:, r] / np.where(aH[:, r] == 0, 1.0, aH[:, r])) + 2 * 3 * U
        e_C = np.where(tail == 0, 0.0, e_X * tail + np.abs(C) * rel)
        # parallel
        S, e_S = np.zeros_like(C), np.zeros_like(e_C)
        for k in range(6):
            pa = frames[:, PA1 + k, None]
            term = (H[:, 8 + k] - 1.0) * pa
            S = S + term
            e_S = e_S + np.abs(pa) * (e_H[:, 8 + k] + 2 * 2 * U * np.abs(H[:, 8 + k] - 1.0)) + 2 * 2 * U * np.abs(term) + 2 * 2 * U * np.abs(S)
        bp = frames[:, BYPASS, None]
        P = 0.5 * (S + (1.0 - S) * bp)
        e_P = 0.5 * (1 + np.abs(bp)) * e_S + 2 * U * (2 * np.abs(bp) * (np.abs(S) + 1) + 2 * np.abs(P))
        if gain:
            g = (frames[:, PREGAIN] * frames[:, OUTGAIN])[:, None]
            e_C, e_P = np.abs(g) * e_C + 2 * 2 * U * np.abs(C * g), np.abs(g) * e_P + 2 * 2 * U * np.abs(P * g)
            C, P = C * g, P * g
        value = kinds_of(C, P)
        bound, rel = np.zeros_like(value), np.zeros_like(value)
        for base, x, e in ((0, C, e_C), (4, P, e_P)):
            m = np.abs(x)
            e_m = e + 2 * 2 * U * m
            top = m.max(axis=1)[:, None]
            bound[:, base] = e; bound[:, base + 1] = e; bound[:, base + 2] = e_m
            # (a magnitude of exactly zero: -inf dB, exact where the zero is exact -- a silent factor, gains of zero -- and unbounded else)
            bound[:, base + 3] = np.where(m == 0, np.where(e_m == 0, 0.0, np.inf), DB * e_m / m + 4 * np.spacing(np.abs(value[:, base + 3])))
            for q, b in ((0, e), (1, e), (2, e_m)):
                rel[:, base + q] = np.where(b == 0, 0.0, b / top)
            rel[:, base + 3] = np.where(m == 0, np.where(e_m == 0, 0.0, np.inf), e_m / m)
    return value, bound, rel


def within(got, value, bound, rel):
    """got [n, 8, K] against bounded_response's triple.  -> (elements that miss their bound, elements left out, elements).  An element is
    left out when its bound says nothing: relative to the largest magnitude of its branch over the frame's bins (RE, IM, MAG), or to
    its own magnitude (DB), beyond LEFT_OUT.  Where the restatement is exact (a bound of zero: a silent factor gives 0, and -inf dB) so is
    the product."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == value.shape == bound.shape == rel.shape and not np.isnan(bound).any() and not np.isnan(value).any()
    left_out = ~(rel <= LEFT_OUT)
    with np.errstate(invalid="ignore"):
        miss = np.where(bound == 0, got != value, ~(np.abs(got - value) <= bound))
    return int((miss & ~left_out).sum()), int(left_out.sum()), int(value.size)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def test_the_dtft_of_the_reference_recurrence_is_the_closed_form():
    """8192 samples of the impulse response of the frozen network, transformed at 0, Nyquist and 31 bins between, against closed_form:
    within 1e-9 of the branch's largest magnitude over the bins.  Where that comes from, per unit of that magnitude:
      truncation   a bandwidth of 37.5 Hz (the golden frames' narrowest; the random ones: 40) decays by exp(-pi 37.5 / 22050) per sample,
                   1e-19 over 8192 samples; asserted below on the responses themselves: the last 64 samples are below 1e-14, and what
                   follows them is a geometric tail of ratio <= 0.9947: below 1e-14 / 0.0053 = 2e-12
      summation    8192 terms: <= 8192 U sum |h| = 9.1e-13 sum |h|; the phase w n of a term is off by <= 8192 pi 2 U = 5.8e-12:
                   together <= 6.7e-12 sum |h|, and sum |h| is asserted below 100: 6.7e-10
      recurrence   a sample of a resonator is three products and two sums of earlier samples: its rounding errors pass through the same
                   filters as the signal, <= 14 resonators x 5 U x sum |h| = 8e-13
    -- 7e-10 in all, under the 1e-9 allowed."""
    frames = response_frames()
    n = 8192
    freqs = np.linspace(0.0, SR / 2.0, 33)
    hc, hp = impulse_responses(frames, SR, n)
    C, P = closed_form(frames, SR, freqs)
    E = np.exp(-1j * np.outer(2.0 * np.pi * freqs / SR, np.arange(n)))
    for name, h, want in (("cascade", hc, C), ("parallel", hp, P)):
        got = h @ E.T
        top = np.abs(want).max(axis=1)
        live = top > 0
        assert np.abs(h[live, -64:]).max(axis=1).max() <= 1e-14 * top[live].min(), name
        assert (np.abs(h[live]).sum(axis=1) <= 100 * top[live]).all(), name
        assert not h[~live].any() and not got[~live].any(), name        # the all-zero frame: silent
        assert (np.abs(got - want).max(axis=1) <= 1e-9 * top).all(), (name, float((np.abs(got - want).max(axis=1) / np.maximum(top, 1e-300)).max()))
    # what the edge frames are there for
    a, b, c = coefficients(frames[49:52], SR)
    assert not a[0].any() and not C[49].any() and np.array_equal(P[49], np.zeros(33))
    assert a[1, 0] == 1.0 - b[1, 0] - c[1, 0] and b[1, 0] > 0 and (a[2, 0], b[2, 0], c[2, 0]) == (0.0, 2.0, -1.0)
    assert np.abs(C[51]).min() > 0        # (N0 with a == 0 is no silent resonator: it is a FIR)


def test_frame_response_is_within_the_forward_error_bound_of_the_restatement():
    import nvspeechplayer_amd as eng
    frames = response_frames()
    freqs = np.linspace(0.0, SR / 2.0, 129)
    golden = slice(0, 49)
    for gain in (False, True):
        value, bound, rel = bounded_response(frames, SR, freqs, gain)
        got = eng.frameResponse(frames, SR, 129, list(range(8)), gain=gain)
        assert got.shape == (len(frames), 8, 129) and got.dtype == np.float64
        miss, left_out, total = within(got, value, bound, rel)
        print("gain %d: %d of %d elements left out, %d miss their bound; median relative bound %.3g" % (gain, left_out, total, miss, float(np.median(rel))))
        assert miss == 0 and left_out <= LEFT_OUT_MOST * total, (gain, miss, left_out, total)
        miss, left_out, total = within(got[golden], value[golden], bound[golden], rel[golden])
        assert miss == 0 and left_out <= LEFT_OUT_MOST * total, ("golden", gain, miss, left_out, total)
    # the condition of the phoneme frames, checked here: below 8e3 per resonator, so their bounds are near 1e-11
    a, b, c = (x[golden, 1:, None] for x in coefficients(frames[golden], SR))
    z1, z2 = twiddles(freqs, SR)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(a == 0, 0.0, (1 + np.abs(b) + np.abs(c)) / np.abs(1.0 - b * z1 - c * z2))
    assert cond.max() < 8e3, float(cond.max())
    value, bound, rel = bounded_response(frames[golden], SR, freqs)
    assert np.median(rel[:, [2, 6]]) < 1e-11 and rel[:, [2, 6]].max() < 1e-9, (float(np.median(rel[:, [2, 6]])), float(rel[:, [2, 6]].max()))


def test_kinds_repeat_and_the_defaults():
    import nvspeechplayer_amd as eng
    frames = response_frames()[:52]
    every = eng.frameResponse(frames, SR, 17, list(range(8)))
    pick = eng.frameResponse(frames, SR, np.linspace(0.0, SR / 2.0, 17), ["parallel_db", "cascade_re", "parallel_db", 2])
    assert np.array_equal(pick.view(np.uint64), every[:, [7, 0, 7, 2]].view(np.uint64))
    default = eng.frameResponse(frames, SR, 17)
    assert np.array_equal(default.view(np.uint64), every[:, [3, 7]].view(np.uint64))
    one = eng.frameResponse(frames[7], SR, [1000.0], "cascade_mag")
    assert one.shape == (1, 1, 1) and one[0, 0, 0] == eng.frameResponse(frames[7:8], SR, [0.0, 1000.0], [2])[0, 0, 1]
    gained = eng.frameResponse(frames, SR, 17, [0, 1, 4, 5], gain=True)
    assert np.array_equal(gained, every[:, [0, 1, 4, 5]] * (frames[:, PREGAIN] * frames[:, OUTGAIN])[:, None, None])
    # MAG and DB from RE and IM, as the header has them; the all-zero frame: 0 and -inf
    with np.errstate(divide="ignore"):
        assert np.array_equal(every[:, 2], np.sqrt(every[:, 0] * every[:, 0] + every[:, 1] * every[:, 1]))
        assert np.allclose(every[:, 3], 20.0 * np.log10(every[:, 2]), rtol=1e-15, atol=0, equal_nan=True)
    assert not every[49, [0, 1, 2, 4, 5, 6]].any() and np.isneginf(every[49, [3, 7]]).all()
    # another rate is another response
    assert not np.array_equal(eng.frameResponse(frames, 16000, [500.0], [2]), eng.frameResponse(frames, SR, [500.0], [2]))


def test_refusals_and_shapes():
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    frames = np.ascontiguousarray(response_frames()[:3])
    freqs = np.array([0.0, 100.0, 11025.0])
    kinds = np.array([0, 7], np.int32)
    out = np.full(3 * 2 * 3 + 1, -7.0)

    def call(fr=frames.ctypes.data, n=3, sr=SR, fq=freqs, nf=3, ks=kinds, nk=2, gain=0, o=out.ctypes.data):
        return L.speechPlayer_frameResponse(fr, n, sr, None if fq is None else fq.ctypes.data, nf, None if ks is None else ks.ctypes.data, nk, gain, o)

    refused = dict(kind_8=dict(ks=np.array([0, 8], np.int32)), kind_negative=dict(ks=np.array([-1, 0], np.int32)), no_kinds=dict(nk=0),
                   negative_kinds=dict(nk=-1), null_kinds=dict(ks=None), no_frequencies=dict(nf=0), too_many_frequencies=dict(nf=4097),
                   null_frequencies=dict(fq=None), nan_frequency=dict(fq=np.array([0.0, np.nan, 1.0])),
                   infinite_frequency=dict(fq=np.array([0.0, 1.0, np.inf])), negative_frames=dict(n=-1), no_frames=dict(fr=None),
                   no_output=dict(o=None), rate_0=dict(sr=0))
    for name, kw in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == 1 and b"frameResponse" in L.speechPlayer_lastError(), name
        assert (out == -7.0).all(), name
    assert call(n=0) == 0 and call(n=0, fr=None, o=None) == 0 and (out == -7.0).all()
    assert call() == 18 and L.speechPlayer_lastErrorCode() == 0 and out[-1] == -7.0
    assert np.array_equal(out[:18].reshape(3, 2, 3).view(np.uint64), eng.frameResponse(frames, SR, freqs, [0, 7]).view(np.uint64))
    many = np.linspace(0.0, 11025.0, 4096)
    assert eng.frameResponse(frames, SR, 4096, [2]).shape == (3, 1, 4096)
    assert np.array_equal(eng.frameResponse(frames, SR, 4096, [2]), eng.frameResponse(frames, SR, many, [2]))
    assert eng.frameResponse(np.zeros((0, 47)), SR, 5).shape == (0, 2, 5)
    for bad, err in ((dict(frequencies=0), ValueError), (dict(frequencies=4097), ValueError), (dict(frequencies=[1.0, float("nan")]), ValueError),
                     (dict(frequencies=[]), ValueError), (dict(kinds=[]), ValueError), (dict(kinds=[8]), ValueError), (dict(kinds="cascade"), KeyError)):
        kw = dict(frequencies=5, kinds=[0])
        kw.update(bad)
        with pytest.raises(err):
            eng.frameResponse(frames, SR, **kw)
    with pytest.raises(ValueError):
        eng.frameResponse(np.zeros((2, 46)), SR, 5)
