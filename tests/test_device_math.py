"""klatt_math.h's exp / cos / sin against mpmath on the host, and the device's results against the host's bit for bit.

tests/native/math_probe.hip compiles the header's KLATT_HD functions with the engine's own hipcc flags, once as they are (on the
device: Horner steps as inline v_fma_f64 with scalar constants) and once with -DKLATT_NO_SCALAR_CONSTANTS (the compiler's own
fused multiply-adds).  The arguments are the ones the coefficient code forms: ex = (-pi / sr) bw and th = (2 pi / sr) (-f) at every
sample rate the engine is used at, over the direct stages' eligibility bounds (|bw| <= 690 sr / pi, |f| <= 9900 sr / 2 pi), densely
around every reduction boundary and every class margin of the kernels (0.499 / 0.501: fade_classes, klatt_seeds), at the doubles
nearest the multiples of pi / 2, and uniformly over the header's stated domain.

CPU: the host results against mpmath at 128 bits, per function and reduction class, held to the bounds klatt_math.h states; the
share of results that differ from glibc's is printed, not asserted.  GPU: the device returns the host's bits on every argument, in
both builds; the predicates agree; each shortcut returns its full function's bits wherever its predicate holds.  Together these
carry the host's measured bounds over to the device.
"""
import ctypes
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "native", "math_probe.hip")
_HEADER = os.path.join(os.path.dirname(_HERE), "nvspeechplayer_amd", "csrc", "klatt_math.h")

FAST_EXP, FAST_COS, FAST_SIN, EXP_UNREDUCED, COS_UNREDUCED, COS_QUADRANT_M1, EXP_IS_UNREDUCED, COS_IS_UNREDUCED, COS_IS_QUADRANT_M1 = range(9)
FUNCTIONS = {"fast_exp": FAST_EXP, "fast_cos": FAST_COS, "fast_sin": FAST_SIN, "exp_unreduced": EXP_UNREDUCED,
             "cos_unreduced": COS_UNREDUCED, "cos_quadrant_m1": COS_QUADRANT_M1, "exp_is_unreduced": EXP_IS_UNREDUCED,
             "cos_is_unreduced": COS_IS_UNREDUCED, "cos_is_quadrant_m1": COS_IS_QUADRANT_M1}
# each shortcut, the predicate under which it must equal its full function, and that function
SHORTCUTS = ((EXP_UNREDUCED, EXP_IS_UNREDUCED, FAST_EXP), (COS_UNREDUCED, COS_IS_UNREDUCED, FAST_COS),
             (COS_QUADRANT_M1, COS_IS_QUADRANT_M1, FAST_COS))

RATES = (8000, 11025, 16000, 22050, 44100, 48000)
LOG2E = 1.4426950408889634074          # klatt::kLog2e
TWO_OVER_PI = 0.63661977236758134308   # klatt::kTwoOverPi
# pi to 60 digits: Fraction -> float rounds correctly, so k pi / 2 below is the double nearest the true multiple
_PI = Fraction("3.14159265358979323846264338327950288419716939937510582097494459")

# The bounds klatt_math.h states (measured on the argument sets below; ulp = 2^(e - 52) for 2^e <= |true value| < 2^(e + 1)).
EXP_MAX_ULP = 1.0
TRIG_MAX_ULP = 1.5              # cos and sin where |true value| >= TRIG_REL_FLOOR
TRIG_REL_FLOOR = 2.0 ** -30     # (nearer the zeros the reduction's absolute error dominates)
TRIG_MAX_ABS = 2.0 ** -90       # cos and sin: |error| <= TRIG_MAX_ULP ulp + TRIG_MAX_ABS everywhere in |t| <= 1e4


def _build(out, defines):
    from nvspeechplayer_amd import _native
    newest = max(os.path.getmtime(_SRC), os.path.getmtime(_HEADER))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # (as nvspeechplayer_amd/_native.py finds it)
        tmp = out + ".tmp.%d" % os.getpid()
        subprocess.check_call([hipcc] + _native.HIPCC_FLAGS + list(defines) + _native.LINK_FLAGS + ["-o", tmp, _SRC])
        os.replace(tmp, out)
    lib = ctypes.CDLL(out)
    for name in ("math_host", "math_device"):
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    return lib


_libs = {}


def probe(scalar_constants=True):
    """The probe library: the header as the engine compiles it, or (False) with -DKLATT_NO_SCALAR_CONSTANTS."""
    if scalar_constants not in _libs:
        name = "libmath_probe.so" if scalar_constants else "libmath_probe_nsc.so"
        _libs[scalar_constants] = _build(os.path.join(_HERE, "native", name), () if scalar_constants else ("-DKLATT_NO_SCALAR_CONSTANTS",))
    return _libs[scalar_constants]


def run(lib, fn, args, device=False):
    x = np.ascontiguousarray(args, dtype=np.float64)
    out = np.empty_like(x)
    rc = (lib.math_device if device else lib.math_host)(fn, x.ctypes.data, out.ctypes.data, len(x))
    assert rc == 0, "math_%s(%d): error %d" % ("device" if device else "host", fn, rc)
    return out


def _around(centers, steps, rel=0.0, n_rel=0, rng=None):
    """Every center, its `steps` neighbours on each side (ulp by ulp), and n_rel points within a relative `rel` of each."""
    lo = hi = np.asarray(centers, dtype=np.float64)
    out = [lo]
    for _ in range(steps):
        lo = np.nextafter(lo, -np.inf); hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    if n_rel:
        out.append((np.asarray(centers)[:, None] * (1.0 + rng.uniform(-rel, rel, (len(lo), n_rel)))).ravel())
    return np.concatenate(out)


def exp_arguments(n_sweep=150000, steps=512, n_rel=4096, n_uniform=600000, seed=1):
    """Arguments of fast_exp: ex = (-pi / sr) bw (klatt_engine.hip base_args, klatt_device.h coefficient_parts) at every rate for bw
    over [0, 690 sr / pi], bandwidths that put ex * log2e on +-0.5, +-1.5 and the class margins +-0.499 / +-0.501 (and bw
    over [0, sr / 4] once more), the same boundaries as plain arguments, and |x| <= 700 uniformly."""
    rng = np.random.default_rng(seed)
    parts = [np.array([0.0, -0.0])]
    bounds = [s * b for b in (0.5, 1.5, 0.499, 0.501, 1.499, 1.501) for s in (1, -1)]
    for sr in RATES:
        neg = -math.pi / sr
        top = 690.0 * sr / math.pi
        parts.append(neg * np.linspace(0.0, top, n_sweep))
        parts.append(neg * rng.uniform(0.0, top, n_sweep))
        parts.append(neg * rng.uniform(0.0, 0.25 * sr, n_sweep // 2))      # bandwidths of speech and a little beyond
        bws = np.array([b / LOG2E / neg for b in bounds if b < 0])      # (bandwidths are >= 0: only the negative side)
        parts.append(neg * _around(bws, steps // 8, 1e-9, n_rel // 8, rng))
    parts.append(_around(np.array(bounds) / LOG2E, steps, 1e-9, n_rel, rng))
    parts.append(_around(np.array(bounds) / LOG2E, 0, 3e-3, n_rel, rng))
    parts.append(rng.uniform(-700.0, 700.0, n_uniform))
    return np.concatenate(parts)


def multiples_of_half_pi(limit=1.0e4, neighbours=2):
    """The doubles nearest k pi / 2 for every k with |k pi / 2| <= limit, with `neighbours` doubles on each side."""
    kmax = int(limit / (math.pi / 2))
    centers = np.array([float(k * _PI / 2) for k in range(-kmax, kmax + 1)])
    return _around(centers, neighbours)


def trig_arguments(n_sweep=150000, steps=512, n_rel=4096, n_uniform=600000, seed=2):
    """Arguments of fast_cos / fast_sin: th = (2 pi / sr) (-f) at every rate for f over +-9900 sr / 2 pi, frequencies that put
    th * 2 / pi on +-0.5 ... +-2.5 and the class margins +-0.499 / +-0.501 / +-1.499 / +-1.501, the same boundaries as plain
    arguments, the doubles nearest every multiple of pi / 2 with two neighbours each side, and |t| <= 1e4 uniformly."""
    rng = np.random.default_rng(seed)
    parts = [np.array([0.0, -0.0])]
    bounds = [s * b for b in (0.5, 1.5, 2.5, 0.499, 0.501, 1.499, 1.501) for s in (1, -1)]
    for sr in RATES:
        two = (math.pi * 2) / sr
        top = 9900.0 * sr / (2.0 * math.pi)
        parts.append(two * -np.linspace(-top, top, n_sweep))
        parts.append(two * -rng.uniform(-top, top, n_sweep))
        parts.append(two * -rng.uniform(-0.3 * sr, 0.9 * sr, n_sweep // 4))      # formants of speech, above Nyquist and negative
        fs = np.array([-b / TWO_OVER_PI / two for b in bounds])
        parts.append(two * -_around(fs, steps // 8, 1e-9, n_rel // 8, rng))
    parts.append(_around(np.array(bounds) / TWO_OVER_PI, steps, 1e-9, n_rel, rng))
    parts.append(_around(np.array(bounds) / TWO_OVER_PI, 0, 3e-3, n_rel, rng))
    parts.append(multiples_of_half_pi())
    parts.append(rng.uniform(-1.0e4, 1.0e4, n_uniform))
    return np.concatenate(parts)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the host build against mpmath

def _ulp_of(y):
    """ulp of the exact value y (an mpmath number): 2^(e - 52) for 2^e <= |y| < 2^(e + 1), 2^-1074 below the normal range."""
    import mpmath
    m, e = mpmath.frexp(abs(y))          # |y| = m 2^e, 0.5 <= m < 1
    return math.ldexp(1.0, max(int(e) - 53, -1074))


def _errors(fn_mp, args, got):
    """Per result: error in ulp of the true value, absolute error, |true value|, ulp of the true value."""
    import mpmath
    n = len(args)
    ulps, abs_err, mag, ulp = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    for i, (x, g) in enumerate(zip(args.tolist(), got.tolist())):
        y = fn_mp(mpmath.mpf(x))
        d = abs(mpmath.mpf(g) - y)
        abs_err[i] = float(d)
        mag[i] = abs(float(y))
        ulp[i] = _ulp_of(y) if y != 0 else 0.0
        ulps[i] = float(d / ulp[i]) if y != 0 else (0.0 if d == 0 else math.inf)
    return ulps, abs_err, mag, ulp


def _stratified(args, scale, classes, n_each, n_rest, seed):
    """Up to n_each arguments of every reduction class in `classes` (rint(x * scale)) and n_rest of all the others, deterministically."""
    rng = np.random.default_rng(seed)
    cls = np.rint(args * scale)
    picks = []
    for sel in [cls == c for c in classes] + [~np.isin(cls, classes)]:
        idx = np.flatnonzero(sel)
        n = n_rest if len(picks) == len(classes) else n_each
        picks.append(idx if len(idx) <= n else rng.choice(idx, n, replace=False))
    return args[np.sort(np.concatenate(picks))]


def test_host_math_against_mpmath():
    """fast_exp, fast_cos and fast_sin as the host compiles them, against mpmath at 128 bits on the rate-derived arguments above
    (about 150 000), per reduction class (k of exp, the quadrant n of cos / sin): exp <= EXP_MAX_ULP ulp; cos and sin <= TRIG_MAX_ULP
    ulp where the true value is >= TRIG_REL_FLOOR, and within TRIG_MAX_ULP ulp + TRIG_MAX_ABS everywhere (the zeros included: the
    doubles nearest every multiple of pi / 2 up to 1e4 are in the set).  Prints per class the worst error in ulp, how many results
    are more than 1 ulp off, the largest absolute error near the zeros and the share of results that differ from glibc's."""
    import mpmath
    mpmath.mp.prec = 128
    lib = probe()
    quadrants = (-3, -2, -1, 0, 1)
    halfpi = multiples_of_half_pi()
    odd = np.rint(halfpi * TWO_OVER_PI) % 2 == 1
    sets = (("exp", FAST_EXP, mpmath.exp, math.exp, _stratified(exp_arguments(), LOG2E, (-2, -1, 0, 1), 6000, 16000, 3), LOG2E),
            ("cos", FAST_COS, mpmath.cos, math.cos, np.concatenate([_stratified(trig_arguments(), TWO_OVER_PI, quadrants, 4000, 12000, 4), halfpi[odd]]), TWO_OVER_PI),
            ("sin", FAST_SIN, mpmath.sin, math.sin, np.concatenate([_stratified(trig_arguments(), TWO_OVER_PI, quadrants, 2000, 6000, 5), halfpi[~odd]]), TWO_OVER_PI))
    checked = 0
    print()
    print("%-4s %-8s %7s %9s %8s %10s %14s %9s" % ("fn", "class", "args", "max ulp", "> 1 ulp", "near zero", "max |err| there", "!= glibc"))
    for name, fn, fn_mp, fn_libm, args, scale in sets:
        got = run(lib, fn, args)
        ulps, abs_err, mag, ulp = _errors(fn_mp, args, got)
        libm = np.array([fn_libm(x) for x in args.tolist()])
        cls = np.rint(args * scale)
        checked += len(args)
        rel = np.ones(len(args), bool) if name == "exp" else mag >= TRIG_REL_FLOOR
        classes = (-2, -1, 0, 1) if name == "exp" else quadrants
        label = "k" if name == "exp" else "n"
        groups = [("%s = %d" % (label, c), cls == c) for c in classes]
        groups += [("%s <= %d" % (label, classes[0] - 1), cls < classes[0]), ("%s >= %d" % (label, classes[-1] + 1), cls > classes[-1])]
        for title, sel in groups:
            r, z = sel & rel, sel & ~rel
            print("%-4s %-8s %7d %9.3f %8d %10d %14.3g %8.2f%%" % (
                name, title, int(sel.sum()), float(ulps[r].max()) if r.any() else 0.0, int((ulps[r] > 1.0).sum()), int(z.sum()),
                float(abs_err[z].max()) if z.any() else 0.0, 100.0 * float(np.mean(got[sel] != libm[sel])) if sel.any() else 0.0))
        worst = int(np.argmax(np.where(rel, ulps, 0.0)))
        assert ulps[rel].max() <= (EXP_MAX_ULP if name == "exp" else TRIG_MAX_ULP), (name, args[worst], got[worst], ulps[worst])
        if name != "exp":
            assert (~rel).sum() > 10000          # the zeros were reached
            assert np.all(abs_err <= TRIG_MAX_ULP * ulp + TRIG_MAX_ABS), (name, float(abs_err[~rel].max()))
        assert got[args == 0].tolist() == [fn_libm(0.0)] * int((args == 0).sum())
    assert checked >= 100000


def test_host_shortcuts_on_rate_arguments():
    """exp_unreduced, cos_unreduced and cos_quadrant_m1 return their full function's bits wherever their predicate holds, on the
    rate-derived argument sets (tests/native/check_math.cpp checks the same at 22.05 kHz-sized ranges); and the predicates are
    what their definitions say."""
    lib = probe()
    for args, pred_fn, scale in ((exp_arguments(), EXP_IS_UNREDUCED, LOG2E), (trig_arguments(), COS_IS_UNREDUCED, TWO_OVER_PI)):
        assert np.array_equal(run(lib, pred_fn, args), (np.rint(args * scale) == 0).astype(np.float64))
    t = trig_arguments()
    assert np.array_equal(run(lib, COS_IS_QUADRANT_M1, t), (np.rint(t * TWO_OVER_PI) == -1).astype(np.float64))
    for short, pred, full in SHORTCUTS:
        args = exp_arguments() if full == FAST_EXP else trig_arguments()
        on = run(lib, pred, args) == 1.0
        assert on.sum() > 50000
        a, b = run(lib, short, args[on]), run(lib, full, args[on])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (short, int(np.count_nonzero(a != b)))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the device's bits against the host's

@pytest.mark.gpu
@pytest.mark.parametrize("scalar_constants", [True, False])
def test_device_math_equals_host(scalar_constants):
    """Every function and predicate of klatt_math.h on the device returns the host's bits on every argument (about 9 M for exp and
    9 M for cos / sin: the sets above with every argument's two neighbours), as the engine compiles it and with the compiler's own
    fused multiply-adds; on the device each shortcut equals its full function wherever its predicate holds."""
    lib = probe(scalar_constants)
    xe = exp_arguments()
    te = trig_arguments()
    xe = np.concatenate([xe, np.nextafter(xe, np.inf), np.nextafter(xe, -np.inf)])
    te = np.concatenate([te, np.nextafter(te, np.inf), np.nextafter(te, -np.inf)])
    assert len(xe) > 8000000 and len(te) > 8000000
    dev = {}
    for name, fn in FUNCTIONS.items():
        args = xe if "exp" in name else te
        host = run(lib, fn, args)
        dev[fn] = run(lib, fn, args, device=True)
        bad = np.flatnonzero(host.view(np.uint64) != dev[fn].view(np.uint64))
        assert len(bad) == 0, "%s (scalar constants %s): %d of %d results differ from the host's; first: x=%r device %r host %r" % (
            name, scalar_constants, len(bad), len(args), args[bad[0]], dev[fn][bad[0]], host[bad[0]])
    for short, pred, full in SHORTCUTS:
        on = dev[pred] == 1.0
        assert on.sum() > 100000
        assert np.array_equal(dev[short][on].view(np.uint64), dev[full][on].view(np.uint64)), short
