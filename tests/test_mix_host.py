"""The mix export on the host (include/speechPlayer_batch.h: speechPlayer_pcmMix; nvspeechplayer_amd.pcmMix, MixTerm, check_mix_request;
csrc/klatt_mix.h): the product's CPU statement against a pure-numpy restatement of the definition -- bit for bit, both formats --, the
exact integer powers, the clip powers, the SNR a returned gain realises, and every refusal by its message.  `restate`, `gains_of`, `CASES`
and `case_terms` are the comparands tests/test_gpu_mix.py shares.  No GPU."""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.test_convolve_host import bits, to_int16, x_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
FULL_SCALE_2 = 1073676289.0      # 32767^2


def round_to_float32(fr):
    """A Fraction rounded ONCE to binary32, nearest even, gradual underflow (the values here never overflow)."""
    if fr == 0:
        return np.float32(0.0)
    sign, fr = (-1.0, -fr) if fr < 0 else (1.0, fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    elif Fraction(2) ** (e + 1) <= fr:
        e += 1
    q = max(e, -126) - 23      # the exponent of the last place
    scaled = fr / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * math.ldexp(n, q))


def fma32(v, g, acc):
    """fmaf(v, g, acc) on float32 arrays, one rounding.  The product of two float32 is exact in binary64; the binary64 sum with acc is
    rounded once more before the rounding to float32, and the two roundings differ from one only where the sum was inexact AND landed
    exactly half way between two float32 (or in the subnormal range, where the half-way pattern moves): those elements -- math.fma would
    not help, it rounds to binary64 first too -- are redone in exact rational arithmetic."""
    v, g, acc = np.asarray(v, np.float32), np.float32(g), np.asarray(acc, np.float32)
    p = v.astype(np.float64) * np.float64(g)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)      # (TwoSum: the sum's rounding error, exactly)
    r = s.astype(np.float32)
    risky = (err != 0) & (((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | (np.abs(s) < 2.0 ** -120))
    for i in np.flatnonzero(risky):
        r[i] = round_to_float32(Fraction(float(v[i])) * Fraction(float(g)) + Fraction(float(acc[i])))
    return r


def source_values(src):
    src = np.asarray(src)
    return x_of(src) if src.dtype == np.int16 else src.astype(np.float32)


def utterance_power(pcm):
    """P_u = (double)S_u / (double)L_u / 32767^2 from the exact integer sum, 0 for no samples."""
    pcm = np.asarray(pcm)
    S = int(np.sum(pcm.astype(np.int64) ** 2))
    assert S < 2 ** 53
    return float(S) / float(len(pcm)) / FULL_SCALE_2 if len(pcm) else 0.0


def clip_power(c):
    """P_c: the squares summed in ascending order in binary64, over N."""
    acc = 0.0
    for v in np.asarray(c, np.float32).tolist():
        acc += v * v
    return acc / len(c)


def power_of(src):
    return utterance_power(src) if np.asarray(src).dtype == np.int16 else clip_power(src)


def gain_of(Ps, Pv, db):
    d = Pv * 10.0 ** (db / 10.0)
    return np.float32(min(math.sqrt(Ps / d), 4294967296.0)) if Ps > 0 and d > 0 else np.float32(0.0)


def gains_of(pcm, sources, terms):
    """The float32 gains of MixTerm objects against `sources`, walked from the definition."""
    Ps = utterance_power(pcm)
    return np.array([np.float32(t.level) if t.levelKind else gain_of(Ps, power_of(sources[t.source]), t.level) for t in terms], np.float32)


def restate(pcm, sources, terms, speechGain=1.0, gains=None, dtype=np.float32):
    """The definition in numpy float32 operations: -> the mixture of `pcm` with MixTerm objects whose source indexes `sources`."""
    pcm = np.asarray(pcm)
    gains = gains_of(pcm, sources, terms) if gains is None else gains
    L, m = len(pcm), np.arange(len(pcm), dtype=np.int64)
    acc = np.float32(speechGain) * x_of(pcm)
    for t, g in zip(terms, gains):
        src = source_values(sources[t.source])
        N = len(src)
        v = np.zeros(L, np.float32)
        if t.loop:
            v = src[(t.offset + m) % N]
        else:
            i = m - t.offset
            ok = (i >= 0) & (i < N)
            v[ok] = src[i[ok]]
        acc = fma32(v, g, acc)
    y = (acc + np.float32(0.0)).astype(np.float32)
    return y if np.dtype(dtype) == np.float32 else to_int16(y)


def seeded_pcm(L, seed, scale=12000):
    return np.clip(np.random.default_rng(5000 + seed).normal(0, scale, L), -32768, 32767).astype(np.int16)


def seeded_clip(N, seed, scale=0.3):
    return (scale * np.random.default_rng(7000 + seed).standard_normal(N)).astype(np.float32)


CLIP_LENGTHS = (1, 3, 1023, 1024, 1025, 7001)      # N = 1, 3, T - 1, T, T + 1 and N > L of every test row


def bank():
    """The clips of the shared cases: the lengths above, and a silent clip."""
    return [seeded_clip(N, k) if N > 1 else np.array([0.5], np.float32) for k, N in enumerate(CLIP_LENGTHS)] + [np.zeros(300, np.float32)]


SILENT_CLIP = len(CLIP_LENGTHS)


def case_terms(L, own, other, otherLen, noise=lambda k: k):
    """The shared case list for a row of L samples, as {name: (terms, speechGain)}: `own` and `other` are the source numbers of the row's
    own utterance and of another one (of otherLen samples), noise(k) that of clip k."""
    from nvspeechplayer_amd import MixTerm as M
    cases = {}
    for k, N in enumerate(CLIP_LENGTHS):
        cases["loop_N%d_from_0" % N] = ([M(noise=noise(k), snr=10.0)], 1.0)
        cases["loop_N%d_from_last" % N] = ([M(noise=noise(k), gain=0.5, offset=N - 1)], 1.0)
    for name, off in dict(negative=-37, far_negative=-6000, zero=0, positive=5, tile=1024, last=L - 1, beyond=L, far_beyond=L + 5000).items():
        cases["once_%s" % name] = ([M(noise=noise(5), snr=5.0, offset=off, loop=False)], 1.0)
        cases["once_utterance_%s" % name] = ([M(utterance=other, gain=0.25, offset=off, loop=False)], 1.0)
    cases["no_terms"] = ([], 1.0)
    cases["no_terms_half"] = ([], 0.5)
    cases["speech_gain_0"] = ([M(noise=noise(3), snr=0.0, offset=17)], 0.0)
    cases["own_utterance"] = ([M(utterance=own, snr=0.0, offset=0, loop=False), M(utterance=own, snr=6.0, offset=L // 2)], 1.0)
    cases["other_utterance_looped"] = ([M(utterance=other, snr=3.0, offset=otherLen - 1)], -1.0)
    cases["silent_clip"] = ([M(noise=noise(SILENT_CLIP), snr=10.0), M(noise=noise(2), snr=20.0)], 1.0)
    cases["clamp"] = ([M(noise=noise(4), snr=-200.0), M(noise=noise(4), snr=200.0)], 1.0)
    cases["two_talkers_and_noise"] = ([M(noise=noise(5), snr=15.0, offset=100), M(utterance=other, snr=0.0, offset=-50, loop=False), M(noise=noise(1), gain=-0.125)], 0.75)
    return cases


def many_terms(L, own, other, otherLen, noise=lambda k: k, n=64):
    """A row with 64 terms: every clip and both utterances, looped and once, SNRs and gains."""
    from nvspeechplayer_amd import MixTerm as M
    rng = np.random.default_rng(64)
    terms = []
    for j in range(n):
        k = j % (len(CLIP_LENGTHS) + 2)
        N = CLIP_LENGTHS[k] if k < len(CLIP_LENGTHS) else (L if k == len(CLIP_LENGTHS) else otherLen)
        src = dict(noise=noise(k)) if k < len(CLIP_LENGTHS) else dict(utterance=own if k == len(CLIP_LENGTHS) else other)
        loop = j % 3 != 0
        level = dict(snr=float(rng.integers(-10, 30))) if j % 2 else dict(gain=float(rng.uniform(-0.2, 0.2)))
        terms.append(M(offset=int(rng.integers(0, N)) if loop else int(rng.integers(-2000, 2000)), loop=loop, **src, **level))
    return terms


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs, restype in (("speechPlayer_pcmMix", 11, ctypes.c_longlong), ("speechPlayer_batch_setNoiseBank", 4, ctypes.c_int),
                                 ("speechPlayer_batch_noiseBank", 4, ctypes.c_longlong), ("speechPlayer_batch_exportPower", 5, ctypes.c_longlong),
                                 ("speechPlayer_batch_exportMixed", 11, ctypes.c_longlong)):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is restype and len(fn.argtypes) == nargs, name
    section = header.split("A batch's PCM mixed with noise and other utterances")[1].split("speechPlayer_pcmMix(")[0]
    for word in ("mix_gain", "WHOLE-SIGNAL", "on the HOST", "Lemma", "MODE_FAST", "live handles", "NodePlayer", "VAD-weighted", "loudness weighting", "random",
                 "speechPlayer_mixTerm_t", "speechPlayer_mixSource_t", "kMixMaxTerms = 64", "kMixTile = 1024"):
        assert word in section, word
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_mix.h")).read()
    assert '#include "klatt_convolve.h"' in shared and "KLATT_RES_HD float mix_gain" in shared and "WHOLE-SIGNAL" in shared
    for name, pattern, value in (("kMixTile", r"constexpr int kMixTile = (\d+);", speechPlayer.MIX_TILE), ("kMixMaxTerms", r"constexpr int kMixMaxTerms = (\d+);", speechPlayer.MIX_MAX_TERMS)):
        assert int(re.search(pattern, shared).group(1)) == value, name
    for name, pattern, value in (("kMixMaxCallTerms", r"kMixMaxCallTerms = 1ll << (\d+);", speechPlayer.MIX_MAX_CALL_TERMS),
                                 ("kMixMaxClips", r"kMixMaxClips = 1ll << (\d+);", speechPlayer.MIX_MAX_CLIPS), ("kMixMaxBank", r"kMixMaxBank = 1ll << (\d+);", speechPlayer.MIX_MAX_BANK)):
        assert 1 << int(re.search(pattern, shared).group(1)) == value, name
    for method in ("setNoiseBank", "noiseBankPowers", "powerTensor", "mixedTensor"):
        assert callable(getattr(speechPlayer.BatchPlayer, method)), method
    assert nvspeechplayer_amd.pcmMix is speechPlayer.pcmMix and nvspeechplayer_amd.MixTerm is speechPlayer.MixTerm
    assert nvspeechplayer_amd.mixTermDtype is speechPlayer.mixTermDtype and speechPlayer.mixTermDtype.itemsize == 40
    assert [speechPlayer.mixTermDtype.fields[f][1] for f in ("kind", "levelKind", "source", "offset", "level", "loop", "reserved")] == [0, 4, 8, 16, 24, 32, 36]


def test_the_rounding_helpers():
    """fma32 is one rounding: against exact rational arithmetic on seeded operands, on constructed half-way cases, and where binary64 would
    round twice."""
    rng = np.random.default_rng(3)
    v = rng.standard_normal(4000).astype(np.float32)
    acc = (rng.standard_normal(4000) * 10.0 ** rng.uniform(-6, 3, 4000)).astype(np.float32)
    g = np.float32(0.37)
    got = fma32(v, g, acc)
    for i in range(0, 4000, 7):
        assert bits(got[i:i + 1])[0] == bits(np.array([round_to_float32(Fraction(float(v[i])) * Fraction(float(g)) + Fraction(float(acc[i])))]))[0], i
    # 1 + 2^-24 + 2^-60: binary64 rounds the sum to the half-way point 1 + 2^-24 and then to even, 1; one rounding gives 1 + 2^-23
    one = fma32(np.array([2.0 ** -30 + 2.0 ** -6], np.float32), np.float32(2.0 ** -30 + 2.0 ** -18), np.array([1.0], np.float32))
    exact = Fraction(2.0 ** -30 + 2.0 ** -6) * Fraction(2.0 ** -30 + 2.0 ** -18) + 1
    assert one[0] == round_to_float32(exact)
    assert round_to_float32(Fraction(1) + Fraction(1, 2 ** 24)) == np.float32(1.0) and round_to_float32(Fraction(1) + Fraction(3, 2 ** 24)) == np.float32(1.0 + 2.0 ** -22)
    assert round_to_float32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 70)) == np.float32(1.0 + 2.0 ** -23)
    assert round_to_float32(Fraction(1, 2 ** 149)) == np.float32(2.0 ** -149) and round_to_float32(Fraction(1, 2 ** 150)) == 0.0 and round_to_float32(Fraction(-3, 2 ** 150)) == np.float32(-2.0 ** -148)


ROW_LENGTHS = (3, 1023, 1024, 1025, 2049, 5000)


def test_the_statement_against_the_numpy_restatement():
    """pcmMix equals the restatement bit for bit, float32 and int16, on the whole case list for rows of every edge length, and its gains
    equal the definition's."""
    import nvspeechplayer_amd as eng
    clips = bank()
    other = seeded_pcm(2500, 99)
    for r, L in enumerate(ROW_LENGTHS):
        pcm = seeded_pcm(L, r)
        sources = clips + [pcm, other]
        own, oth = len(clips), len(clips) + 1
        cases = case_terms(L, own, oth, len(other))
        if L in (3, 1025):
            cases["many"] = (many_terms(L, own, oth, len(other)), 0.9)
        for name, (terms, sg) in cases.items():
            want_g = gains_of(pcm, sources, terms)
            got, got_g = eng.pcmMix(pcm, sources, terms, speechGain=sg, gains=True)
            assert np.array_equal(bits(got_g), bits(want_g)), (L, name, got_g, want_g)
            want = restate(pcm, sources, terms, sg, want_g)
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (L, name, np.flatnonzero(bits(got) != bits(want))[:5])
            got16 = eng.pcmMix(pcm, sources, terms, speechGain=sg, dtype=np.int16)
            assert got16.dtype == np.int16 and np.array_equal(got16, to_int16(want)), (L, name)
            if name == "clamp":
                assert got_g[0] == np.float32(2.0 ** 32) and 0 < got_g[1] < 1e-6
            if name == "silent_clip":
                assert bits(got_g[:1])[0] == 0 and got_g[1] > 0
            if name.startswith("once_") and name.endswith("beyond"):
                assert np.array_equal(bits(got), bits(x_of(pcm) + np.float32(0)))      # contributes nothing
    # silent speech: every SNR gain is +0, whatever the source; a linear gain still applies
    silent = np.zeros(700, np.int16)
    M = eng.MixTerm
    terms = [M(noise=5, snr=-20.0), M(utterance=len(clips) + 1, snr=0.0), M(noise=2, gain=0.5)]
    got, g = eng.pcmMix(silent, clips + [silent, other], terms, gains=True)
    assert not bits(g[:2]).any() and g[2] == 0.5 and np.array_equal(bits(got), bits(restate(silent, clips + [silent, other], terms)))
    # nothing to mix
    assert len(eng.pcmMix(np.zeros(0, np.int16), clips, [M(noise=0, gain=1.0)])) == 0
    # a structured array of terms is the same request
    arr = np.array([t.record() for t in terms], eng.mixTermDtype)
    assert np.array_equal(bits(eng.pcmMix(silent, clips + [silent, other], arr)), bits(got))


def test_powers_are_exact():
    """S_u is the integer sum; the clip powers are the ascending binary64 sum, bit for bit (through the gains they give: a term at 0 dB
    against a known source reveals Ps / Pv)."""
    from nvspeechplayer_amd import _native
    import nvspeechplayer_amd as eng
    L = _native.load()
    M = eng.MixTerm
    # 70000 samples of -32768: S_u = 70000 * 2^30, far beyond 32 bits.  Against a clip of constant 0.5 (P_c = 0.25) the 0 dB gain is
    # sqrt(2^30 / 32767^2 / 0.25) = 65536 / 32767 to the last bit; a sum that wrapped at 32 or 48 bits would give another gain.
    full = np.full(70000, -32768, np.int16)
    _, g = eng.pcmMix(full, [np.full(16, 0.5, np.float32), full], [M(noise=0, snr=0.0), M(utterance=1, snr=0.0)], gains=True)
    assert g[0] == np.float32(math.sqrt(float(70000 * 2 ** 30) / 70000.0 / FULL_SCALE_2 / 0.25)) == np.float32(65536.0 / 32767.0) and g[1] == 1.0
    _, g = eng.pcmMix(np.array([1, -1, 1], np.int16), [np.full(16, 0.5, np.float32), full], [M(utterance=1, snr=0.0)], gains=True)
    assert g[0] == np.float32(1.0 / 32768.0)      # ... and as the SOURCE of an SNR term: sqrt(1 / 2^30)
    for seed, N in enumerate((1, 2, 999, 4096, 50001)):
        c = seeded_clip(N, 20 + seed, scale=3.0)
        pcm = seeded_pcm(1777, seed)
        _, g = eng.pcmMix(pcm, [c, pcm], [M(noise=0, snr=0.0), M(utterance=1, snr=0.0, loop=False)], gains=True)
        assert bits(g[:1])[0] == bits(np.array([gain_of(utterance_power(pcm), clip_power(c), 0.0)]))[0], N
        assert g[1] == 1.0
    assert L.speechPlayer_lastErrorCode() == 0


def test_the_gain_realises_the_snr():
    """|10 log10(Ps / (g^2 Pv)) - level| <= 1e-6 dB for the returned float32 gain: rounding g to float32 allows
    10 log10((1 + 2^-24)^2) = 5.2e-7 dB, the three binary64 operations and the logarithm a few 1e-15."""
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    clips = bank()
    pcm, other = seeded_pcm(3000, 1), seeded_pcm(2000, 2, scale=300)
    sources = clips + [pcm, other]
    Ps = utterance_power(pcm)
    worst = 0.0
    for level in (-40.0, -12.5, -3.0, 0.0, 0.1, 5.0, 10.0, 20.0, 33.3, 60.0):
        terms = [M(noise=k, snr=level) for k in range(len(CLIP_LENGTHS))] + [M(utterance=len(clips) + 1, snr=level), M(utterance=len(clips), snr=level)]
        _, g = eng.pcmMix(pcm, sources, terms, gains=True)
        for t, gj in zip(terms, g):
            realised = 10.0 * math.log10(Ps / (float(gj) ** 2 * power_of(sources[t.source])))
            worst = max(worst, abs(realised - level))
            assert abs(realised - level) <= 1e-6, (level, t, realised)
    print("largest SNR error: %.3g dB" % worst)


def mix_call(L, pcm, length, sources, terms, speechGain=1.0, gains=None, fmt=1, out=None, capacity=None, nSources=None, nTerms=None):
    from nvspeechplayer_amd import speechPlayer as sp
    p = lambda a: None if a is None else a.ctypes.data
    table = np.zeros(max(len(sources), 1), sp._mixSourceDtype)
    for k, (a, n, f) in enumerate(sources):
        table[k] = (0 if a is None else a.ctypes.data, n, f, 0)
    keep = (table, terms)
    got = L.speechPlayer_pcmMix(p(pcm), length, speechGain, table.ctypes.data if len(sources) else None, len(sources) if nSources is None else nSources,
                                p(terms) if terms is not None and len(terms) else None, (0 if terms is None else len(terms)) if nTerms is None else nTerms, p(gains), fmt,
                                p(out), (0 if out is None else len(out)) if capacity is None else capacity)
    del keep
    return got


def test_every_refusal_of_the_c_entry_point():
    from nvspeechplayer_amd import _native
    import nvspeechplayer_amd as eng
    L = _native.load()
    pcm = np.arange(200, dtype=np.int16)
    out = np.full(300, -7.0, np.float32)
    gains = np.full(8, -7.0, np.float32)
    clip, quiet, bad = np.full(50, 0.25, np.float32), np.zeros(0, np.int16), np.full(50, 0.25, np.float32)
    good_sources = [(clip, 50, 1), (pcm, 200, 0), (quiet, 0, 0)]

    def term(kind=0, levelKind=0, source=0, offset=0, level=10.0, loop=1):
        return np.array([(kind, levelKind, source, offset, level, loop, 0)], eng.mixTermDtype)

    def call(terms="one", sources=good_sources, **kw):
        a = dict(pcm=pcm, length=200, sources=sources, terms=term() if isinstance(terms, str) else terms, out=out, gains=gains)
        a.update(kw)
        return mix_call(L, a.pop("pcm"), a.pop("length"), a.pop("sources"), a.pop("terms"), **a)

    def with_value(v):
        c = bad.copy()
        c[7] = v
        return [(c, 50, 1)] + good_sources[1:]

    refused = dict(
        length_negative=(dict(length=-1), "length -1"), no_pcm=(dict(pcm=None), "length 200"), format_2=(dict(fmt=2), "format 2"), format_negative=(dict(fmt=-1), "format -1"),
        sources_negative=(dict(nSources=-1), "-1 sources"), terms_negative=(dict(nTerms=-1), "-1 terms"), terms_65=(dict(terms=np.repeat(term(), 65)), "65 terms"),
        no_terms_array=(dict(terms=None, nTerms=1), "1 terms"), capacity_short=(dict(capacity=199), "capacity is 199"),
        speech_gain_nan=(dict(speechGain=float("nan")), "speechGain nan"), speech_gain_inf=(dict(speechGain=float("inf")), "speechGain inf"),
        speech_gain_above=(dict(speechGain=2.0 ** 33), "speechGain"),
        source_format=(dict(sources=[(clip, 50, 2)]), "source 0 has format 2"), clip_empty=(dict(sources=[(clip, 0, 1)]), "source 0 has 0 samples"),
        source_negative=(dict(sources=[(clip, -1, 0)]), "source 0 has -1 samples"), source_null=(dict(sources=[(None, 5, 0)]), "source 0 has 5 samples"),
        clip_nan=(dict(sources=with_value(np.nan)), "sample 7 of clip 0 is nan"), clip_inf=(dict(sources=with_value(np.inf)), "sample 7 of clip 0 is inf"),
        clip_minus_inf=(dict(sources=with_value(-np.inf)), "sample 7 of clip 0 is -inf"), clip_above=(dict(sources=with_value(np.float32(65536.0 * (1 + 2.0 ** -23)))), "sample 7 of clip 0"),
        clip_below=(dict(sources=with_value(-131072.0)), "sample 7 of clip 0"),
        kind_2=(dict(terms=term(kind=2)), "row 0, term 0: kind 2"), kind_negative=(dict(terms=term(kind=-1)), "row 0, term 0: kind -1"),
        level_kind_2=(dict(terms=term(levelKind=2)), "levelKind 2"), loop_2=(dict(terms=term(loop=2)), "loop 2"), loop_negative=(dict(terms=term(loop=-1)), "loop -1"),
        source_beyond=(dict(terms=term(source=3)), "clip 3 is not in the bank"), source_below=(dict(terms=term(source=-1)), "clip -1 is not in the bank"),
        utterance_beyond=(dict(terms=term(kind=1, source=3)), "source 3 is not an utterance"),
        kind_names_utterance=(dict(terms=term(kind=0, source=1)), "kind 0 names source 1"), kind_names_clip=(dict(terms=term(kind=1, source=0)), "kind 1 names source 0"),
        looped_empty=(dict(terms=term(kind=1, source=2)), "a looped source of length 0"),
        loop_offset_N=(dict(terms=term(offset=50)), "offset 50 of a looped source of 50 samples"), loop_offset_negative=(dict(terms=term(offset=-1)), "offset -1 of a looped source"),
        offset_above=(dict(terms=term(loop=0, offset=2 ** 44 + 1)), "offset 17592186044417"), offset_below=(dict(terms=term(loop=0, offset=-2 ** 44 - 1)), "offset -17592186044417"),
        snr_nan=(dict(terms=term(level=np.nan)), "an SNR of nan dB"), snr_inf=(dict(terms=term(level=np.inf)), "an SNR of inf dB"), snr_above=(dict(terms=term(level=200.5)), "an SNR of 200.5 dB"),
        snr_below=(dict(terms=term(level=-1000.0)), "an SNR of -1000 dB"),
        gain_nan=(dict(terms=term(levelKind=1, level=np.nan)), "gain nan"), gain_inf=(dict(terms=term(levelKind=1, level=-np.inf)), "gain -inf"),
        gain_above=(dict(terms=term(levelKind=1, level=2.0 ** 32 + 1)), "gain 4.29497e+09"))
    for name, (kw, message) in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        text = L.speechPlayer_lastError().decode()
        assert text.startswith("pcmMix: ") and message in text, (name, text)
        assert np.all(out == -7.0) and np.all(gains == -7.0), name
    second = np.concatenate([term(), term(kind=1, source=1, level=np.nan)])
    assert call(terms=second) == -1 and b"row 0, term 1: an SNR of nan dB" in L.speechPlayer_lastError()
    # sizing, nothing to compute, the limits themselves, and the entry point is as usable as before
    assert call(out=None, capacity=0) == 200 and L.speechPlayer_lastErrorCode() == 0 and gains[0] != -7.0 and np.all(gains[1:] == -7.0)
    assert call(pcm=None, length=0, out=None, gains=None) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert call(terms=term(loop=0, offset=2 ** 44), gains=None) == 200 and call(terms=term(loop=0, offset=-2 ** 44), gains=None) == 200
    assert call(terms=term(level=200.0), gains=None) == 200 and call(terms=term(level=-200.0), gains=None) == 200
    assert call(terms=term(levelKind=1, level=-2.0 ** 32), gains=None, speechGain=2.0 ** 32) == 200
    assert call(terms=term(kind=1, source=2, loop=0), gains=None) == 200      # a source of no samples, placed once: nothing
    assert call(sources=with_value(-65536.0), gains=None) == 200
    assert call(terms=np.repeat(term(), 64), gains=None) == 200
    assert call(capacity=200) == 200 and np.all(out[:200] != -7.0) and np.all(out[200:] == -7.0)


def test_a_null_batch_is_an_argument_error():
    from nvspeechplayer_amd import _native
    L = _native.load()
    start = np.zeros(1, np.int64)
    for name, call in (("setNoiseBank", lambda: L.speechPlayer_batch_setNoiseBank(None, None, None, 0)), ("noiseBank", lambda: L.speechPlayer_batch_noiseBank(None, None, None, 0)),
                       ("exportPower", lambda: L.speechPlayer_batch_exportPower(None, None, 0, None, None)),
                       ("exportMixed", lambda: L.speechPlayer_batch_exportMixed(None, None, 0, None, start.ctypes.data, None, None, None, 1, 0, None))):
        assert call() == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and L.speechPlayer_lastError().decode() == "%s: no batch" % name, name


def test_mix_request_checks():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    M, check = sp.MixTerm, sp.check_mix_request
    t = M(noise=2, snr=10.0)
    assert t.record() == (0, 0, 2, 0, 10.0, 1, 0) and M(utterance=3, gain=0.5, offset=-4, loop=False).record() == (1, 1, 3, -4, 0.5, 0, 0)
    flat, start, sg, fmt = check([[t], [], [t, M(utterance=0, gain=1)]], 3, None, None)
    assert flat.dtype == sp.mixTermDtype and len(flat) == 3 and list(start) == [0, 1, 1, 3] and start.dtype == np.int64 and sg is None and fmt == 1
    flat2, start2, sg, fmt = check((flat, [0, 1, 1, 3]), 3, 0.5, torch.int16)
    assert flat2.tobytes() == flat.tobytes() and list(start2) == [0, 1, 1, 3] and sg.dtype == np.float32 and list(sg) == [0.5] * 3 and fmt == 0
    assert list(check([[], []], 2, [1, 2], np.int16)[2]) == [1.0, 2.0]
    assert check([[t] * 64], 1, None, np.float32)[3] == 1
    for name, kw in dict(neither=dict(snr=1.0), both=dict(noise=1, utterance=2, snr=1.0), no_level=dict(noise=1), both_levels=dict(noise=1, snr=1.0, gain=1.0),
                         loop=dict(noise=1, snr=1.0, loop=2)).items():
        with pytest.raises(ValueError):
            M(**kw)
            pytest.fail(name)
    for name, kw in dict(real=dict(noise=1.0, snr=1.0), flag=dict(utterance=True, snr=1.0), offset=dict(noise=1, snr=1.0, offset=0.5)).items():
        with pytest.raises(TypeError):
            M(**kw)
            pytest.fail(name)
    value = dict(rows=([[t]], 2, None), terms_65=([[t] * 65], 1, None), start_short=((flat, [0, 3]), 3, None), start_late=((flat, [1, 1, 1, 3]), 3, None),
                 start_back=((flat, [0, 2, 1, 3]), 3, None), start_end=((flat, [0, 1, 1, 2]), 3, None), gains_short=([[t], []], 2, [1.0]))
    for name, (terms, n, sg) in value.items():
        with pytest.raises(ValueError):
            check(terms, n, sg, None)
            pytest.fail(name)
    kinds = dict(not_a_list=(t, 1, None, None), not_terms=([[1, 2]], 1, None, None), wrong_dtype=((np.zeros(3, np.int64), [0, 3]), 1, None, None),
                 start_real=((flat, [0.0, 1.0, 1.0, 3.0]), 3, None, None), gain_text=([[t]], 1, "loud", None), gain_2d=([[t]], 1, [[1.0]], None),
                 float64=([[t]], 1, None, torch.float64), int32=([[t]], 1, None, np.int32), name=([[t]], 1, None, "pcm"))
    for name, (terms, n, sg, dtype) in kinds.items():
        with pytest.raises(TypeError):
            check(terms, n, sg, dtype)
            pytest.fail(name)
    import nvspeechplayer_amd as eng
    for pcm in (np.zeros(10, np.float32), np.zeros((2, 10), np.int16), [1, 2, 3]):
        with pytest.raises(TypeError):
            eng.pcmMix(pcm, [], [])
    with pytest.raises(TypeError):
        eng.pcmMix(np.zeros(10, np.int16), [np.zeros(4, np.int32)], [])
    with pytest.raises(RuntimeError, match="sample 1 of clip 0"):
        eng.pcmMix(np.zeros(10, np.int16), [np.array([0.0, np.nan])], [t.__class__(noise=0, gain=1.0)])


def test_the_statement_under_sanitizers(tmp_path):
    """csrc/klatt_mix.h (the bank, the refusals, the statement, the kernel's tile / wrap / skip arithmetic) in a program of its own,
    tests/native/check_mix.cpp, against brute force under AddressSanitizer + UBSan.  Nothing loaded into python is run under one."""
    exe = str(tmp_path / "check_mix")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_mix.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out
