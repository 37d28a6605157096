"""The mix onto a signal and the power of a signal's row on the host (include/speechPlayer_batch.h: speechPlayer_signalMix,
speechPlayer_signalPower; nvspeechplayer_amd.signalMix, signalPower, check_mix_request's signal case; csrc/klatt_sigpower.h): the fixed
tree against a numpy restatement of the definition -- bit for bit --, its derived error bound against math.fsum, the int16 case against the
exact integer sum, the statement of the mix against the restatement tests/test_mix_host.py uses for the fmaf chain, signalMix == pcmMix on
int16 inputs, the SNR a gain realises, and every refusal by its message.  `power_restated`, `signal_gains` and `restate_signal` are the
comparands tests/test_gpu_signal_mix.py shares.  No GPU."""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.test_convolve_host import bits, to_int16, x_of
from tests.test_mix_host import CLIP_LENGTHS, FULL_SCALE_2, bank, clip_power, fma32, gain_of, seeded_clip, seeded_pcm, source_values, utterance_power

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
BLOCK, LEAF = 2048, 8


def bits64(v):
    """The bits of one binary64 value."""
    return int(np.array([v], np.float64).view(np.uint64)[0])


def power_restated(x):
    """The definition of a float32 row's power in explicit binary64 additions: the squares padded with +0 to whole blocks, the eight
    columns of the leaves added in ascending order, eight explicit pairwise halvings, a Python loop over the blocks from +0.0, over L."""
    x = np.asarray(x, np.float32)
    L = len(x)
    Q = 0.0
    for b in range(-(-L // BLOCK)):
        sq = np.zeros(BLOCK, np.float64)
        part = x[b * BLOCK:(b + 1) * BLOCK].astype(np.float64)
        sq[:len(part)] = part * part
        sq = sq.reshape(BLOCK // LEAF, LEAF)
        t = sq[:, 0] + sq[:, 1]
        for q in range(2, LEAF):
            t = t + sq[:, q]
        for _ in range(8):
            t = t[0::2] + t[1::2]
        assert t.shape == (1,)
        Q = Q + float(t[0])
    return Q / float(L) if L else 0.0


def row_power(x):
    """A row's power by its dtype: the tree (float32) or the exact integer sum (int16)."""
    x = np.asarray(x)
    return utterance_power(x) if x.dtype == np.int16 else power_restated(x)


def signal_gains(x, sources, terms):
    """The float32 gains of MixTerm objects on a signal's row: utterance= names a row (its power by its dtype), noise= a clip."""
    Ps = row_power(x)
    return np.array([np.float32(t.level) if t.levelKind else gain_of(Ps, row_power(sources[t.source]) if t.kind else clip_power(sources[t.source]), t.level)
                     for t in terms], np.float32)


def restate_signal(x, sources, terms, speechGain=1.0, gains=None, dtype=np.float32):
    """tests/test_mix_host.py's restatement with the row's samples in place of the PCM: float32 as they are, int16 over 32767."""
    x = np.asarray(x)
    gains = signal_gains(x, sources, terms) if gains is None else gains
    L, m = len(x), np.arange(len(x), dtype=np.int64)
    acc = np.float32(speechGain) * source_values(x)
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


def seeded_row(L, seed, scale=0.2):
    """A float32 row no int16 PCM gives: noise whose level drifts over four decades, a -0.0 and the bound itself where there is room."""
    rng = np.random.default_rng(9000 + seed)
    x = (scale * rng.standard_normal(L) * 10.0 ** rng.uniform(-2, 2, L)).astype(np.float32)
    np.clip(x, -65536.0, 65536.0, out=x)
    if L > 4:
        x[1], x[3] = -0.0, 65536.0 if seed % 2 else 0.75
    return x


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs, restype in (("speechPlayer_batch_exportPowerOf", 6, ctypes.c_longlong), ("speechPlayer_batch_exportMixedOf", 12, ctypes.c_longlong),
                                 ("speechPlayer_signalPower", 4, ctypes.c_int), ("speechPlayer_signalMix", 12, ctypes.c_longlong)):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is restype and len(fn.argtypes) == nargs, name
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_sigpower.h")).read()
    mix = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_mix.h")).read()
    assert '#include "klatt_sigpower.h"' in mix
    for word in ("Lemma", "EXACT in binary64", "FMA", "WHOLE-SIGNAL", "klatt_signal_power", "atomics", "2^16"):
        assert word in shared, word
    assert int(re.search(r"constexpr int kSigPowerBlock = (\d+);", shared).group(1)) == speechPlayer.SIGNAL_POWER_BLOCK == BLOCK
    assert int(re.search(r"constexpr int kSigPowerLeaf = (\d+);", shared).group(1)) == LEAF
    assert 1 << int(re.search(r"kSigPowerMaxBlocks = 1ll << (\d+);", shared).group(1)) == speechPlayer.SIGNAL_POWER_MAX_BLOCKS
    # the two sentences that kept the mix at the head of the chain are gone, and what remains out is said
    for text in (header, mix, open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "until host and device share a fixed reduction shape" not in text and "a signal as the speech row of exportMixed" not in text
        assert "use speechGain = 0 for the noise bed" not in text
    for word in ("a term from a different signal", "live handles", "NodePlayer", "loudness weighting"):
        assert word in header.split("A batch's PCM mixed with noise and other utterances")[1].split("speechPlayer_pcmMix(")[0], word
    assert nvspeechplayer_amd.signalMix is speechPlayer.signalMix and nvspeechplayer_amd.signalPower is speechPlayer.signalPower
    import inspect
    assert "signal" in inspect.signature(speechPlayer.BatchPlayer.mixedTensor).parameters and "signal" in inspect.signature(speechPlayer.BatchPlayer.powerTensor).parameters
    assert "signalRows" in inspect.signature(speechPlayer.check_mix_request).parameters


POWER_LENGTHS = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4097, 3 * 2048 + 5)


def test_signal_power_of_float32_is_the_tree_bit_for_bit():
    import nvspeechplayer_amd as eng
    for seed, L in enumerate(POWER_LENGTHS):
        for scale in (0.2, 300.0):
            x = seeded_row(L, seed, scale)
            got = eng.signalPower(x)
            assert bits64(got) == bits64(power_restated(x)), (L, scale, got, power_restated(x))
            assert got >= 0.0 and (L > 0 or bits64(got) == 0)
    assert eng.signalPower(np.full(5000, 1.0, np.float32)) == 1.0 and eng.signalPower(np.full(4096, -65536.0, np.float32)) == 2.0 ** 32
    assert bits64(eng.signalPower(np.full(3000, -0.0, np.float32))) == 0
    # the shape matters: one ascending chain over the same squares rounds differently
    x = seeded_row(3 * 2048 + 5, 77)
    sq = np.zeros(4 * BLOCK)
    sq[:len(x)] = x.astype(np.float64) ** 2
    plain = 0.0
    for v in sq.tolist():
        plain += v
    assert plain / len(x) != eng.signalPower(x), "a plain ascending chain happened to give the tree's bits: choose another seed"


def test_signal_power_is_within_its_derived_bound():
    """|P - exact| <= (16 + nBlocks) * 2^-53 * P: a square is exact; a leaf makes 7 additions, the tree 8 levels, the row nBlocks - 1
    more (the first adds to +0 exactly), and the division one rounding: 7 + 8 + nBlocks - 1 + 1 = 15 + nBlocks relative errors of at most
    2^-53 each on non-negative terms, so the relative error is below (15 + nBlocks) * 2^-53 * (1 + tiny) <= (16 + nBlocks) * 2^-53."""
    import nvspeechplayer_amd as eng
    for seed, L in enumerate(POWER_LENGTHS[1:] + (20000,)):
        x = seeded_row(L, 40 + seed, 5.0)
        want = math.fsum(v * v for v in x.tolist()) / L      # (a float32's square is exact in binary64; fsum rounds their sum once)
        got = eng.signalPower(x)
        nBlocks = -(-L // BLOCK)
        err = abs(Fraction(got) - Fraction(want))
        print("L %d: error %.3g of the bound" % (L, float(err / (Fraction(16 + nBlocks, 2 ** 53) * Fraction(want)))))
        assert err <= Fraction(16 + nBlocks, 2 ** 53) * Fraction(want), (L, float(err), got, want)


def test_signal_power_of_int16_is_the_pools():
    import nvspeechplayer_amd as eng
    for seed, L in enumerate((0, 1, 3, 2048, 5000)):
        pcm = seeded_pcm(L, seed)
        S = int(np.sum(pcm.astype(np.int64) ** 2))
        want = float(S) / float(L) / FULL_SCALE_2 if L else 0.0
        assert bits64(eng.signalPower(pcm)) == bits64(want) == bits64(utterance_power(pcm)), L
    assert eng.signalPower(np.full(70000, -32768, np.int16)) == float(70000 * 2 ** 30) / 70000.0 / FULL_SCALE_2      # beyond 32 bits


ROW_LENGTHS = (0, 3, 1023, 1025, 2049, 5000)


def signal_cases(L, own, other, otherLen, silent):
    """Looped and placed terms, SNR and gain levels, clips and rows of either dtype as sources: {name: (terms, speechGain)}."""
    from nvspeechplayer_amd import MixTerm as M
    cases = {}
    for k, N in enumerate(CLIP_LENGTHS):
        cases["loop_N%d" % N] = ([M(noise=k, snr=10.0, offset=N - 1)], 1.0)
    for name, off in dict(negative=-37, zero=0, positive=5, tile=1024, last=L - 1, beyond=L + 5000).items():
        cases["once_clip_%s" % name] = ([M(noise=5, snr=5.0, offset=off, loop=False)], 1.0)
        cases["once_row_%s" % name] = ([M(utterance=other, snr=-3.0, offset=off, loop=False)], 0.5)
    cases["no_terms"] = ([], 0.5)
    cases["own_row"] = ([M(utterance=own, snr=0.0, offset=0, loop=False)] + ([M(utterance=own, snr=6.0, offset=L // 2)] if L else []), 1.0)
    cases["other_row_looped"] = ([M(utterance=other, snr=3.0, offset=otherLen - 1), M(utterance=other + 1, gain=0.25, offset=7)], -1.0)
    cases["silent_source"] = ([M(utterance=silent, snr=10.0, loop=False), M(noise=len(CLIP_LENGTHS), snr=10.0), M(noise=2, snr=20.0)], 1.0)
    cases["clamp"] = ([M(noise=4, snr=-200.0), M(utterance=other, snr=200.0)], 1.0)
    cases["gains"] = ([M(noise=5, gain=0.5, offset=100), M(utterance=other, gain=-0.125, offset=-50, loop=False)], 0.75)
    return cases


def test_signal_mix_of_float32_rows_against_the_numpy_restatement():
    """Bit for bit, float32 and int16 outputs, gains included; a silent row or a silent source gives gain +0."""
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    clips = bank()
    other, other16, silent = seeded_row(2500, 99), seeded_pcm(1700, 98), np.zeros(300, np.float32)
    for r, L in enumerate(ROW_LENGTHS):
        x = seeded_row(L, r)
        sources = clips + [x, other, other16, silent]
        own, oth, sil = len(clips), len(clips) + 1, len(clips) + 3
        for name, (terms, sg) in signal_cases(L, own, oth, len(other), sil).items():
            want_g = signal_gains(x, sources, terms)
            got, got_g = eng.signalMix(x, sources, terms, speechGain=sg, gains=True)
            assert np.array_equal(bits(got_g), bits(want_g)), (L, name, got_g, want_g)
            want = restate_signal(x, sources, terms, sg, want_g)
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (L, name, np.flatnonzero(bits(got) != bits(want))[:5])
            got16 = eng.signalMix(x, sources, terms, speechGain=sg, dtype=np.int16)
            assert got16.dtype == np.int16 and np.array_equal(got16, to_int16(want)), (L, name)
            if name == "silent_source" and L:
                assert not bits(got_g[:2]).any() and got_g[2] > 0
            if name == "clamp" and L >= 1000:
                assert got_g[0] == np.float32(2.0 ** 32) and 0 < got_g[1] < 1e-6
            if L == 0:
                assert not bits(got_g[[t.levelKind == 0 for t in terms]]).any()      # a row of nothing is silent
    # a silent row: every SNR gain is +0, whatever the source; a linear gain still applies
    quiet = np.zeros(700, np.float32)
    terms = [M(noise=5, snr=-20.0), M(utterance=len(clips) + 1, snr=0.0), M(noise=2, gain=0.5)]
    got, g = eng.signalMix(quiet, clips + [quiet, other], terms, gains=True)
    assert not bits(g[:2]).any() and g[2] == 0.5 and np.array_equal(bits(got), bits(restate_signal(quiet, clips + [quiet, other], terms)))
    # one float32 source named as a clip and as a row in one call: the ascending clip power for the one, the tree for the other
    both = seeded_clip(5000, 3, scale=2.0)
    terms = [M(noise=0, snr=0.0), M(utterance=0, snr=0.0), M(noise=0, snr=6.0)]
    _, g = eng.signalMix(other, [both], terms, gains=True)
    assert clip_power(both) != power_restated(both) and np.array_equal(bits(g), bits(signal_gains(other, [both], terms)))
    # an int16 row mixed with float32 rows, and the other way round
    pcm = seeded_pcm(1500, 5)
    terms = [M(utterance=1, snr=4.0, offset=11), M(utterance=0, snr=0.0, loop=False)]
    for x in (pcm, other):
        got, g = eng.signalMix(x, [pcm, other], terms, gains=True)
        assert np.array_equal(bits(g), bits(signal_gains(x, [pcm, other], terms))) and np.array_equal(bits(got), bits(restate_signal(x, [pcm, other], terms)))


def test_signal_mix_of_int16_inputs_is_pcm_mix():
    import nvspeechplayer_amd as eng
    from tests.test_mix_host import case_terms, many_terms
    clips = bank()
    other = seeded_pcm(2500, 99)
    for r, L in enumerate((3, 1025, 5000)):
        pcm = seeded_pcm(L, r)
        sources = clips + [pcm, other]
        cases = case_terms(L, len(clips), len(clips) + 1, len(other))
        cases["many"] = (many_terms(L, len(clips), len(clips) + 1, len(other)), 0.9)
        for name, (terms, sg) in cases.items():
            for dtype in (np.float32, np.int16):
                a, ga = eng.pcmMix(pcm, sources, terms, speechGain=sg, dtype=dtype, gains=True)
                b, gb = eng.signalMix(pcm, sources, terms, speechGain=sg, dtype=dtype, gains=True)
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes() and ga.tobytes() == gb.tobytes(), (L, name, dtype)


def test_the_gain_realises_the_snr():
    """The tolerance of tests/test_mix_host.py::test_the_gain_realises_the_snr: |10 log10(Ps / (g^2 Pv)) - level| <= 1e-6 dB."""
    import nvspeechplayer_amd as eng
    M = eng.MixTerm
    clips = bank()
    x, other, other16 = seeded_row(3000, 1), seeded_row(2000, 2, scale=0.003), seeded_pcm(900, 3)
    sources = clips + [x, other, other16]
    Ps = eng.signalPower(x)
    for level in (-40.0, -12.5, -3.0, 0.0, 0.1, 5.0, 10.0, 20.0, 33.3, 60.0):
        terms = [M(noise=k, snr=level) for k in range(len(CLIP_LENGTHS))] + [M(utterance=len(clips) + k, snr=level) for k in range(3)]
        _, g = eng.signalMix(x, sources, terms, gains=True)
        for t, gj in zip(terms, g):
            Pv = eng.signalPower(sources[t.source]) if t.kind else clip_power(sources[t.source])
            realised = 10.0 * math.log10(Ps / (float(gj) ** 2 * Pv))
            assert abs(realised - level) <= 1e-6, (level, t, realised)


def mix_call(L, x, inFormat, length, sources, terms, speechGain=1.0, gains=None, fmt=1, out=None, capacity=None, nSources=None, nTerms=None):
    from nvspeechplayer_amd import speechPlayer as sp
    p = lambda a: None if a is None else a.ctypes.data
    table = np.zeros(max(len(sources), 1), sp._mixSourceDtype)
    for k, (a, n, f) in enumerate(sources):
        table[k] = (0 if a is None else a.ctypes.data, n, f, 0)
    keep = (table, terms)
    got = L.speechPlayer_signalMix(p(x), inFormat, length, speechGain, table.ctypes.data if len(sources) else None, len(sources) if nSources is None else nSources,
                                   p(terms) if terms is not None and len(terms) else None, (0 if terms is None else len(terms)) if nTerms is None else nTerms, p(gains), fmt,
                                   p(out), (0 if out is None else len(out)) if capacity is None else capacity)
    del keep
    return got


def test_every_refusal_of_the_c_entry_points():
    from nvspeechplayer_amd import _native
    import nvspeechplayer_amd as eng
    L = _native.load()
    x = np.linspace(-1, 1, 200).astype(np.float32)
    out = np.full(300, -7.0, np.float32)
    gains = np.full(8, -7.0, np.float32)
    clip, row16, quiet, empty = np.full(50, 0.25, np.float32), np.arange(200, dtype=np.int16), np.zeros(0, np.int16), np.zeros(0, np.float32)
    good_sources = [(clip, 50, 1), (row16, 200, 0), (quiet, 0, 0), (empty, 0, 1)]

    def term(kind=0, levelKind=0, source=0, offset=0, level=10.0, loop=1):
        return np.array([(kind, levelKind, source, offset, level, loop, 0)], eng.mixTermDtype)

    def call(terms="one", sources=good_sources, **kw):
        a = dict(x=x, inFormat=1, length=200, sources=sources, terms=term() if isinstance(terms, str) else terms, out=out, gains=gains)
        a.update(kw)
        return mix_call(L, a.pop("x"), a.pop("inFormat"), a.pop("length"), a.pop("sources"), a.pop("terms"), **a)

    def with_value(v, at=7):
        c = x.copy()
        c[at] = v
        return c

    def clip_with(v):
        c = clip.copy()
        c[7] = v
        return [(c, 50, 1)] + good_sources[1:]

    refused = dict(
        in_format_2=(dict(inFormat=2), "input format 2"), in_format_negative=(dict(inFormat=-1), "input format -1"),
        length_negative=(dict(length=-1), "length -1"), no_samples=(dict(x=None), "length 200"), format_2=(dict(fmt=2), "format 2"),
        sources_negative=(dict(nSources=-1), "-1 sources"), terms_negative=(dict(nTerms=-1), "-1 terms"), terms_65=(dict(terms=np.repeat(term(), 65)), "65 terms"),
        no_terms_array=(dict(terms=None, nTerms=1), "1 terms"), capacity_short=(dict(capacity=199), "capacity is 199"),
        speech_gain_nan=(dict(speechGain=float("nan")), "speechGain nan"), speech_gain_above=(dict(speechGain=2.0 ** 33), "speechGain"),
        source_format=(dict(sources=[(clip, 50, 2)]), "source 0 has format 2"), source_negative=(dict(sources=[(clip, -1, 1)]), "source 0 has -1 samples"),
        source_null=(dict(sources=[(None, 5, 1)]), "source 0 has 5 samples"),
        clip_nan=(dict(sources=clip_with(np.nan)), "sample 7 of clip 0 is nan"), clip_above=(dict(sources=clip_with(-131072.0)), "sample 7 of clip 0"),
        value_nan=(dict(x=with_value(np.nan)), "sample 7 is nan"), value_inf=(dict(x=with_value(-np.inf, 0)), "sample 0 is -inf"),
        value_above=(dict(x=with_value(np.float32(65536.0 * (1 + 2.0 ** -23)), 199)), "sample 199 is"), value_gain_only=(dict(x=with_value(1e30), terms=term(levelKind=1, level=1.0)), "sample 7 is 1e+30"),
        kind_2=(dict(terms=term(kind=2)), "row 0, term 0: kind 2"), level_kind_2=(dict(terms=term(levelKind=2)), "levelKind 2"), loop_2=(dict(terms=term(loop=2)), "loop 2"),
        clip_beyond=(dict(terms=term(source=4)), "clip 4 is not in the bank"), row_beyond=(dict(terms=term(kind=1, source=4)), "row 0, term 0: source 4 is not a row of the signal"),
        row_negative=(dict(terms=term(kind=1, source=-1)), "source -1 is not a row of the signal"),
        clip_names_int16=(dict(terms=term(kind=0, source=1)), "kind 0 names source 1"), clip_empty=(dict(terms=term(kind=0, source=3, loop=0)), "row 0, term 0: clip 3 has 0 samples"),
        looped_empty=(dict(terms=term(kind=1, source=3)), "a looped source of length 0"), looped_empty_int16=(dict(terms=term(kind=1, source=2)), "a looped source of length 0"),
        loop_offset_N=(dict(terms=term(offset=50)), "offset 50 of a looped source of 50 samples"), offset_above=(dict(terms=term(loop=0, offset=2 ** 44 + 1)), "offset 17592186044417"),
        snr_nan=(dict(terms=term(level=np.nan)), "an SNR of nan dB"), snr_above=(dict(terms=term(level=200.5)), "an SNR of 200.5 dB"),
        gain_inf=(dict(terms=term(levelKind=1, level=-np.inf)), "gain -inf"), gain_above=(dict(terms=term(levelKind=1, level=2.0 ** 32 + 1)), "gain 4.29497e+09"))
    for name, (kw, message) in refused.items():
        assert call(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        text = L.speechPlayer_lastError().decode()
        assert text.startswith("signalMix: ") and message in text, (name, text)
        assert np.all(out == -7.0) and np.all(gains == -7.0), name
    second = np.concatenate([term(), term(kind=1, source=1, level=np.nan)])
    assert call(terms=second) == -1 and b"row 0, term 1: an SNR of nan dB" in L.speechPlayer_lastError()
    # what is admitted: a float32 row as a kind-1 source, an empty one placed once, sizing, the bound itself
    assert call(terms=term(kind=1, source=0), gains=None) == 200 and call(terms=term(kind=1, source=3, loop=0), gains=None) == 200
    assert call(out=None, capacity=0) == 200 and L.speechPlayer_lastErrorCode() == 0 and gains[0] != -7.0 and np.all(gains[1:] == -7.0)
    assert call(x=None, length=0, out=None, gains=None) == 0 and call(x=with_value(-65536.0), gains=None) == 200
    assert call(x=row16, inFormat=0, gains=None) == 200 and L.speechPlayer_lastErrorCode() == 0
    # ---- signalPower ----
    power = np.full(1, -7.0)
    p = lambda a: None if a is None else a.ctypes.data
    with_nan, above = with_value(np.nan), with_value(1e5)
    for name, (args, message) in dict(in_format=((p(x), 2, 200, p(power)), "input format 2"), length=((p(x), 1, -1, p(power)), "length -1"), no_samples=((None, 1, 5, p(power)), "length 5"),
                                      too_long=((p(x), 0, 2 ** 33 + 1, p(power)), "length 8589934593"), no_output=((p(x), 1, 200, None), "no output"),
                                      nan=((p(with_nan), 1, 200, p(power)), "sample 7 is nan"), above=((p(above), 1, 200, p(power)), "sample 7 is 100000")).items():
        assert L.speechPlayer_signalPower(*args) == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT, name
        text = L.speechPlayer_lastError().decode()
        assert text.startswith("signalPower: ") and message in text and power[0] == -7.0, (name, text)
    assert L.speechPlayer_signalPower(None, 1, 0, p(power)) == 0 and power[0] == 0.0 and L.speechPlayer_lastErrorCode() == 0
    for bad in (np.zeros(4, np.float64), np.zeros((2, 2), np.float32), [1.0]):
        with pytest.raises(TypeError):
            eng.signalPower(bad)
        with pytest.raises(TypeError):
            eng.signalMix(bad, [], [])
    with pytest.raises(RuntimeError, match="sample 1 is inf"):
        eng.signalPower(np.array([0.0, np.inf], np.float32))


def test_mix_request_checks_of_a_signal():
    from nvspeechplayer_amd import speechPlayer as sp
    M, check = sp.MixTerm, sp.check_mix_request
    rows = [[M(noise=9, snr=1.0), M(utterance=2, snr=0.0)], [], [M(utterance=0, gain=1.0), M(utterance=1, gain=1.0), M(utterance=3, snr=2.0)]]
    flat, start, sg, fmt = check(rows, 3, None, None, signalRows=4)
    assert len(flat) == 5 and list(start) == [0, 2, 2, 5]
    assert check(rows, 3, None, None)[0].tobytes() == flat.tobytes()      # the pool's case leaves the sources to the library
    with pytest.raises(ValueError, match=r"mixedTensor: row 2, term 2: source 3 is not a row of the signal \(3\)"):
        check(rows, 3, None, None, signalRows=3)
    with pytest.raises(ValueError, match=r"row 0, term 1: source 2 is not a row of the signal \(2\)"):
        check((flat, start), 3, None, None, signalRows=2)
    with pytest.raises(ValueError, match=r"row 1, term 0: source -1 is not a row of the signal \(4\)"):
        check([[], [M(utterance=-1, gain=1.0)]], 2, None, None, signalRows=4)
    assert len(check([[M(noise=100, snr=0.0)]], 1, None, None, signalRows=0)[0]) == 1      # a clip's number is the bank's, not the signal's
    for bad in (1.5, True, -1, "4"):
        with pytest.raises(TypeError):
            check(rows, 3, None, None, signalRows=bad)


def test_the_index_arithmetic_under_sanitizers(tmp_path):
    """csrc/klatt_sigpower.h (the block walk, the leaf ownership, the load masks, the tree, the Lemma) in a program of its own,
    tests/native/check_signal_power.cpp, against brute force under AddressSanitizer + UBSan.  Nothing loaded into python is run under one."""
    exe = str(tmp_path / "check_signal_power")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_signal_power.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out
