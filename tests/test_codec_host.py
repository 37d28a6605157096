"""The codec export on the host (include/speechPlayer_batch.h: speechPlayer_pcmCode, speechPlayer_signalCode, speechPlayer_codecDecode;
nvspeechplayer_amd.pcmCode, signalCode, codecDecode, codecTable, CODECS; csrc/klatt_codec.h): the product's CPU statements against what
CPython's audioop answered (tests/golden/codec_golden.npz, written by tests/golden/make_codec_golden.py: every int16 value and every code
for the two G.711 laws, 24 rows for IMA ADPCM with the encoder's final state) and against a transcription of the definition written
here in numpy and plain Python, independent of the shared header; the float32 input, round trips, the decode table, every refusal,
and a model of both kernels' walks in a program of its own under the sanitizers (tests/native/check_codec.cpp).  `golden`, `LAWS`,
`adpcm_rows` and `statement` are what tests/test_gpu_codec.py shares.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_convolve_host import bits, x_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
LAWS = ("ulaw", "alaw")
EVERY = np.arange(-32768, 32768, dtype=np.int16)
ADPCM_LENGTHS = (0, 1, 2, 7, 64, 65, 1001, 4096)
ADPCM_KINDS = ("uniform", "sine", "square")
STEP = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
        130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963,
        1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358,
        5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623,
        27086, 29794, 32767]
INDEX = [-1, -1, -1, -1, 2, 4, 6, 8]
_golden = None


def golden():
    """The recorded answers of audioop, read once."""
    global _golden
    if _golden is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "codec_golden.npz")) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def adpcm_rows():
    """(kind, L, x, codes, decoded, (val, idx)) of every ADPCM row of the fixture."""
    g = golden()
    for kind in ADPCM_KINDS:
        for L in ADPCM_LENGTHS:
            key = "adpcm_%s_%d_" % (kind, L)
            yield kind, L, g[key + "x"], g[key + "codes"], g[key + "decoded"], tuple(int(v) for v in g[key + "state"])


def top(v):
    """The bit index of the highest set bit of every element of v > 0 (int64)."""
    return np.floor(np.log2(v.astype(np.float64))).astype(np.int64)      # (exact: v < 2^53)


def ulaw_encode(s):
    v = np.asarray(s, np.int64) >> 2
    m = np.where(v < 0, 0x7F, 0xFF)
    v = np.minimum(np.abs(v), 8158) + 33
    seg = top(v) - 5
    return (((seg << 4) | ((v >> (seg + 1)) & 15)) ^ m).astype(np.uint8)


def ulaw_decode(code):
    c = ~np.asarray(code, np.int64) & 255
    t = (((c & 15) << 3) + 132) << ((c & 0x70) >> 4)
    return np.where(c & 0x80, 132 - t, t - 132).astype(np.int16)


def alaw_encode(s):
    v = np.asarray(s, np.int64) >> 3
    m = np.where(v >= 0, 0xD5, 0x55)
    v = np.where(v >= 0, v, -v - 1)
    seg = np.where(v < 32, 0, top(np.maximum(v, 1)) - 4)
    return (((seg << 4) | np.where(seg < 2, (v >> 1) & 15, (v >> seg) & 15)) ^ m).astype(np.uint8)


def alaw_decode(code):
    c = np.asarray(code, np.int64) ^ 0x55
    t, seg = (c & 15) << 4, (c & 0x70) >> 4
    t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(c & 0x80, t, -t).astype(np.int16)


def adpcm(x):
    """The ADPCM statement, line for line: int16 [L] -> (codes uint8 [L], decoded int16 [L], (val, idx))."""
    val = idx = 0
    codes, dec = np.zeros(len(x), np.uint8), np.zeros(len(x), np.int16)
    for n, s in enumerate(np.asarray(x).tolist()):
        step = STEP[idx]
        diff = s - val
        sign = 8 if diff < 0 else 0
        if sign:
            diff = -diff
        delta, vp = 0, step >> 3
        if diff >= step:
            delta = 4; diff -= step; vp += step
        if diff >= step >> 1:
            delta |= 2; diff -= step >> 1; vp += step >> 1
        if diff >= step >> 2:
            delta |= 1; vp += step >> 2
        val = min(max(val - vp if sign else val + vp, -32768), 32767)
        idx = min(max(idx + INDEX[delta], 0), 88)
        codes[n], dec[n] = delta | sign, val
    return codes, dec, (val, idx)


def adpcm_decode(codes):
    val = idx = 0
    dec = np.zeros(len(codes), np.int16)
    for n, c in enumerate(np.asarray(codes).tolist()):
        step = STEP[idx]
        vp = (step >> 3) + (step if c & 4 else 0) + (step >> 1 if c & 2 else 0) + (step >> 2 if c & 1 else 0)
        val = min(max(val - vp if c & 8 else val + vp, -32768), 32767)
        idx = min(max(idx + INDEX[c & 7], 0), 88)
        dec[n] = val
    return dec


def statement(x, codec, npt=np.int16):
    """(decoded, codes) of a row by the host's statement: signalCode, which takes int16 and float32 rows."""
    import nvspeechplayer_amd as eng
    return eng.signalCode(np.ascontiguousarray(x), codec, codes=True, decoded=True, dtype=npt)


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer as sp
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs in (("speechPlayer_pcmCode", 8), ("speechPlayer_signalCode", 9), ("speechPlayer_codecDecode", 7), ("speechPlayer_batch_exportCoded", 9),
                        ("speechPlayer_batch_exportCodedOf", 10)):
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and len(fn.argtypes) == nargs, name
    section = header.split("through a speech codec")[1].split("speechPlayer_batch_exportCoded(")[0]
    for word in ("0 \"ulaw\", 1 \"alaw\", 2 \"adpcm\"", "ONE PER SAMPLE", "seg = top(v) - 5", "seg = v < 32 ? 0 : top(v) - 4", "INDEX[delta]", "G.722", "G.726", "GSM", "nibbles",
                 "WAV block headers", "packet loss", "live handles", "NodePlayer", "kCodeTile = 1024", "kFilterTile = 64"):
        assert word in section, word
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_codec.h")).read()
    assert '#include "klatt_filter.h"' in shared and "Out of scope" in shared and "filter_load_rows" in shared and "filter_pack" in shared
    table = [int(v) for v in re.search(r"kAdpcmTable\{\{([^}]*)\}\}", shared).group(1).replace("\n", " ").split(",")]
    assert table == STEP and len(STEP) == 89
    assert sp.CODE_TILE == int(re.search(r"constexpr int kCodeTile = (\d+);", shared).group(1)) == 1024
    assert sp.CODECS == ["ulaw", "alaw", "adpcm"] and callable(sp.BatchPlayer.codedTensor)
    for name in ("pcmCode", "signalCode", "codecDecode", "codecTable", "CODECS"):
        assert getattr(nvspeechplayer_amd, name) is getattr(sp, name), name
    # the filter's kernel and the strings its tests read are as they were
    filt = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_filter.h")).read()
    assert "klatt_codec" not in filt


def test_g711_is_audioops_exhaustively():
    """lin2ulaw / lin2alaw of all 65 536 int16 values and ulaw2lin / alaw2lin of all 256 codes: the statement, the transcription and the
    recorded answers agree."""
    import nvspeechplayer_amd as eng
    g = golden()
    all_codes = np.arange(256, dtype=np.uint8)
    for law, enc, dec in (("ulaw", ulaw_encode, ulaw_decode), ("alaw", alaw_encode, alaw_decode)):
        want_codes, want_table = g[law + "_encode"], g[law + "_decode"]
        assert want_codes.shape == (65536,) and want_table.shape == (256,) and want_table.dtype == np.int16
        decoded, codes = eng.pcmCode(EVERY, law, codes=True)
        assert codes.dtype == np.uint8 and decoded.dtype == np.int16
        assert np.array_equal(codes, want_codes), law
        assert np.array_equal(enc(EVERY), want_codes), law
        assert np.array_equal(eng.codecDecode(all_codes, law), want_table), law
        assert np.array_equal(dec(all_codes), want_table), law
        assert np.array_equal(decoded, want_table[want_codes]), law
        assert len(set(want_codes.tolist())) == (255 if law == "ulaw" else 256)      # (mu-law's negative zero is never produced)
        # the codes alone, the decoded samples alone, float32 out
        assert np.array_equal(eng.pcmCode(EVERY, law, codes=True, decoded=False), want_codes)
        assert np.array_equal(eng.pcmCode(EVERY, law), decoded)
        f = eng.pcmCode(EVERY, law, dtype=np.float32)
        assert f.dtype == np.float32 and np.array_equal(bits(f), bits(x_of(decoded)))


def test_adpcm_is_audioops_on_every_row():
    """The 24 rows: codes, decoded samples and the encoder's final (val, idx); the decoder alone rebuilds the same samples and state."""
    import nvspeechplayer_amd as eng
    rows = list(adpcm_rows())
    assert len(rows) == 24 and sorted({r[1] for r in rows}) == sorted(ADPCM_LENGTHS)
    for kind, L, x, codes, decoded, state in rows:
        tag = (kind, L)
        assert x.dtype == np.int16 and len(x) == len(codes) == len(decoded) == L, tag
        (d, c), st = eng.pcmCode(x, "adpcm", codes=True, state=True)
        assert np.array_equal(c, codes) and np.array_equal(d, decoded) and st == state, tag
        tc, td, ts = adpcm(x)
        assert np.array_equal(tc, codes) and np.array_equal(td, decoded) and ts == state, tag
        back, st = eng.codecDecode(codes, "adpcm", state=True)
        assert np.array_equal(back, decoded) and st == state, tag
        assert np.array_equal(adpcm_decode(codes), decoded), tag
        assert c.max(initial=0) <= 15
        f = eng.pcmCode(x, "adpcm", dtype=np.float32)
        assert np.array_equal(bits(f), bits(x_of(decoded))), tag
    big = [r for r in rows if r[1] == 4096]
    assert all(len(set(r[3].tolist())) >= 8 for r in big if r[0] != "square") and any(r[5][1] > 80 for r in big), "the rows exercise the codec"
    assert any(r[4].min() == -32768 and r[4].max() == 32767 for r in big), "the clamp of val is met"


def test_float32_input_is_the_int16_it_rounds_to():
    """pcmCode of float32(s / 32767) equals pcmCode of s for all 65 536 s, every codec; values beyond +-1 clip; halves round to even."""
    import nvspeechplayer_amd as eng
    x = x_of(EVERY)
    shuffled = np.random.default_rng(5).permutation(65536)
    for codec in eng.CODECS:
        rows = (EVERY, x) if codec != "adpcm" else (EVERY[shuffled], x[shuffled])
        d16, c16 = eng.pcmCode(rows[0], codec, codes=True)
        d32, c32 = eng.signalCode(rows[1], codec, codes=True)
        assert np.array_equal(c16, c32) and np.array_equal(d16, d32), codec
        d, c = eng.signalCode(rows[0], codec, codes=True)
        assert np.array_equal(c16, c) and np.array_equal(d16, d), codec
    beyond = np.array([1.0, 1.0001, 2.0, 65536.0, -1.0, -32768 / 32767, -1.001, -65536.0, 0.0, -0.0], np.float32)
    as16 = np.array([32767] * 4 + [-32767, -32768, -32768, -32768, 0, 0], np.int16)
    for codec in eng.CODECS:
        a, b = eng.signalCode(beyond, codec, codes=True), eng.pcmCode(as16, codec, codes=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), codec
    halves = (np.array([0.5, 1.5, 2.5, -0.5, -1.5], np.float64) / 32767.0).astype(np.float32)
    q = np.rint(halves * np.float32(32767.0)).astype(np.int16)      # (the statement's product, rounded to nearest even)
    assert np.array_equal(eng.signalCode(halves, "adpcm", codes=True, decoded=False), eng.pcmCode(q, "adpcm", codes=True, decoded=False))


def test_round_trips_and_the_table():
    """decode(encode(decode(c))) == decode(c) for all 256 codes of both laws (compared on the decoded values: mu-law's negative zero
    re-encodes to positive zero); codecTable is codecDecode of the 256 codes; codecDecode of pcmCode's codes is its decoded output."""
    import nvspeechplayer_amd as eng
    all_codes = np.arange(256, dtype=np.uint8)
    for law in LAWS:
        table = eng.codecTable(law)
        assert table.dtype == np.int16 and np.array_equal(table, eng.codecDecode(all_codes, law))
        d = eng.codecDecode(all_codes, law)
        again = eng.pcmCode(d, law, codes=True, decoded=False)
        assert np.array_equal(eng.codecDecode(again, law), d), law
        differ = np.flatnonzero(again != all_codes)
        assert list(differ) == ([0x7F] if law == "ulaw" else []), (law, differ)
    with pytest.raises(ValueError):
        eng.codecTable("adpcm")
    rng = np.random.default_rng(8)
    x = rng.integers(-32768, 32768, 3000).astype(np.int16)
    for codec in eng.CODECS:
        d, c = eng.pcmCode(x, codec, codes=True)
        assert np.array_equal(eng.codecDecode(c, codec), d), codec
        assert np.array_equal(bits(eng.codecDecode(c, codec, dtype=np.float32)), bits(x_of(d))), codec
    # a codec by its number
    assert np.array_equal(eng.pcmCode(x, 2), eng.pcmCode(x, "adpcm"))


def test_binding_request_checks():
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer as sp
    assert sp.check_codec_request("alaw", True, False, None) == (1, True, False, 0)
    assert sp.check_codec_request(2, False, True, torch.float32) == (2, False, True, 1)
    assert sp.check_codec_request("ulaw", True, True, np.int16) == (0, True, True, 0)
    x = np.zeros(4, np.int16)
    for bad in ("g722", 3, -1, None, True, 1.0):
        with pytest.raises(KeyError):
            eng.pcmCode(x, bad)
    with pytest.raises(ValueError):
        eng.pcmCode(x, "ulaw", codes=False, decoded=False)
    for kw in (dict(codes=1), dict(decoded=None), dict(dtype=np.float64), dict(dtype=torch.int32)):
        with pytest.raises(TypeError):
            eng.pcmCode(x, "ulaw", **kw)
    for pcm in (np.zeros(4, np.float32), np.zeros((2, 2), np.int16)):
        with pytest.raises(TypeError):
            eng.pcmCode(pcm, "ulaw")
    for codes in (np.zeros(4, np.int16), [1, 2], np.zeros((2, 2), np.uint8)):
        with pytest.raises(TypeError):
            eng.codecDecode(codes, "ulaw")
    with pytest.raises(TypeError):
        eng.signalCode(np.zeros(4, np.float64), "ulaw")
    with pytest.raises(RuntimeError, match="sample 2 is"):
        eng.signalCode(np.array([0, 0, np.nan], np.float32), "alaw")
    with pytest.raises(RuntimeError, match="code 1 is 16"):
        eng.codecDecode(np.array([15, 16], np.uint8), "adpcm")
    # rows of nothing
    for codec in eng.CODECS:
        d, c = eng.pcmCode(np.zeros(0, np.int16), codec, codes=True)
        assert d.shape == c.shape == (0,) and eng.codecDecode(c, codec).shape == (0,)


def test_every_refusal_of_the_c_entry_points():
    """Every refusal of speechPlayer_pcmCode, signalCode and codecDecode writes nothing and names its entry point."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    pcm = np.arange(200, dtype=np.int16)
    dec = np.full(300, -7, np.int16)
    codes = np.full(300, 201, np.uint8)
    state = np.full(2, -9, np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def run(pcm=pcm, length=200, codec=2, fmt=0, dec=dec, codes=codes, capacity=300, of_signal=None):
        if of_signal is None:
            return L.speechPlayer_pcmCode(p(pcm), length, codec, fmt, p(dec), p(codes), capacity, p(state))
        return L.speechPlayer_signalCode(p(pcm), of_signal, length, codec, fmt, p(dec), p(codes), capacity, p(state))

    def untouched():
        return np.all(dec == -7) and np.all(codes == 201) and np.all(state == -9)

    refused = dict(length_negative=(dict(length=-1), b"length -1"), length_above=(dict(length=(1 << 44) + 1), b"length"), no_pcm=(dict(pcm=None), b"with its samples"),
                   codec_3=(dict(codec=3), b"codec 3"), codec_negative=(dict(codec=-1), b"codec -1"), format_2=(dict(fmt=2), b"format 2"),
                   format_negative=(dict(fmt=-1), b"format -1"), no_output=(dict(dec=None, codes=None), b"no output"), capacity_short=(dict(capacity=199), b"capacity is 199"))
    for name, (kw, words) in refused.items():
        assert run(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"pcmCode" in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        assert untouched(), name
    x = np.linspace(-1, 1, 200).astype(np.float32)
    refused = dict(in_format_2=(dict(of_signal=2), b"input format 2"), in_format_negative=(dict(of_signal=-1), b"input format -1"),
                   sample_nan=(dict(pcm=np.where(np.arange(200) == 9, np.nan, x).astype(np.float32), of_signal=1), b"sample 9 is"),
                   sample_large=(dict(pcm=np.where(np.arange(200) == 9, 65537.0, x).astype(np.float32), of_signal=1), b"sample 9 is"),
                   codec_3=(dict(pcm=x, of_signal=1, codec=3), b"codec 3"), no_output=(dict(pcm=x, of_signal=1, dec=None, codes=None), b"no output"))
    for name, (kw, words) in refused.items():
        assert run(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"signalCode" in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        assert untouched(), name

    out = np.full(300, -7, np.int16)
    ok = np.arange(200, dtype=np.uint8) % 16

    def decode(codes=ok, length=200, codec=2, fmt=0, out=out, capacity=300):
        return L.speechPlayer_codecDecode(p(codes), length, codec, fmt, p(out), capacity, p(state))

    refused = dict(length_negative=(dict(length=-1), b"length -1"), no_codes=(dict(codes=None), b"with its codes"), no_codes_g711=(dict(codes=None, codec=0), b"with its codes"),
                   codec_3=(dict(codec=3), b"codec 3"), format_2=(dict(fmt=2), b"format 2"), no_output=(dict(out=None), b"no output"),
                   capacity_short=(dict(capacity=199), b"capacity is 199"), code_16=(dict(codes=np.where(np.arange(200) == 77, 16, ok).astype(np.uint8)), b"code 77 is 16"),
                   code_255=(dict(codes=np.where(np.arange(200) == 199, 255, ok).astype(np.uint8)), b"code 199 is 255"))
    for name, (kw, words) in refused.items():
        assert decode(**kw) == -1, name
        assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"codecDecode" in L.speechPlayer_lastError() and words in L.speechPlayer_lastError(), (name, L.speechPlayer_lastError())
        assert np.all(out == -7) and np.all(state == -9), name
    # nothing to compute, one output alone, the capacity itself, a G.711 law takes every code, no state asked for -- and all is as usable as before
    assert run(pcm=None, length=0, dec=None, codes=None, capacity=0) == 0 and L.speechPlayer_lastErrorCode() == 0 and list(state) == [0, 0]
    assert decode(codes=None, length=0, out=None, capacity=0) == 0 and L.speechPlayer_lastErrorCode() == 0
    assert run(codes=None, capacity=200) == 200 and np.all(codes == 201) and np.all(dec[200:] == -7) and dec[:200].any()
    assert run(dec=None) == 200 and np.all(codes[200:] == 201) and np.all(codes[:200] <= 15)
    assert decode(codes=np.arange(200, dtype=np.uint8) + 56, codec=0) == 200 and list(state) == [0, 0]
    assert L.speechPlayer_pcmCode(p(pcm), 200, 1, 1, p(np.zeros(200, np.float32)), None, 200, None) == 200
    assert run(pcm=x, of_signal=1) == 200 and tuple(state) != (0, 0)


def test_the_kernels_walks_under_sanitizers(tmp_path):
    """csrc/klatt_codec.h (the statements, a model of the G.711 kernel's tile walk and of the ADPCM kernel's loads, in-place staging and
    stores, the uint8 run included) in a program of its own, tests/native/check_codec.cpp, under AddressSanitizer + UBSan: 0, 1, 63, 64,
    65 and 130 rows, lengths around both tiles, packed and padded, misaligned outputs -- every output element written exactly once,
    nothing outside input or output touched, the statement's bits.  Nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_codec")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_codec.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out
