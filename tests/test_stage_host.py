"""Signal stages without a GPU (include/speechPlayer_batch.h, "Signal stages"; csrc/klatt_stage.h): the entry points are declared, exported
and bound; speechPlayer_resampleEmitted against a brute-force count; the host model of every stage kind, tests/native/check_stage.cpp, in
a program of its own under AddressSanitizer + UBSan; every refusal of check_stage_request and check_stage_push, and the refusals of the C
entry points that need no device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
# srcRate, dstRate: the ratios up / down = 320/441, 320/147, 2/1, 160/441, 1/2, 1/12 and 1/1
RATES = [(22050, 16000), (22050, 48000), (22050, 44100), (22050, 8000), (22050, 11025), (48000, 4000), (16000, 16000)]


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer as sp
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs, restype in (("speechPlayer_batch_stageResample", 8, ctypes.c_void_p), ("speechPlayer_batch_stageFilter", 7, ctypes.c_void_p),
                                 ("speechPlayer_batch_stageCode", 3, ctypes.c_void_p), ("speechPlayer_stage_plan", 4, ctypes.c_longlong),
                                 ("speechPlayer_stage_push", 9, ctypes.c_longlong), ("speechPlayer_stage_reset", 3, ctypes.c_int),
                                 ("speechPlayer_stage_counts", 3, ctypes.c_int), ("speechPlayer_stage_free", 1, None),
                                 ("speechPlayer_resampleEmitted", 6, ctypes.c_longlong)):
        assert name + "(" in header and name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is restype and len(fn.argtypes) == nargs, name
    section = header.split(" * Signal stages:")[1].split("typedef void* speechPlayer_stage_t;")[0]
    for word in ("Lemma", "2 Z - 1", "THE STATE UNCHANGED", "2^44", "2^20", "freed", "neither output", "not a code stage", "overlaps the chunk", "NodePlayer",
                 "fused kernel", "saving a stage's state", "convolution, spectrogram, LPC, pitch and tempo", "ceil(max(N' - Z, 0) up / down)"):
        assert word in section, word
    for name, maker in (("klatt_resample.h", "klatt_stage.h"), ("klatt_filter.h", "klatt_stage.h"), ("klatt_codec.h", "klatt_stage.h")):
        assert maker in open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", name)).read(), name
    for maker in ("speechPlayer_batch_stageResample);", "speechPlayer_batch_stageFilter);", "speechPlayer_batch_stageCode);"):
        assert maker in header.split(" * Signal stages:")[0], maker      # the whole-row exports' notes point at the stages
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_stage.h")).read()
    assert '#include "klatt_codec.h"' in shared and "The lemma" in shared and "Out of scope" in shared
    assert "kStageMaxRows = 1ll << 20" in shared and sp.STAGE_MAX_ROWS == 1 << 20
    assert '#include "klatt_stage.h"' in open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_engine.hip")).read()
    for name in ("resampleStage", "filterStage", "codeStage"):
        assert callable(getattr(sp.BatchPlayer, name)), name
    for name in ("push", "reset", "close", "plan"):
        assert callable(getattr(sp.SignalStage, name)), name
    assert isinstance(sp.SignalStage.consumed, property) and isinstance(sp.SignalStage.emitted, property)
    for name in ("SignalStage", "SignalChain", "resampleEmitted", "check_stage_request", "check_stage_push"):
        assert getattr(nvspeechplayer_amd, name) is getattr(sp, name), name
    assert "Signal stages" in open(os.path.join(ROOT, "docs", "KERNELS.md")).read() and "SignalChain" in open(os.path.join(ROOT, "README.md")).read()


@pytest.mark.parametrize("rates", RATES)
def test_resample_emitted_is_the_brute_force_count(rates):
    """For N = 0 .. 4 Z + 3 consumed samples: open, the m with floor(m down / up) + Z <= N - 1 -- every tap at or before the last sample
    consumed --; ended, the statement's length.  Equal rates filter nothing (y[m] = x[m]): no taps, Z = 0 in the count."""
    import nvspeechplayer_amd as eng
    src, dst = rates
    g = math.gcd(src, dst)
    up, down = dst // g, src // g
    taps = eng.resampleKernel(src, dst)[0].shape[1]
    Z = 0 if src == dst else taps // 2
    assert src == dst or Z == math.ceil(6 / (0.99 * min(1.0, up / down)))
    for N in range(4 * (taps // 2) + 4):
        brute = sum(1 for m in range((N + 2) * up) if m * down // up + Z <= N - 1)
        assert eng.resampleEmitted(N, src, dst) == brute, (N, "open")
        assert eng.resampleEmitted(N, src, dst, ended=True) == -(-N * up // down) == eng.speechPlayer.resampledLength(N, src, dst), (N, "ended")
    assert (up, down) in {(320, 441), (320, 147), (2, 1), (160, 441), (1, 2), (1, 12), (1, 1)}


def test_the_host_model_of_every_stage_under_sanitizers(tmp_path):
    """tests/native/check_stage.cpp: the header's bookkeeping and the shared statements driven chunk by chunk equal resample_host,
    filter_host and code_host on the concatenation -- chunks of 0, 1, Z - 1, Z, 2 Z - 2, 2 Z - 1 and 2 Z, a stream that stays below Z
    until it ends, an end with an empty last chunk, a row reused after its end -- under AddressSanitizer + UBSan, every chunk in an
    allocation of exactly its size.  Nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_stage")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_stage.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out


def test_every_refusal_of_check_stage_request():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    from tests.test_filter_host import TELEPHONE, stable
    check = sp.check_stage_request
    kind, n, plan = check("resample", 5, 22050, 8000)
    assert (kind, n) == (0, 5) and plan[:6] == (22050, 8000, 6, 0.99, 0, 0.0) and plan[7:] == (160, 441, 2 * math.ceil(6 / (0.99 * 160 / 441)))
    kind, n, (sec, start, of, tail, _) = check("filter", 3, [TELEPHONE, stable(2, 1)], filterOf=[1, 0, 1], tail=7)
    assert (kind, n, tail) == (1, 3, 7) and list(start) == [0, 4, 6] and list(of) == [1, 0, 1] and sec.shape == (6, 5)
    assert check("code", 1 << 20, "adpcm")[::2] == (2, (2, True, True, 0)) and check("code", 1, 0)[2][0] == 0
    with pytest.raises(KeyError):
        check("convolve", 1)
    for bad in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="nRows"):
            check("code", bad, "ulaw")
    for bad in (1.0, True, "3", None):
        with pytest.raises(TypeError, match="nRows"):
            check("code", bad, "ulaw")
    # what the plans refuse, in the stage's name
    for kw in (dict(srcRate=0), dict(rate=-8000), dict(zeros=0), dict(rolloff=0.0), dict(rolloff=1.5), dict(rolloff=float("nan")), dict(window="blackman"),
               dict(window="kaiser", beta=-1.0), dict(rate=22051), dict(rate=100, zeros=200), dict(srcRate=3, rate=4096, zeros=150)):
        args = dict(srcRate=22050, rate=16000, zeros=6, rolloff=0.99, window="hann", beta=None)
        args.update(kw)
        with pytest.raises(ValueError, match="resampleStage"):
            check("resample", 2, **args)
    with pytest.raises(TypeError, match="resampleStage"):
        check("resample", 2, 22050.0, 16000)
    with pytest.raises(ValueError, match="filterStage"):
        check("filter", 2, [TELEPHONE, TELEPHONE])                      # two filters and no filterOf
    with pytest.raises(ValueError, match="filterStage"):
        check("filter", 2, TELEPHONE, filterOf=[0])                     # filterOf is per row of the stage
    with pytest.raises(ValueError, match="filterStage"):
        check("filter", 2, TELEPHONE, filterOf=[0, 1])
    with pytest.raises(ValueError, match="filterStage"):
        check("filter", 2, TELEPHONE, tail=-1)
    with pytest.raises(ValueError, match="filterStage"):
        check("filter", 2, np.zeros((17, 5), np.float32))
    with pytest.raises(TypeError, match="filterStage"):
        check("filter", 2, np.zeros((2, 4), np.float32))
    for bad in ("gsm", 3, -1, True):
        with pytest.raises(KeyError, match="codeStage"):
            check("code", 2, bad)
    # a push
    push = sp.check_stage_push
    x = torch.zeros((3, 8), dtype=torch.int16)
    sig, flags, fmt, codes, decoded = push("filter", 3, (x, [8, 0, 3]), end=[True, False, True])
    assert sig[2] == 3 and list(flags) == [1, 0, 1] and (fmt, codes, decoded) == (1, False, True)
    flags = push("code", 3, (x, [8, 0, 3]), end=True, codes=True)
    assert list(flags[1]) == [1, 1, 1] and flags[2:] == (0, True, True) and push("resample", 3, (x, [1, 2, 3]))[1] is None
    assert list(push("resample", 3, (x.float().reshape(-1), [0, 8, 8, 24]), end=False, dtype=torch.int16)[1]) == [0, 0, 0]
    with pytest.raises(ValueError, match="3 rows for a stage of 4"):
        push("filter", 4, (x, [8, 0, 3]))
    with pytest.raises(ValueError, match="end has 2"):
        push("filter", 3, (x, [8, 0, 3]), end=[True, False])
    for bad in ([1, 0, 1], "yes", [[True, False, True]]):
        with pytest.raises(TypeError, match="end"):
            push("filter", 3, (x, [8, 0, 3]), end=bad)
    with pytest.raises(ValueError, match="code stage"):
        push("filter", 3, (x, [8, 0, 3]), codes=True)
    with pytest.raises(ValueError, match="code stage"):
        push("resample", 3, (x, [8, 0, 3]), decoded=False)
    with pytest.raises(ValueError, match="codes, decoded or both"):
        push("code", 3, (x, [8, 0, 3]), decoded=False)
    with pytest.raises(TypeError, match="codes"):
        push("code", 3, (x, [8, 0, 3]), codes=1)
    with pytest.raises(TypeError, match="dtype"):
        push("filter", 3, (x, [8, 0, 3]), dtype=torch.float64)
    with pytest.raises(ValueError, match="row 1 has 9 samples"):
        push("filter", 3, (x, [8, 9, 3]))
    with pytest.raises(TypeError):
        push("filter", 3, x)
    with pytest.raises(KeyError):
        push("tempo", 3, (x, [8, 0, 3]))
    with pytest.raises(TypeError, match="SignalChain"):
        sp.SignalChain([])


def test_the_refusals_of_the_c_entry_points_that_need_no_device():
    from nvspeechplayer_amd import _native
    L = _native.load()

    def refused(got, word):
        assert got in (-1, None) and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and word in L.speechPlayer_lastError(), (got, word, L.speechPlayer_lastError())

    refused(L.speechPlayer_resampleEmitted(-1, 22050, 16000, 6, 0.99, 0), b"resampleEmitted")
    refused(L.speechPlayer_resampleEmitted((1 << 44) + 1, 22050, 16000, 6, 0.99, 0), b"2^44")
    refused(L.speechPlayer_resampleEmitted(10, 0, 16000, 6, 0.99, 0), b"sample rates")
    refused(L.speechPlayer_resampleEmitted(10, 22050, 16000, 0, 0.99, 0), b"zeros")
    refused(L.speechPlayer_resampleEmitted(10, 22050, 16000, 6, 1.5, 1), b"rolloff")
    refused(L.speechPlayer_resampleEmitted(10, 22050, 22051, 6, 0.99, 1), b"up is above")
    assert L.speechPlayer_resampleEmitted(1 << 44, 22050, 48000, 6, 0.99, 1) == -(-(1 << 44) * 320 // 147) and L.speechPlayer_lastErrorCode() == 0
    # no batch, no stage, and a handle that names no stage
    refused(L.speechPlayer_batch_stageResample(None, 1, 22050, 16000, 6, 0.99, 0, 0.0), b"stageResample: no batch")
    refused(L.speechPlayer_batch_stageFilter(None, 1, None, None, 1, None, 0), b"stageFilter: no batch")
    refused(L.speechPlayer_batch_stageCode(None, 1, 0), b"stageCode: no batch")
    lens = np.zeros(4, np.int64)
    word = ctypes.c_longlong(0)
    for handle, text in ((None, b"no stage"), (ctypes.addressof(word), b"is not a stage")):
        refused(L.speechPlayer_stage_plan(handle, lens.ctypes.data, None, None), text)
        refused(L.speechPlayer_stage_push(handle, None, None, None, 1, None, 0, None, None), text)
        refused(L.speechPlayer_stage_reset(handle, None, None), text)
        refused(L.speechPlayer_stage_counts(handle, lens.ctypes.data, None), text)
        L.speechPlayer_stage_free(handle)      # frees nothing
