"""Signal stages that keep a window, without a GPU (include/speechPlayer_batch.h, "Signal stages that keep a window";
csrc/klatt_stage_window.h): the entry points are declared, exported and bound; speechPlayer_spectrogramEmitted against a brute-force count;
the host model of both kinds, tests/native/check_stage_window.cpp, in a program of its own under AddressSanitizer + UBSan; every refusal of
check_stage_request and check_stage_push for the two kinds, and the refusals of the C entry points that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer as sp
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs, restype in (("speechPlayer_batch_stageConvolve", 7, ctypes.c_void_p), ("speechPlayer_batch_stageSpectrogram", 11, ctypes.c_void_p),
                                 ("speechPlayer_spectrogramEmitted", 5, ctypes.c_longlong)):
        assert name + "(" in header and name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is restype and len(fn.argtypes) == nargs, name
    old, new = header.split(" * Signal stages that keep a window:")
    new = new.split("speechPlayer_spectrogramEmitted(long long consumed")[0]
    for word in ("Lemma", "K_r - 1", "nFft - 1", "before + after", "floor((N - after - 1 - phase) / hop) + 1", "ceil((N - phase) / hop)", "THE STATE UNCHANGED",
                 "2^27", "2^20", "2^44", "BIT FOR BIT", "4 ulp", "0 is float64", "in STEPS", "ends a chain", "[history | chunk | +0]", "deviceCodes", "LPC, pitch and tempo",
                 "mix stage", "klatt_stage_window.h"):
        assert word in new, word
    for maker in ("speechPlayer_batch_stageConvolve);", "speechPlayer_batch_stageSpectrogram)."):
        assert maker in old.split(" * Signal stages:")[0], maker      # the whole-row exports' notes point at the new makers
    assert "speechPlayer_batch_stageConvolve, speechPlayer_batch_stageSpectrogram" in old.split(" * Signal stages:")[1]      # ... and so does the first section
    shared = open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_stage_window.h")).read()
    for word in ('#include "klatt_stage.h"', '#include "klatt_convolve.h"', '#include "klatt_spectrum.h"', "The lemma", "kStageMaxHistory = 1ll << 27",
                 "klatt_stage_convolve", "klatt_stage_spectrogram", "klatt_stage_history_rows", "conv_rows<true, F32, In>(", "spec_rows<F32>(", "stage_sample("):
        assert word in shared, word
    # one body per family, called by the whole-row kernel and by the stage's; the tap chain and the transform are called, not restated
    csrc = os.path.join(ROOT, "nvspeechplayer_amd", "csrc")
    conv, spec = open(os.path.join(csrc, "klatt_convolve.h")).read(), open(os.path.join(csrc, "klatt_spectrum.h")).read()
    assert conv.count("conv_step4(acc, v, h4)") == 1 and "conv_rows<false, F32, In>(" in conv and "conv_step4(" not in shared
    assert spec.count("spec_unpack(z[") == 2 and "spec_rows<F32>(" in spec and "spec_unpack(" not in shared.split("#pragma once")[1]
    assert os.path.exists(os.path.join(ROOT, "profiles", "stage_window_kernels.txt"))
    assert sp.STAGE_MAX_HISTORY == 1 << 27 and sp.STAGE_KINDS[3:] == ["convolution", "spectrogram"] and sp.STAGE_KINDS[:3] == ["resample", "filter", "code"]
    assert '#include "klatt_stage_window.h"' in open(os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "klatt_engine.hip")).read()
    for name in ("convolveStage", "spectrogramStage"):
        assert callable(getattr(sp.BatchPlayer, name)), name
    assert nvspeechplayer_amd.spectrogramEmitted is sp.spectrogramEmitted and "spectrogramEmitted" in nvspeechplayer_amd.__all__
    assert "4.27" in open(os.path.join(ROOT, "docs", "KERNELS.md")).read() and "spectrogramStage" in open(os.path.join(ROOT, "README.md")).read()
    assert "klatt_stage_window.h" in open(os.path.join(ROOT, "DESIGN.md")).read()


@pytest.mark.parametrize("nFft", [64, 256])
def test_spectrogram_emitted_is_the_brute_force_count(nFft):
    """For N = 0 .. 3 nFft + hop consumed samples: open, the j with c_j + nFft / 2 - 1 <= N - 1 -- the whole frame at or before the last
    sample consumed --; ended, the statement's count, the j with c_j < N.  hop 300 is above nFft = 256: samples are skipped."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd.speechPlayer import _step_counts
    for hop in (1, 7, 64, 256, 300):
        for phase in sorted({0, 5, hop - 1, nFft, nFft + 3}):
            for N in range(3 * nFft + hop + 1):
                centres = range(phase, N + nFft, hop)
                opened = sum(1 for c in centres if c + nFft // 2 - 1 <= N - 1)
                ended = sum(1 for c in centres if c < N)
                assert eng.spectrogramEmitted(N, nFft, hop, phase) == opened, (hop, phase, N, "open")
                assert eng.spectrogramEmitted(N, nFft, hop, phase, ended=True) == ended == int(_step_counts(N, hop, phase)), (hop, phase, N, "ended")


def test_the_host_model_of_both_kinds_under_sanitizers(tmp_path):
    """tests/native/check_stage_window.cpp: the header's bookkeeping and the shared statements driven chunk by chunk equal convolve_host and
    spectrogram_host on the concatenation -- chunks of 0, 1, K - 2, K - 1, K and 2 K for K in 1, 2, 5 and 1025 taps; of 0, 1, hop - 1, hop,
    nFft / 2 - 1, nFft / 2, nFft - 1 and nFft; a stream that stays below K - 1 / below one frame until it ends, an end with an empty last
    chunk, a row reused after its end -- under AddressSanitizer + UBSan, every chunk in an allocation of exactly its size.  Nothing loaded
    into python is run under a sanitizer."""
    exe = str(tmp_path / "check_stage_window")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_stage_window.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out


def test_every_refusal_of_check_stage_request_for_the_two_kinds():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    check = sp.check_stage_request
    kind, n, (h, start, of, tail, fmt) = check("convolution", 3, [[1.0, 0.5], np.ones(5)], irOf=[1, 0, 1], tail=False)
    assert (kind, n, tail, fmt) == (3, 3, 0, 1) and list(start) == [0, 2, 7] and list(of) == [1, 0, 1] and h.dtype == np.float32
    assert check("convolution", 2, np.ones(4))[2][2:4] == (None, 1)
    kind, n, plan = check("spectrogram", 4, 512, 160, log="db")
    assert (kind, n) == (4, 4) and plan[:3] == (512, 160, 0) and plan[5:] == (257, 2, 10.0, 1e-10, 1)
    assert check("spectrogram", 1, bank=sp.melFilterbank(22050, 1024, 20))[2][5] == 20
    with pytest.raises(KeyError, match="convolve"):
        check("convolve", 1, np.ones(4))
    for kind, maker, args in (("convolution", "convolveStage", (np.ones(4),)), ("spectrogram", "spectrogramStage", ())):
        for bad in (0, -1, (1 << 20) + 1):
            with pytest.raises(ValueError, match=maker + ": nRows"):
                check(kind, bad, *args)
        for bad in (1.0, True, "3", None):
            with pytest.raises(TypeError, match=maker + ": nRows"):
                check(kind, bad, *args)
    # the convolution's arguments: check_convolve_request's refusals, under the maker's name
    for bad, error, word in (([], ValueError, "at least one"), (np.ones((2, 2)), TypeError, "irs must be"), ([np.ones(3), np.ones((2, 2))], TypeError, "response 1"),
                             (np.ones(65537), ValueError, "65537 taps"), ([np.ones(65536)] * 17, ValueError, "taps in all"), ([1.0, float("nan")], ValueError, "tap 1 of response 0"),
                             ([1.0, 1e10], ValueError, "2\\^32"), ("room", TypeError, "irs must be")):
        with pytest.raises(error, match="convolveStage: .*" + word):
            check("convolution", 2, bad)
    with pytest.raises(ValueError, match="convolveStage: irOf is needed"):
        check("convolution", 2, [np.ones(2), np.ones(3)])
    with pytest.raises(ValueError, match="convolveStage: irOf has 3 entries for 2 rows"):
        check("convolution", 2, [np.ones(2), np.ones(3)], irOf=[0, 1, 0])
    with pytest.raises(ValueError, match="convolveStage: irOf must lie"):
        check("convolution", 2, [np.ones(2), np.ones(3)], irOf=[0, 2])
    with pytest.raises(TypeError, match="convolveStage: irOf"):
        check("convolution", 2, [np.ones(2), np.ones(3)], irOf=[0.0, 1.0])
    with pytest.raises(ValueError, match="convolveStage: tail"):
        check("convolution", 2, np.ones(2), tail=2)
    with pytest.raises(ValueError, match="convolveStage: .*histories.*2\\^27"):
        check("convolution", 1 << 20, np.ones(65536))
    assert check("convolution", 1 << 11, np.ones(65536))[1] == 1 << 11      # 2^11 (2^16 - 1) < 2^27
    with pytest.raises(ValueError, match="convolveStage: .*histories"):
        check("convolution", 3000, [np.ones(65536), np.ones(2)], irOf=[0] * 2100 + [1] * 900)
    # the spectrogram's: check_spectrogram_request's refusals, under the maker's name
    for kw, error, word in ((dict(nFft=100), ValueError, "power of two"), (dict(nFft=32), ValueError, "power of two"), (dict(nFft=8192), ValueError, "power of two"),
                            (dict(nFft=64.0), ValueError, "integer"), (dict(hop=0), ValueError, "hop"), (dict(phase=-1), ValueError, "phase"),
                            (dict(window=np.ones(5)), ValueError, "window needs"), (dict(nFft=64, window=np.full(64, np.inf)), ValueError, "window value"),
                            (dict(bank=np.ones((3, 5))), ValueError, "bank must be"), (dict(nFft=64, bank=np.full((2, 33), np.nan)), ValueError, "bank value"),
                            (dict(power=3), ValueError, "power"), (dict(log="bel"), ValueError, "log must be"), (dict(log="db", floor=0.0), ValueError, "floor > 0"),
                            (dict(log=float("inf")), ValueError, "finite")):
        with pytest.raises(error, match="spectrogramStage: .*" + word):
            check("spectrogram", 2, **kw)
    with pytest.raises(ValueError, match="spectrogramStage: .*histories.*2\\^27"):
        check("spectrogram", 1 << 20, 4096)
    assert check("spectrogram", 1 << 20, 128)[1] == 1 << 20      # 2^20 x 127 < 2^27
    # a push
    push = sp.check_stage_push
    x = torch.zeros((3, 8), dtype=torch.int16)
    assert push("convolution", 3, (x, [8, 0, 3]), end=[True, False, True])[2:] == (1, False, True)
    assert push("convolution", 3, (x, [8, 0, 3]), dtype=torch.int16)[2] == 0
    assert push("spectrogram", 3, (x, [8, 0, 3]))[2] == 1 and push("spectrogram", 3, (x, [8, 0, 3]), dtype=torch.float64)[2] == 0
    with pytest.raises(TypeError, match="dtype"):
        push("spectrogram", 3, (x, [8, 0, 3]), dtype=torch.int16)
    with pytest.raises(TypeError, match="dtype"):
        push("convolution", 3, (x, [8, 0, 3]), dtype=torch.float64)
    for kind in ("convolution", "spectrogram"):
        with pytest.raises(ValueError, match="code stage"):
            push(kind, 3, (x, [8, 0, 3]), codes=True)
        with pytest.raises(ValueError, match="code stage"):
            push(kind, 3, (x, [8, 0, 3]), decoded=False)
        with pytest.raises(ValueError, match="3 rows for a stage of 4"):
            push(kind, 4, (x, [8, 0, 3]))
        with pytest.raises(ValueError, match="end has 2"):
            push(kind, 3, (x, [8, 0, 3]), end=[True, False])


def test_the_refusals_of_the_c_entry_points_that_need_no_device():
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()

    def refused(got, word):
        assert got in (-1, None) and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and word in L.speechPlayer_lastError(), (got, word, L.speechPlayer_lastError())

    refused(L.speechPlayer_spectrogramEmitted(-1, 512, 160, 0, 0), b"spectrogramEmitted")
    refused(L.speechPlayer_spectrogramEmitted((1 << 44) + 1, 512, 160, 0, 0), b"2^44")
    for nFft in (0, 32, 100, 8192):
        refused(L.speechPlayer_spectrogramEmitted(10, nFft, 160, 0, 0), b"power of two")
    refused(L.speechPlayer_spectrogramEmitted(10, 512, 0, 0, 1), b"hop")
    refused(L.speechPlayer_spectrogramEmitted(10, 512, 160, -1, 1), b"phase")
    assert L.speechPlayer_spectrogramEmitted(1 << 44, 64, 1, 0, 1) == 1 << 44 and L.speechPlayer_lastErrorCode() == 0
    assert L.speechPlayer_spectrogramEmitted(1 << 44, 64, 1, 0, 0) == (1 << 44) - 31
    assert L.speechPlayer_spectrogramEmitted(1 << 44, 4096, 1 << 50, 1 << 50, 1) == 0      # (a hop or phase beyond any row means the same as 2^40)
    for bad in ((-1, 512, 160, 0), (10, 100, 160, 0), (10, 512, 0, 0), (10, 512, 160, -1)):
        with pytest.raises(ValueError, match="spectrogramEmitted"):
            eng.spectrogramEmitted(*bad)
    h, start = np.ones(4, np.float32), np.array([0, 4], np.int64)
    refused(L.speechPlayer_batch_stageConvolve(None, 1, h.ctypes.data, start.ctypes.data, 1, None, 1), b"stageConvolve: no batch")
    refused(L.speechPlayer_batch_stageSpectrogram(None, 1, 512, 160, 0, None, None, 0, 2, 0.0, 1e-10), b"stageSpectrogram: no batch")
