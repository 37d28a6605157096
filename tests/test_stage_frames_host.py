"""Signal stages on the step grid, without a GPU (include/speechPlayer_batch.h, "Signal stages on the step grid";
csrc/klatt_stage_frames.h): the entry points are declared, exported and bound; speechPlayer_lpcEmitted / pitchEmitted against a brute-force
count; the host model of both kinds, tests/native/check_stage_frames.cpp, in a program of its own under AddressSanitizer + UBSan; every
refusal of check_stage_request and check_stage_push for the two kinds and of SignalChain's fan, and the refusals of the C entry points that
need no device; and the condition that keeps tests/test_gpu_stage_frames.py honest, on the host statements for its very inputs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import stage_frames as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1


def test_entry_points_are_declared_exported_and_bound():
    import nvspeechplayer_amd
    from nvspeechplayer_amd import _native, speechPlayer as sp
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name, nargs, restype in (("speechPlayer_batch_stageLpc", 9, ctypes.c_void_p), ("speechPlayer_batch_stagePitch", 10, ctypes.c_void_p),
                                 ("speechPlayer_lpcEmitted", 5, ctypes.c_longlong), ("speechPlayer_pitchEmitted", 6, ctypes.c_longlong)):
        assert name + "(" in header and name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is restype and len(fn.argtypes) == nargs, name
        declared = header.split(name + "(")[1].split(");")[0]
        assert declared.count(",") + 1 == nargs, name
    assert header.count(" * Signal stages on the step grid:") == 1 and header.count(" * Signal stages that keep a window:") == 1 and header.count(" * Signal stages:") == 1
    section = header.split(" * Signal stages on the step grid:")[1].split("speechPlayer_pitchEmitted(long long consumed")[0]
    assert header.index(" * Signal stages that keep a window:") < header.index(" * Signal stages on the step grid:")
    for word in ("floor(nWin / 2), nWin - 1 - floor(nWin / 2)", "Nf = W + lagMax", "H = nWin - 1", "H = Nf - 1", "before + after", "lemma", "2^45", "2^27", "2^20", "2^44",
                 "BIT FOR BIT", "no ulp bar", "0 is float64", "in STEPS", "ends a chain", "deviceCodes is refused", "THE STATE UNCHANGED", "fresh row",
                 "floor((N - after - 1 - phase) / hop) + 1", "ceil((N - phase) / hop)", "speechPlayer_batch_exportLpcResidual", "nearest", "tempo", "mix stage",
                 "saving a stage's state", "NodePlayer", "fused kernel", "klatt_stage_frames.h", "uploaded once"):
        assert word in section, word
    csrc = os.path.join(ROOT, "nvspeechplayer_amd", "csrc")
    shared = open(os.path.join(csrc, "klatt_stage_frames.h")).read()
    for word in ('#include "klatt_stage.h"', '#include "klatt_lpc.h"', '#include "klatt_pitch.h"', "klatt_stage_lpc", "klatt_stage_pitch", "lpc_rows<F32>(", "pitch_rows<F32>(",
                 "stage_sample(", "row.outLen", "(row.M + j) * A.hop"):
        assert word in shared, word
    # one body per family, called by the whole-row kernel and by the stage's; nothing per sample is restated
    lpc, pitch = open(os.path.join(csrc, "klatt_lpc.h")).read(), open(os.path.join(csrc, "klatt_pitch.h")).read()
    assert lpc.count("lpc_levinson(r, order, a, k, E, stages)") == 1 and lpc.count("lpc_rows<F32>(") == 1 and "lpc_levinson(" not in shared.split("#pragma once")[1]
    assert pitch.count("pitch_lane_choice(dm,") == 1 and pitch.count("pitch_rows<F32>(") == 1 and "pitch_cmnd(" not in shared.split("#pragma once")[1]
    stage = open(os.path.join(csrc, "klatt_stage.h")).read()
    for word in ("kStageLpc = 5", "kStagePitch = 6", "stage_lpc_frames(int nWin, long long hop, long long phase)", "stage_pitch_frames(int nWin, int lagMax, long long hop, long long phase)",
                 "stage_has_frames(g.kind)", "klatt_stage_frames.h"):
        assert word in stage, word
    engine = open(os.path.join(csrc, "klatt_engine.hip")).read()
    assert '#include "klatt_stage_frames.h"' in engine and engine.count("packed_row_table(sel.counts.data()") == 1      # one step table for every frame kind
    assert sp.STAGE_FRAME_KINDS == ["lpc", "pitch"] and sp.STAGE_KINDS == ["resample", "filter", "code", "convolution", "spectrogram"]
    assert sp.check_stage_request("lpc", 2)[0] == 5 and sp.check_stage_request("pitch", 2, 16000)[0] == 6
    for name in ("lpcStage", "pitchStage"):
        assert callable(getattr(sp.BatchPlayer, name)), name
    for name in ("lpcEmitted", "pitchEmitted", "STAGE_FRAME_KINDS"):
        assert getattr(nvspeechplayer_amd, name) is getattr(sp, name) and name in nvspeechplayer_amd.__all__, name
    assert "4.28" in open(os.path.join(ROOT, "docs", "KERNELS.md")).read() and "klatt_stage_frames.h" in open(os.path.join(ROOT, "README.md")).read()
    assert "lpcStage" in open(os.path.join(ROOT, "README.md")).read() and "klatt_stage_frames.h" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "stage_frames.txt"))


def brute(N, before, after, hop, phase):
    centres = range(phase, N + before + after + 2, hop)
    return sum(1 for c in centres if c + after <= N - 1), sum(1 for c in centres if c < N)


@pytest.mark.parametrize("nWin", [33, 64])
def test_lpc_emitted_is_the_brute_force_count(nWin):
    """For N = 0 .. 3 nWin + hop consumed samples: open, the j with c_j + after <= N - 1; ended, the j with c_j < N, the statement's count.
    nWin 33 splits (16, 16), nWin 64 (32, 31): the split is asymmetric only when the frame's length is even."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd.speechPlayer import _step_counts
    before, after = nWin // 2, nWin - 1 - nWin // 2
    assert (before, after) == ((16, 16) if nWin == 33 else (32, 31)) == sf.lpc_frame((4, nWin))
    for hop in (1, 7, nWin, nWin + 44):
        for phase in sorted({0, 5, hop - 1, nWin + 3}):
            for N in range(3 * nWin + hop + 1):
                opened, ended = brute(N, before, after, hop, phase)
                assert eng.lpcEmitted(N, nWin, hop, phase) == opened, (hop, phase, N, "open")
                assert eng.lpcEmitted(N, nWin, hop, phase, ended=True) == ended == int(_step_counts(N, hop, phase)), (hop, phase, N, "ended")


@pytest.mark.parametrize("lagMax", [65, 64])
def test_pitch_emitted_is_the_brute_force_count(lagMax):
    """The same with the frame of Nf = W + lagMax samples, W 32: Nf 97 splits (48, 48), Nf 96 (48, 47)."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd.speechPlayer import _step_counts
    W, Nf = 32, 32 + lagMax
    before, after = Nf // 2, Nf - 1 - Nf // 2
    assert (before, after) == ((48, 48) if lagMax == 65 else (48, 47)) == sf.pitch_frame((W, 2, lagMax))
    for hop in (1, 7, Nf, Nf + 44):
        for phase in sorted({0, 5, hop - 1, Nf + 3}):
            for N in range(3 * Nf + hop + 1):
                opened, ended = brute(N, before, after, hop, phase)
                assert eng.pitchEmitted(N, W, lagMax, hop, phase) == opened, (hop, phase, N, "open")
                assert eng.pitchEmitted(N, W, lagMax, hop, phase, ended=True) == ended == int(_step_counts(N, hop, phase)), (hop, phase, N, "ended")


def test_the_host_model_of_both_kinds_under_sanitizers(tmp_path):
    """tests/native/check_stage_frames.cpp: stage_row_plan, stage_sample and stage_history_from_chunk with the two geometries over edge and
    random chunkings, ends and resets -- every emitted step's frame, read through the virtual row, is the frame of the concatenated stream,
    and lpc_frame_host / pitch_frame_host on it equal lpc_host / pitch_host of the whole stream bit for bit -- under AddressSanitizer +
    UBSan, every chunk in an allocation of exactly its size.  Nothing loaded into python is run under a sanitizer."""
    exe = str(tmp_path / "check_stage_frames")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "native", "check_stage_frames.cpp"), "-o", exe])
    out = subprocess.check_output([exe], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out


def test_every_refusal_of_check_stage_request_for_the_two_kinds():
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    check = sp.check_stage_request
    kind, n, plan = check("lpc", 3, 16, 512, 160, 0, None, sp.lagWindow(16, 16000.0), ("lpc", "error"))
    assert (kind, n) == (5, 3) and plan[:4] == (16, 512, 160, 0) and plan[4] is None and len(plan[5]) == 17 and plan[6:] == (10, 17, 1)
    kind, n, plan = check("pitch", 4, 16000, nWin=160, lagMin=44, lagMax=300, fields=("f0", "voiced", "period"))
    assert (kind, n) == (6, 4) and plan[:4] == (16000, 160, 44, 300) and plan[5:] == (256, 0, 19, 3, 1)
    assert check("pitch", 1, 22050)[2][2:4] == (44, 368)
    with pytest.raises(KeyError, match="yin"):
        check("yin", 1, 16000)
    for kind, maker, args in (("lpc", "lpcStage", ()), ("pitch", "pitchStage", (16000,))):
        for bad in (0, -1, (1 << 20) + 1):
            with pytest.raises(ValueError, match=maker + ": nRows"):
                check(kind, bad, *args)
        for bad in (1.0, True, "3", None):
            with pytest.raises(TypeError, match=maker + ": nRows"):
                check(kind, bad, *args)
    # LPC's arguments: check_lpc_request's refusals, under the maker's name
    for kw, error, word in ((dict(order=0), ValueError, "order"), (dict(order=33), ValueError, "order"), (dict(order=2.0), ValueError, "order"), (dict(nWin=16), ValueError, "nWin"),
                            (dict(nWin=4097), ValueError, "nWin"), (dict(hop=0), ValueError, "hop"), (dict(hop=2.5), ValueError, "hop must be an integer"),
                            (dict(phase=-1), ValueError, "phase"), (dict(window=np.ones(511)), ValueError, "window needs 512"),
                            (dict(window=np.where(np.arange(512) == 3, np.inf, 1.0)), ValueError, "window value must be finite"),
                            (dict(lagWindow=np.ones(16)), ValueError, "lagWindow needs 17"), (dict(lagWindow=np.where(np.arange(17) == 3, np.nan, 1.0)), ValueError, "lagWindow value"),
                            (dict(fields=()), ValueError, "no fields"), (dict(fields=("lpc", "lsf")), KeyError, "lsf"), (dict(fields=32), ValueError, "fields 32")):
        with pytest.raises(error, match="lpcStage: .*" + word):
            check("lpc", 2, **kw)
    with pytest.raises(ValueError, match="lpcStage: .*histories.*2\\^27"):
        check("lpc", 1 << 20, nWin=4096)
    assert check("lpc", 1 << 20, nWin=129)[1] == 1 << 20      # 2^20 x 128 = 2^27
    with pytest.raises(ValueError, match="lpcStage: .*histories"):
        check("lpc", 1 << 20, nWin=130)
    # the pitch's: check_pitch_request's refusals
    for kw, error, word in ((dict(sampleRate=0), ValueError, "sampleRate"), (dict(sampleRate=16000.0), ValueError, "sampleRate"), (dict(lagMin=44), ValueError, "come together"),
                            (dict(lagMin=1, lagMax=100), ValueError, "lagMin and lagMax"), (dict(lagMin=100, lagMax=100), ValueError, "lagMin and lagMax"),
                            (dict(lagMin=2, lagMax=1025), ValueError, "lagMin and lagMax"), (dict(nWin=31), ValueError, "nWin"), (dict(nWin=2049), ValueError, "nWin"),
                            (dict(hop=0), ValueError, "hop"), (dict(phase=-1), ValueError, "phase"), (dict(threshold=1.5), ValueError, "threshold"),
                            (dict(threshold=float("nan")), ValueError, "threshold"), (dict(fields=()), ValueError, "no fields"), (dict(fields="pitch"), KeyError, "pitch"),
                            (dict(fields=64), ValueError, "fields 64"), (dict(fmin=500.0, fmax=60.0), ValueError, "fmin")):
        with pytest.raises(error, match=("pitchLags" if word == "fmin" else "pitchStage") + ".*" + word):
            check("pitch", 2, **{**dict(sampleRate=16000), **kw})
    with pytest.raises(ValueError, match="pitchStage: .*histories.*2\\^27"):
        check("pitch", 1 << 20, 16000, nWin=2048, lagMin=2, lagMax=1024)
    assert check("pitch", 1 << 20, 16000, nWin=64, lagMin=2, lagMax=65)[1] == 1 << 20      # 2^20 x 128 = 2^27
    # a push
    push = sp.check_stage_push
    x = torch.zeros((3, 8), dtype=torch.int16)
    for kind in sp.STAGE_FRAME_KINDS:
        assert push(kind, 3, (x, [8, 0, 3]), end=[True, False, True])[2:] == (1, False, True)
        assert push(kind, 3, (x, [8, 0, 3]), dtype=torch.float64)[2] == 0 and push(kind, 3, (x, [8, 0, 3]), dtype=torch.float32)[2] == 1
        with pytest.raises(TypeError, match="dtype"):
            push(kind, 3, (x, [8, 0, 3]), dtype=torch.int16)
        with pytest.raises(ValueError, match="code stage"):
            push(kind, 3, (x, [8, 0, 3]), codes=True)
        with pytest.raises(ValueError, match="code stage"):
            push(kind, 3, (x, [8, 0, 3]), decoded=False)
        with pytest.raises(ValueError, match="3 rows for a stage of 4"):
            push(kind, 4, (x, [8, 0, 3]))
        with pytest.raises(ValueError, match="end has 2"):
            push(kind, 3, (x, [8, 0, 3]), end=[True, False])
        with pytest.raises(TypeError, match="end must be"):
            push(kind, 3, (x, [8, 0, 3]), end=[1, 0, 1])
    with pytest.raises(KeyError, match="yin"):
        push("yin", 3, (x, [8, 0, 3]))


class FakeStage(object):
    """A SignalStage that records its pushes: SignalChain needs the kind, the row count, push and reset alone."""

    def __new__(cls, kind, nRows=2):
        from nvspeechplayer_amd import speechPlayer as sp
        self = object.__new__(sp.SignalStage)
        self.kind, self.nRows, self.log = kind, nRows, []
        self.push = lambda signal, end=None, **kw: self.log.append(("push", signal, end, kw)) or (kind, signal, end)
        self.reset = lambda rows=None: self.log.append(("reset", rows))
        self._h = None
        return self


def test_the_fan_at_the_end_of_a_chain():
    """SignalChain([.., (a, b, c)]): the pair arriving at the fan goes to each of its stages with the same end, the results come back as a
    tuple in order, no keyword reaches the fan, reset reaches every stage; an empty fan is a TypeError, a fan that is not last, a terminal
    stage before the end and unlike row counts are ValueErrors."""
    from nvspeechplayer_amd import speechPlayer as sp
    f, r, a, b, c = (FakeStage(k) for k in ("filter", "resample", "lpc", "pitch", "code"))
    chain = sp.SignalChain([f, r, (a, b, c)])
    assert chain.stages == [f, r, a, b, c] and chain.fan == [a, b, c]
    got = chain.push("x", end=True)
    mid = ("resample", ("filter", "x", True), True)
    assert got == (("lpc", mid, True), ("pitch", mid, True), ("code", mid, True))
    assert all(s.log == [("push", mid, True, {})] for s in (a, b, c)) and f.log == [("push", "x", True, {})]
    with pytest.raises(TypeError, match="defaults"):
        chain.push("x", dtype=None)
    chain.reset([True, False])
    assert all(s.log[-1] == ("reset", [True, False]) for s in (f, r, a, b, c))
    assert sp.SignalChain([[a, b]]).push("y") == (("lpc", "y", None), ("pitch", "y", None))      # a fan alone, as a list
    assert sp.SignalChain([f, a]).push("z", dtype="d") == ("lpc", ("filter", "z", None), None) and a.log[-1][3] == {"dtype": "d"}
    for bad in ([f, ()], [()], [f, []]):
        with pytest.raises(TypeError, match="fan"):
            sp.SignalChain(bad)
    with pytest.raises(TypeError, match="SignalStage"):
        sp.SignalChain([f, (a, "pitch")])
    with pytest.raises(ValueError, match="fan of stages comes last"):
        sp.SignalChain([f, (a, b), c])
    with pytest.raises(ValueError, match="rows"):
        sp.SignalChain([f, (a, FakeStage("pitch", 3))])
    for kind, word in (("lpc", "an lpc stage comes last"), ("pitch", "a pitch stage comes last"), ("code", "a code stage comes last"), ("spectrogram", "a spectrogram stage comes last")):
        with pytest.raises(ValueError, match=word):
            sp.SignalChain([FakeStage(kind), f])
        with pytest.raises(ValueError, match=word):
            sp.SignalChain([FakeStage(kind), (a, b)])


def test_the_refusals_of_the_c_entry_points_that_need_no_device():
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()

    def refused(got, word):
        assert got in (-1, None) and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and word in L.speechPlayer_lastError(), (got, word, L.speechPlayer_lastError())

    refused(L.speechPlayer_lpcEmitted(-1, 512, 160, 0, 0), b"lpcEmitted")
    refused(L.speechPlayer_lpcEmitted((1 << 44) + 1, 512, 160, 0, 0), b"2^44")
    for nWin in (0, 1, 4097):
        refused(L.speechPlayer_lpcEmitted(10, nWin, 160, 0, 0), b"nWin")
    refused(L.speechPlayer_lpcEmitted(10, 512, 0, 0, 1), b"hop")
    refused(L.speechPlayer_lpcEmitted(10, 512, 160, -1, 1), b"phase")
    assert L.speechPlayer_lpcEmitted(1 << 44, 64, 1, 0, 1) == 1 << 44 and L.speechPlayer_lastErrorCode() == 0
    assert L.speechPlayer_lpcEmitted(1 << 44, 64, 1, 0, 0) == (1 << 44) - 31 and L.speechPlayer_lpcEmitted(1 << 44, 33, 1, 0, 0) == (1 << 44) - 16
    assert L.speechPlayer_lpcEmitted(1 << 44, 4096, 1 << 50, 1 << 50, 1) == 0      # (a hop or phase beyond any row means the same as 2^45)
    refused(L.speechPlayer_pitchEmitted(-1, 1024, 368, 256, 0, 0), b"pitchEmitted")
    refused(L.speechPlayer_pitchEmitted((1 << 44) + 1, 1024, 368, 256, 0, 0), b"2^44")
    for nWin in (0, 31, 2049):
        refused(L.speechPlayer_pitchEmitted(10, nWin, 368, 256, 0, 0), b"nWin")
    for lagMax in (0, 2, 1025):
        refused(L.speechPlayer_pitchEmitted(10, 1024, lagMax, 256, 0, 0), b"lagMax")
    refused(L.speechPlayer_pitchEmitted(10, 1024, 368, 0, 0, 1), b"hop")
    refused(L.speechPlayer_pitchEmitted(10, 1024, 368, 256, -1, 1), b"phase")
    assert L.speechPlayer_pitchEmitted(1 << 44, 32, 64, 1, 0, 0) == (1 << 44) - 47 and L.speechPlayer_pitchEmitted(1 << 44, 32, 65, 1, 0, 1) == 1 << 44
    for bad in ((-1, 512, 160, 0), (10, 1, 160, 0), (10, 512, 0, 0), (10, 512, 160, -1)):
        with pytest.raises(ValueError, match="lpcEmitted"):
            eng.lpcEmitted(*bad)
    for bad in ((-1, 1024, 368, 256, 0), (10, 16, 368, 256, 0), (10, 1024, 2000, 256, 0), (10, 1024, 368, 0, 0)):
        with pytest.raises(ValueError, match="pitchEmitted"):
            eng.pitchEmitted(*bad)
    refused(L.speechPlayer_batch_stageLpc(None, 1, 16, 512, 256, 0, None, None, 10), b"stageLpc: no batch")
    refused(L.speechPlayer_batch_stagePitch(None, 1, 16000, 1024, 44, 368, 0.1, 256, 0, 9), b"stagePitch: no batch")
    # a push needs a stage, and a stage a device: deviceCodes on a frame kind is refused in tests/test_gpu_stage_frames.py; without a stage
    # the push is refused before it looks at anything else
    refused(L.speechPlayer_stage_push(None, None, None, None, 1, ctypes.c_void_p(16), 0, None, None), b"stage_push: no stage")


# ---- the inputs of tests/test_gpu_stage_frames.py ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("g", sf.LPC_GEOMETRY)
def test_the_lpc_inputs_run_every_stage_and_hold_a_silent_step(g, n):
    """On the host statement of every segment the GPU test compares: at least half of the steps run all `order` stages of the recursion (a
    test on inputs that stop early would compare zeros), and at least one step is silent -- 0 stages, its frame all +0."""
    import nvspeechplayer_amd as eng
    order, nWin, hop, phase = g[:4]
    stages = []
    for row in sf.streams(n, *sf.lpc_case(g, n)):
        for x in row:
            stages += list(eng.signalLpc(x, order, nWin, hop, phase, fields="stages")[:, 0])
    stages = np.array(stages)
    assert (stages == order).sum() * 2 >= len(stages) > 0 and (stages == 0).any(), (g, n, len(stages), int((stages == order).sum()), int((stages == 0).sum()))


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("g", sf.PITCH_GEOMETRY)
def test_the_pitch_inputs_hold_voiced_and_unvoiced_steps(g, n):
    """On the host statement of every segment the GPU test compares: voiced and unvoiced steps both occur, the voiced ones near the tone's
    period."""
    import nvspeechplayer_amd as eng
    W, lagMin, lagMax, hop, phase = g[:5]
    voiced, period = [], []
    for row in sf.streams(n, *sf.pitch_case(g, n)):
        for x in row:
            got = eng.signalPitch(x, sf.PITCH_RATE, nWin=W, hop=hop, phase=phase, threshold=sf.PITCH_THRESHOLD, fields=("period", "voiced"), lagMin=lagMin, lagMax=lagMax)
            period += list(got[:, 0])
            voiced += list(got[:, 1])
    voiced, period = np.array(voiced), np.array(period)
    assert (voiced == 1).sum() >= 1 and (voiced == 0).sum() >= 1, (g, n, len(voiced), int(voiced.sum()))
    near = np.abs(period[voiced == 1] - sf.pitch_period(g)) < 1.0
    assert near.sum() * 2 >= len(near), (g, n, period[voiced == 1])
