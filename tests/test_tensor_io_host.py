"""Tensor I/O of a batch, the parts that need no GPU: the two C entry points (include/speechPlayer_batch.h:
speechPlayer_batch_setUtterancesDevice, speechPlayer_batch_exportPcm) are declared, exported and bound, refuse a NULL batch with
SPEECHPLAYER_ERR_ARGUMENT, and BatchPlayer.setUtterancesTensor's argument checks (check_frames_tensor) refuse what they document."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["speechPlayer_batch_setUtterancesDevice", "speechPlayer_batch_exportPcm", "speechPlayer_batch_device", "speechPlayer_batch_lengths"]
ERR_ARGUMENT = 1


def test_entry_points_are_declared_exported_and_bound():
    from nvspeechplayer_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read(), flags=re.S)
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _native.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name        # prototypes set by _native.load
    assert lib.speechPlayer_batch_exportPcm.restype is ctypes.c_longlong


def test_null_batch_is_an_argument_error():
    from nvspeechplayer_amd import _native
    lib = _native.load()
    fs = np.array([0, 1], np.int64)
    m = np.ones(1, np.uint32)
    rc = lib.speechPlayer_batch_setUtterancesDevice(None, 1, fs.ctypes.data, None, m.ctypes.data, m.ctypes.data, None, None, None, None)
    assert rc == -1 and _native.last_error_code() == ERR_ARGUMENT
    assert "setUtterancesDevice" in _native.last_error()
    sel = np.zeros(1, np.int64)
    for utterances in (None, sel.ctypes.data):
        rc = lib.speechPlayer_batch_exportPcm(None, utterances, 1, None, 1, 0, None)
        assert rc == -1 and _native.last_error_code() == ERR_ARGUMENT
        assert "exportPcm" in _native.last_error()
    assert lib.speechPlayer_batch_device(None) == -1 and _native.last_error_code() == ERR_ARGUMENT
    assert lib.speechPlayer_batch_lengths(None, None, 0) == -1 and _native.last_error_code() == ERR_ARGUMENT


def frames_ok(n=5):
    import torch
    return torch.zeros((n, 47), dtype=torch.float64)


@pytest.mark.parametrize("case,exc", [
    ("cpu", TypeError),
    ("float32", TypeError),
    ("shape46", ValueError),
    ("noncontiguous", ValueError),
    ("frame_start", ValueError),
    ("not_a_tensor", TypeError),
])
def test_frames_tensor_checks(case, exc):
    """Each refusal on its own: everything else about the arguments is right (on a GPU-less host a CPU tensor is the only kind there
    is, so the device comes last among the checks and the other refusals are reached first)."""
    import torch
    from nvspeechplayer_amd.speechPlayer import check_frames_tensor
    frames, fs = frames_ok(), np.array([0, 2, 5], np.int64)
    if case == "float32":
        frames = frames.float()
    elif case == "shape46":
        frames = torch.zeros((5, 46), dtype=torch.float64)
    elif case == "noncontiguous":
        frames = torch.zeros((47, 5), dtype=torch.float64).t()
        assert frames.shape == (5, 47)
    elif case == "frame_start":
        fs = np.array([0, 2, 4], np.int64)
    elif case == "not_a_tensor":
        frames = np.zeros((5, 47))
    with pytest.raises(exc):
        check_frames_tensor(frames, fs, 0)


def test_frames_tensor_checks_messages_and_frame_start_forms():
    import torch
    from nvspeechplayer_amd.speechPlayer import check_frames_tensor
    with pytest.raises(TypeError, match="CUDA"):
        check_frames_tensor(frames_ok(), [0, 5], 0)
    with pytest.raises(TypeError, match="float64"):
        check_frames_tensor(frames_ok().float(), [0, 5], 0)
    for bad in ([1, 5], [0, 3, 2, 5], [0, 6]):
        with pytest.raises(ValueError, match="frameStart"):
            check_frames_tensor(frames_ok(), bad, 0)
    with pytest.raises(ValueError, match="frameStart"):       # (a tensor frameStart is read like an array)
        check_frames_tensor(frames_ok(), torch.tensor([0, 4]), 0)
