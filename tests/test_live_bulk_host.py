"""Bulk queueing and device-tensor I/O of LIVE handles, the parts that need no GPU: the four C entry points (include/speechPlayer_batch.h:
speechPlayer_queueFramesMany, speechPlayer_queueFramesManyDevice, speechPlayer_synthesizeManyExport, speechPlayer_handleDevice) are
declared, exported and bound, refuse invalid or NULL handles with SPEECHPLAYER_ERR_ARGUMENT and a message that names them, and the
argument checks of LiveGroup.queue / queueTensor / pullTensor (check_live_queue, check_pcm_out) refuse what they document."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["speechPlayer_queueFramesMany", "speechPlayer_queueFramesManyDevice", "speechPlayer_synthesizeManyExport", "speechPlayer_handleDevice"]
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
        assert getattr(lib, name).restype is ctypes.c_int, name


@pytest.mark.parametrize("handle", [None, 12345])
def test_invalid_handles_are_argument_errors(handle):
    """NULL and unknown handles: -1, SPEECHPLAYER_ERR_ARGUMENT and a message naming the function, before anything touches a device."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    handles = (ctypes.c_void_p * 1)(handle)
    fs = np.array([0, 2], np.int64)
    frames = np.zeros((2, 47))
    m = np.array([100, 100], np.uint32)
    produced = (ctypes.c_int * 1)()
    calls = {
        "speechPlayer_queueFramesMany": lambda: L.speechPlayer_queueFramesMany(handles, 1, fs.ctypes.data, frames.ctypes.data, m.ctypes.data,
                                                                               m.ctypes.data, None, None, None),
        "speechPlayer_queueFramesManyDevice": lambda: L.speechPlayer_queueFramesManyDevice(handles, 1, fs.ctypes.data, frames.ctypes.data,
                                                                                           m.ctypes.data, m.ctypes.data, None, None, None, None),
        "speechPlayer_synthesizeManyExport": lambda: L.speechPlayer_synthesizeManyExport(handles, 1, 64, None, 1, 0, None, produced),
        "speechPlayer_handleDevice": lambda: L.speechPlayer_handleDevice(handle),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert _native.last_error_code() == ERR_ARGUMENT, name
        assert name in _native.last_error(), (name, _native.last_error())


def test_bad_arrays_are_argument_errors():
    """What the C entries refuse about the arrays themselves, checked before the handles: a NULL handle array, a frameStart that does
    not start at 0 or decreases, a purge on a handle given no frames, an unknown export format, a row stride below the pull."""
    from nvspeechplayer_amd import _native
    L = _native.load()
    handles = (ctypes.c_void_p * 2)(None, None)
    m = np.full(4, 100, np.uint32)
    frames = np.zeros((4, 47))
    purge = np.array([0, 1], np.uint8)
    produced = (ctypes.c_int * 2)()
    for fs, pg, what in ((np.array([1, 2, 4], np.int64), None, "frameStart"), (np.array([0, 3, 2], np.int64), None, "frameStart"),
                         (np.array([0, 4, 4], np.int64), purge, "purge")):
        assert L.speechPlayer_queueFramesMany(handles, 2, fs.ctypes.data, frames.ctypes.data, m.ctypes.data, m.ctypes.data, None, None,
                                              None if pg is None else pg.ctypes.data) == -1
        assert _native.last_error_code() == ERR_ARGUMENT and what in _native.last_error(), _native.last_error()
    fs = np.array([0, 2, 4], np.int64)
    assert L.speechPlayer_queueFramesMany(None, 2, fs.ctypes.data, frames.ctypes.data, m.ctypes.data, m.ctypes.data, None, None, None) == -1
    assert _native.last_error_code() == ERR_ARGUMENT
    assert L.speechPlayer_queueFramesMany(handles, 0, None, None, None, None, None, None, None) == 0        # nothing to queue
    assert L.speechPlayer_synthesizeManyExport(handles, 2, 64, None, 2, 0, None, produced) == -1
    assert _native.last_error_code() == ERR_ARGUMENT and "format" in _native.last_error()
    assert L.speechPlayer_synthesizeManyExport(handles, 2, 64, None, 0, 63, None, produced) == -1
    assert _native.last_error_code() == ERR_ARGUMENT and "rowStride" in _native.last_error()


def good():
    fs = np.array([0, 2, 5], np.int64)
    return dict(frameStart=fs, minSamples=np.full(5, 100, np.uint32), fadeSamples=np.full(5, 10, np.uint32),
                userIndex=np.arange(5, dtype=np.int32), isNull=np.zeros(5, np.uint8), purge=np.array([1, 0], np.uint8))


@pytest.mark.parametrize("case", ["short_frame_start", "frame_start_not_from_0", "decreasing", "min_length", "fade_length",
                                  "index_length", "null_length", "purge_length", "purge_on_empty_row", "frames_rows", "frames_width"])
def test_live_queue_checks(case):
    """Each refusal of check_live_queue on its own (everything else about the arguments is right): ValueError."""
    from nvspeechplayer_amd.speechPlayer import check_live_queue
    a = good()
    frames = np.zeros((5, 47))
    if case == "short_frame_start":
        a["frameStart"] = np.array([0, 5], np.int64)
    elif case == "frame_start_not_from_0":
        a["frameStart"] = np.array([1, 2, 5], np.int64)
    elif case == "decreasing":
        a["frameStart"] = np.array([0, 6, 5], np.int64)
    elif case == "min_length":
        a["minSamples"] = a["minSamples"][:4]
    elif case == "fade_length":
        a["fadeSamples"] = np.append(a["fadeSamples"], 1)
    elif case == "index_length":
        a["userIndex"] = a["userIndex"][:3]
    elif case == "null_length":
        a["isNull"] = np.zeros(6, np.uint8)
    elif case == "purge_length":
        a["purge"] = np.zeros(3, np.uint8)
    elif case == "purge_on_empty_row":
        a["frameStart"] = np.array([0, 0, 5], np.int64)
    elif case == "frames_rows":
        frames = np.zeros((4, 47))
    elif case == "frames_width":
        frames = np.zeros((5, 46))
    with pytest.raises(ValueError):
        check_live_queue(2, a["frameStart"], a["minSamples"], a["fadeSamples"], a["userIndex"], a["isNull"], a["purge"], frames=frames)


def test_live_queue_checks_accept_and_convert():
    """Sequences and CPU tensors are accepted and come back as the C arrays; optional arrays stay None; frames come back [F, 47] float64."""
    import torch
    from nvspeechplayer_amd.speechPlayer import check_live_queue
    fs, m, f, ix, nu, pg, fr = check_live_queue(2, [0, 2, 5], [1, 2, 3, 4, 5], torch.tensor([5, 4, 3, 2, 1]), frames=[[0.5] * 47] * 5)
    assert fs.dtype == np.int64 and list(fs) == [0, 2, 5]
    assert m.dtype == np.uint32 and f.dtype == np.uint32 and list(f) == [5, 4, 3, 2, 1]
    assert ix is None and nu is None and pg is None
    assert fr.dtype == np.float64 and fr.shape == (5, 47) and fr.flags["C_CONTIGUOUS"]
    a = good()
    fs, m, f, ix, nu, pg, fr = check_live_queue(2, a["frameStart"], a["minSamples"], a["fadeSamples"], a["userIndex"], a["isNull"], a["purge"])
    assert ix.dtype == np.int32 and nu.dtype == np.uint8 and pg.dtype == np.uint8 and fr is None
    # a purge on a row that has frames, and empty rows without a purge, are fine
    check_live_queue(3, [0, 0, 3, 3], [1, 1, 1], [1, 1, 1], purge=[0, 1, 0])


@pytest.mark.parametrize("case,exc", [
    ("not_a_tensor", TypeError),
    ("float64", TypeError),
    ("int32", TypeError),
    ("one_dim", ValueError),
    ("rows", ValueError),
    ("narrow", ValueError),
    ("noncontiguous", ValueError),
    ("cpu", TypeError),
])
def test_pcm_out_checks(case, exc):
    """Each refusal of check_pcm_out on its own; the device comes last (on a GPU-less host a CPU tensor is all there is)."""
    import torch
    from nvspeechplayer_amd.speechPlayer import check_pcm_out
    out = torch.zeros((3, 100), dtype=torch.float32)
    if case == "not_a_tensor":
        out = np.zeros((3, 100), np.float32)
    elif case == "float64":
        out = out.double()
    elif case == "int32":
        out = out.int()
    elif case == "one_dim":
        out = torch.zeros(300, dtype=torch.int16)
    elif case == "rows":
        out = torch.zeros((4, 100), dtype=torch.int16)
    elif case == "narrow":
        out = torch.zeros((3, 99), dtype=torch.int16)
    elif case == "noncontiguous":
        out = torch.zeros((100, 3), dtype=torch.float32).t()
    with pytest.raises(exc):
        check_pcm_out(out, 3, 100, 0)
