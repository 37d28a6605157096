"""Host-side mirror of the reference's ctypes wrapper, over the MI355X engine.

`Frame` and `SpeechPlayer` keep the reference wrapper's names, arguments and
behaviour (reference speechPlayer.py:20-68): durations in milliseconds converted
with the same truncation, `synthesize` returning a ctypes short array carrying
`.length`, or None when nothing was produced.  `BatchPlayer` is the additive batch
interface (include/speechPlayer_batch.h): many frame streams, one kernel launch.

Everything here calls the HIP library through its C-ABI; there is no CPU path.
"""
import math
from ctypes import POINTER, Structure, byref, c_double, c_int, c_short, c_void_p, cast
from ctypes import c_longlong as ctypes_longlong

import numpy as np

from . import _native

speechPlayer_frameParam_t = c_double

FRAME_FIELDS = [
    'voicePitch',
    'vibratoPitchOffset',
    'vibratoSpeed',
    'voiceTurbulenceAmplitude',
    'glottalOpenQuotient',
    'voiceAmplitude',
    'aspirationAmplitude',
    'cf1', 'cf2', 'cf3', 'cf4', 'cf5', 'cf6', 'cfN0', 'cfNP',
    'cb1', 'cb2', 'cb3', 'cb4', 'cb5', 'cb6', 'cbN0', 'cbNP',
    'caNP',
    'fricationAmplitude',
    'pf1', 'pf2', 'pf3', 'pf4', 'pf5', 'pf6',
    'pb1', 'pb2', 'pb3', 'pb4', 'pb5', 'pb6',
    'pa1', 'pa2', 'pa3', 'pa4', 'pa5', 'pa6',
    'parallelBypass',
    'preFormantGain',
    'outputGain',
    'endVoicePitch',
]


class Frame(Structure):
    """47 doubles, field order = the C struct (include/speechPlayer.h; reference speechPlayer.py:20-40)."""
    _fields_ = [(name, speechPlayer_frameParam_t) for name in FRAME_FIELDS]

    def as_array(self):
        return np.frombuffer(bytes(self), dtype=np.float64).copy()

    @classmethod
    def from_array(cls, values):
        f = cls()
        for name, v in zip(FRAME_FIELDS, values):
            setattr(f, name, float(v))
        return f


class SpeechPlayer(object):
    """One live stream (reference speechPlayer.py:44-68)."""

    def __init__(self, sampleRate, noiseSeed=None):
        self.sampleRate = sampleRate
        self._dll = _native.load()
        self._speechHandle = self._dll.speechPlayer_initialize(sampleRate)
        if not self._speechHandle:
            raise RuntimeError("speechPlayer_initialize failed: %s" % _native.last_error())
        if noiseSeed is not None:
            self._dll.speechPlayer_setNoiseSeed(self._speechHandle, int(noiseSeed))

    def queueFrame(self, frame, minFrameDuration, fadeDuration, userIndex=-1, purgeQueue=False):
        frame = byref(frame) if frame else None
        self._dll.speechPlayer_queueFrame(self._speechHandle, frame,
                                          int(minFrameDuration * (self.sampleRate / 1000.0)),
                                          int(fadeDuration * (self.sampleRate / 1000.0)), userIndex, purgeQueue)

    def queueFrameSamples(self, frame, minSamples, fadeSamples, userIndex=-1, purgeQueue=False):
        """Same call with durations already in samples (the C-ABI unit)."""
        frame = byref(frame) if frame else None
        self._dll.speechPlayer_queueFrame(self._speechHandle, frame, int(minSamples), int(fadeSamples), userIndex, purgeQueue)

    def synthesize(self, numSamples):
        buf = (c_short * numSamples)()
        res = self._dll.speechPlayer_synthesize(self._speechHandle, numSamples, buf)
        if res > 0:
            buf.length = min(res, len(buf))
            return buf
        else:
            return None

    def getLastIndex(self):
        return self._dll.speechPlayer_getLastIndex(self._speechHandle)

    @staticmethod
    def synthesizeMany(players, numSamples, out=None):
        """Advance many live players together in one kernel launch (speechPlayer_synthesizeMany).
        Returns a list with what each player's synthesize(numSamples) would have returned.  With `out` (a C-contiguous int16
        array [len(players), >= numSamples]) the samples land in its rows instead and the return value is the array of
        per-player sample counts (no buffer is allocated per player and pull)."""
        n = len(players)
        if n == 0:
            return []
        dll = players[0]._dll
        handles = (c_void_p * n)(*[p._speechHandle for p in players])
        produced = (c_int * n)()
        if out is not None:
            if out.dtype != np.int16 or out.ndim != 2 or out.shape[0] < n or out.shape[1] < numSamples or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous int16 array [n, >= numSamples]")
            ptrs = (out.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(out.strides[0])).astype(np.uint64)
            rc = dll.speechPlayer_synthesizeMany(handles, n, numSamples, ptrs.ctypes.data, produced)
            if rc != 0:
                raise RuntimeError("speechPlayer_synthesizeMany failed: %s" % _native.last_error())
            return np.frombuffer(produced, dtype=np.int32).copy()
        bufs = [(c_short * numSamples)() for _ in range(n)]
        ptrs = (c_void_p * n)(*[cast(b, c_void_p) for b in bufs])
        rc = dll.speechPlayer_synthesizeMany(handles, n, numSamples, ptrs, produced)
        if rc != 0:
            raise RuntimeError("speechPlayer_synthesizeMany failed: %s" % _native.last_error())
        res = []
        for b, got in zip(bufs, produced):
            if got > 0:
                b.length = min(got, len(b))
                res.append(b)
            else:
                res.append(None)
        return res

    @staticmethod
    def synthesizeManyDevice(players, numSamples):
        """The same, PCM left in HBM (speechPlayer_synthesizeManyDevice): -> (device pointer, row stride in samples,
        produced[n]).  Row i holds produced[i] samples of players[i]."""
        n = len(players)
        dll = players[0]._dll
        handles = (c_void_p * n)(*[p._speechHandle for p in players])
        produced = (c_int * n)()
        ptr = c_void_p()
        stride = ctypes_longlong()
        rc = dll.speechPlayer_synthesizeManyDevice(handles, n, numSamples, byref(ptr), byref(stride), produced)
        if rc != 0:
            raise RuntimeError("speechPlayer_synthesizeManyDevice failed: %s" % _native.last_error())
        return ptr.value, stride.value, np.frombuffer(produced, dtype=np.int32).copy()

    def close(self):
        if getattr(self, "_speechHandle", None):
            self._dll.speechPlayer_terminate(self._speechHandle)
            self._speechHandle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LiveGroup(object):
    """A fixed set of live players pulled together again and again: the handle array and the result arrays are built once
    (SpeechPlayer.synthesizeMany builds them per call -- about a millisecond for 8192 players, as much as the engine's own host
    work per pull)."""

    def __init__(self, players):
        self.players = list(players)
        n = len(self.players)
        if n == 0:
            raise ValueError("no players")
        self._dll = self.players[0]._dll
        self._handles = (c_void_p * n)(*[p._speechHandle for p in self.players])
        self._produced = (c_int * n)()
        self.produced = np.frombuffer(self._produced, dtype=np.int32)      # a view: overwritten by the next pull
        self._ptr = c_void_p()
        self._stride = ctypes_longlong()
        self._out = None
        self._rows = None

    @property
    def device(self):
        """The HIP (= torch CUDA) device of the group's handles (speechPlayer_handleDevice)."""
        d = self._dll.speechPlayer_handleDevice(self._handles[0])
        if d < 0:
            raise RuntimeError("speechPlayer_handleDevice failed: %s" % _native.last_error())
        return d

    def queue(self, frameStart, frames, minSamples, fadeSamples, userIndex=None, isNull=None, purge=None):
        """Frames into every player in one call (speechPlayer_queueFramesMany): players[i] is given frames frameStart[i] ..
        frameStart[i+1]-1 in order, as that many queueFrameSamples calls (durations in samples), the first of them with purgeQueue when
        purge[i] is set; a frame whose isNull is set is never read.  frames [F, 47] and the other arguments are numpy arrays, sequences or
        CPU tensors (check_live_queue says what is refused)."""
        fs, m, f, ix, nu, pg, fr = check_live_queue(len(self.players), frameStart, minSamples, fadeSamples, userIndex, isNull, purge, frames=frames)
        p = lambda a: None if a is None else a.ctypes.data
        if self._dll.speechPlayer_queueFramesMany(self._handles, len(self.players), p(fs), p(fr), p(m), p(f), p(ix), p(nu), p(pg)) != 0:
            raise RuntimeError("speechPlayer_queueFramesMany failed: %s" % _native.last_error())

    def queueTensor(self, frameStart, frames, minSamples, fadeSamples, userIndex=None, isNull=None, purge=None):
        """queue with `frames` a contiguous torch.float64 CUDA tensor [F, 47] on the group's device (speechPlayer_queueFramesManyDevice);
        nothing is converted (check_frames_tensor, check_live_queue).  Ordered behind the work queued so far on torch's current stream, as
        BatchPlayer.setUtterancesTensor is: no host synchronisation of that stream.  The frames that fit in the players' rings are placed
        by a kernel; only the rows of frames beyond come to the host.  The tensor may be freed or overwritten once the call returns."""
        dev = self.device
        fs = check_frames_tensor(frames, frameStart, dev)
        fs, m, f, ix, nu, pg, _ = check_live_queue(len(self.players), fs, minSamples, fadeSamples, userIndex, isNull, purge)
        p = lambda a: None if a is None else a.ctypes.data
        rc = self._dll.speechPlayer_queueFramesManyDevice(self._handles, len(self.players), p(fs), frames.data_ptr() if fs[-1] else None,
                                                          p(m), p(f), p(ix), p(nu), p(pg), _ready_stream(self, dev))
        if rc != 0:
            raise RuntimeError("speechPlayer_queueFramesManyDevice failed: %s" % _native.last_error())

    def pullTensor(self, numSamples, dtype=None, out=None):
        """pull with the samples left on the device, in a tensor the caller owns (speechPlayer_synthesizeManyExport): -> (pcm, produced).
        pcm [n, numSamples] on the group's device, row i = players[i]'s samples, zero past produced[i]; dtype torch.float32 (default:
        sample / 32767, as BatchPlayer.pcmTensor) or torch.int16.  The pull itself is pull()'s (host-synchronous); the rows are written on
        torch's current stream behind it, with no host wait.  out: a contiguous int16 or float32 CUDA tensor [n, >= numSamples] to fill
        instead (its dtype counts; pcm is then out[:, :numSamples] and the columns beyond are zeros).  produced is a view, overwritten by
        the next pull."""
        import torch
        n = len(self.players)
        dev = self.device
        if out is None:
            dtype = torch.float32 if dtype is None else dtype
            if dtype not in (torch.float32, torch.int16):
                raise TypeError("pullTensor: dtype must be torch.float32 or torch.int16, not %s" % dtype)
            out = torch.empty((n, numSamples), dtype=dtype, device="cuda:%d" % dev)
        fmt = check_pcm_out(out, n, numSamples, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self._dll.speechPlayer_synthesizeManyExport(self._handles, n, numSamples, out.data_ptr() if out.numel() else None, fmt,
                                                         out.shape[1], stream, self._produced)
        if rc != 0:
            raise RuntimeError("speechPlayer_synthesizeManyExport failed: %s" % _native.last_error())
        return out[:, :numSamples], self.produced

    def pullDevice(self, numSamples):
        """-> (device pointer, row stride in samples, produced[n]); the PCM stays in HBM (speechPlayer_synthesizeManyDevice).  The pointer
        is the engine's pull buffer, valid until the next live call on the device (pullTensor: memory of the caller's)."""
        rc = self._dll.speechPlayer_synthesizeManyDevice(self._handles, len(self.players), numSamples, byref(self._ptr), byref(self._stride),
                                                         self._produced)
        if rc != 0:
            raise RuntimeError("speechPlayer_synthesizeManyDevice failed: %s" % _native.last_error())
        return self._ptr.value, self._stride.value, self.produced

    def pull(self, numSamples, out):
        """Samples into the rows of `out` (C-contiguous int16 [n, >= numSamples]); -> produced[n]."""
        n = len(self.players)
        if self._out is not out:
            if out.dtype != np.int16 or out.ndim != 2 or out.shape[0] < n or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous int16 array [n, >= numSamples]")
            self._rows = (out.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(out.strides[0])).astype(np.uint64)
            self._out = out
        if out.shape[1] < numSamples:
            raise ValueError("out has fewer than numSamples columns")
        rc = self._dll.speechPlayer_synthesizeMany(self._handles, n, numSamples, self._rows.ctypes.data, self._produced)
        if rc != 0:
            raise RuntimeError("speechPlayer_synthesizeMany failed: %s" % _native.last_error())
        return self.produced


def setGlobalOption(name, value):
    """speechPlayer_setGlobalOption (include/speechPlayer_batch.h): process-wide options of the live handles -- "live_mode" (arithmetic mode
    of handles created from now on), "live_alone" (up to how many handles of a pull get a wavefront each), "live_layout", "live_cus",
    "live_replicate", "live_trim"."""
    if _native.load().speechPlayer_setGlobalOption(name.encode() if isinstance(name, str) else name, int(value)) != 0:
        raise ValueError("speechPlayer_setGlobalOption(%r, %r) refused" % (name, value))


def pcm_digest(pcm):
    """speechPlayer_batch_digest's per-utterance value for a host int16 array (uint64 arithmetic wraps)."""
    v = np.asarray(pcm, dtype=np.int16).view(np.uint16).astype(np.uint64)
    pos = np.arange(len(v), dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (pos + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) ^ (v + np.uint64(1)) * np.uint64(0xC2B2AE3D27D4EB4F)
        x ^= x >> np.uint64(29); x *= np.uint64(0xBF58476D1CE4E5B9); x ^= x >> np.uint64(32)
        return int(x.sum(dtype=np.uint64))


class _HostBlock(object):
    """Owner of one speechPlayer_hostAlloc block: frees it when the last array view is gone."""
    def __init__(self, dll, nbytes):
        self._dll, self.ptr = dll, dll.speechPlayer_hostAlloc(nbytes)
        if not self.ptr:
            raise MemoryError("speechPlayer_hostAlloc(%d): %s" % (nbytes, _native.last_error()))

    def __del__(self):
        try:
            if self.ptr:
                self._dll.speechPlayer_hostFree(self.ptr)
                self.ptr = None
        except Exception:
            pass


def host_array(shape, dtype):
    """A numpy array in page-locked host memory (speechPlayer_hostAlloc): frames handed to setUtterances from such an array, and PCM
    read into one (readAll / readAllAsync), cross the link as one DMA at its full rate.  Freed with the array."""
    import ctypes
    dt = np.dtype(dtype)
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(x) for x in shape)
    n = int(np.prod(shape)) if len(shape) else 1
    block = _HostBlock(_native.load(), max(n * dt.itemsize, 1))
    raw = (ctypes.c_char * max(n * dt.itemsize, 1)).from_address(block.ptr)
    raw._block = block      # the array's base is `raw`: the block lives as long as any view of the array
    return np.frombuffer(raw, dtype=dt, count=n).reshape(shape)


def _as_array(a):
    """A numpy array of `a` (numpy, sequence or torch tensor; a CUDA tensor is copied to the host, which synchronises), of whatever dtype
    it has."""
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)


def _host_array(a, dtype):
    """_as_array, contiguous and of `dtype`."""
    return np.ascontiguousarray(_as_array(a), dtype=dtype)


def _answer(got, expected=None, error=RuntimeError):
    """The answer of a host statement of the library: a negative one raises `error` with the library's message; any other is the count
    `expected` (None: whatever it is)."""
    if got < 0:
        raise error(_native.last_error())
    assert expected is None or got == expected, (got, expected)
    return got


def _row_statement(what, s, inFormat, args, shape, dtype, counted=True):
    """The host statement speechPlayer_<what> about one row of samples `s` (inFormat None: int16 PCM, a pcm* statement; else a signal*
    one, which takes the format after the pointer): -> its output, a zeroed array of `shape` and `dtype` handed over after `args`,
    followed by its size where the statement takes it (`counted`).  A row or an output of nothing is a null pointer."""
    out = np.zeros(shape, dtype)
    lead = (s.ctypes.data if len(s) else None,) + (() if inFormat is None else (inFormat,))
    fn = getattr(_native.load(), "speechPlayer_" + what)
    _answer(fn(*lead, len(s), *args, out.ctypes.data if out.size else None, *((out.size,) if counted else ())), out.size)
    return out


def _pcm_samples(pcm, what):
    s = np.ascontiguousarray(np.asarray(pcm))
    if s.dtype != np.int16 or s.ndim != 1:
        raise TypeError("%s: pcm must be a one-dimensional int16 array, not %s %s" % (what, s.dtype, list(s.shape)))
    return s


def _step_counts(lens, hop, phase):
    """The steps phase + j * hop below each of the lengths `lens` (one length: a number): int64."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens > phase, (lens - phase + hop - 1) // hop, 0).astype(np.int64)


def check_frames_tensor(frames, frameStart, device):
    """The argument checks of BatchPlayer.setUtterancesTensor, before any library call: `frames` must be a contiguous torch.float64
    tensor [F, 47] with F = frameStart[-1], on CUDA device `device`.  Nothing is converted.  Raises TypeError (not a tensor, another
    dtype, not a CUDA tensor) or ValueError (shape, layout, frameStart, another device).  Returns frameStart as an int64 array."""
    import torch
    if not isinstance(frames, torch.Tensor):
        raise TypeError("frames must be a torch tensor, not %s" % type(frames).__name__)
    if frames.dtype != torch.float64:
        raise TypeError("frames must be torch.float64 (the frame's 47 doubles), not %s" % frames.dtype)
    if frames.dim() != 2 or frames.shape[1] != 47:
        raise ValueError("frames must have the shape [F, 47], not %s" % list(frames.shape))
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous")
    fs = _host_array(frameStart, np.int64)
    if fs.ndim != 1 or len(fs) < 1 or fs[0] != 0 or fs[-1] != frames.shape[0] or (np.diff(fs) < 0).any():
        raise ValueError("frameStart must run from 0 to F = %d without decreasing" % frames.shape[0])
    if not frames.is_cuda:
        raise TypeError("frames must be a CUDA tensor (device memory), not a %s tensor" % frames.device.type)
    if frames.device.index != device:
        raise ValueError("frames are on cuda:%d, the batch on cuda:%d" % (frames.device.index, device))
    return fs


def check_live_queue(n, frameStart, minSamples, fadeSamples, userIndex=None, isNull=None, purge=None, frames=None):
    """The argument checks of LiveGroup.queue / queueTensor that need no GPU, before any library call: frameStart has n + 1 entries and
    runs from 0 without decreasing (F = frameStart[-1] frames); minSamples and fadeSamples have F entries, userIndex and isNull F (or are
    None), purge n (or is None) and is set only on rows that have frames; `frames` (host frames; None: not checked here) is [F, 47].
    Raises ValueError.  Returns the C arrays (frameStart int64, min uint32, fade uint32, userIndex int32, isNull uint8, purge uint8,
    frames float64 [F, 47]; None for what was None)."""
    fs = _host_array(frameStart, np.int64).reshape(-1)
    if len(fs) != n + 1 or fs[0] != 0 or (np.diff(fs) < 0).any():
        raise ValueError("frameStart must have %d entries and run from 0 without decreasing" % (n + 1))
    F = int(fs[-1])
    m = _host_array(minSamples, np.uint32).reshape(-1)
    f = _host_array(fadeSamples, np.uint32).reshape(-1)
    if len(m) != F or len(f) != F:
        raise ValueError("minSamples and fadeSamples need %d entries, not %d and %d" % (F, len(m), len(f)))
    ix = None if userIndex is None else _host_array(userIndex, np.int32).reshape(-1)
    nu = None if isNull is None else _host_array(isNull, np.uint8).reshape(-1)
    if (ix is not None and len(ix) != F) or (nu is not None and len(nu) != F):
        raise ValueError("userIndex and isNull need %d entries" % F)
    pg = None if purge is None else _host_array(purge, np.uint8).reshape(-1)
    if pg is not None:
        if len(pg) != n:
            raise ValueError("purge needs %d entries, not %d" % (n, len(pg)))
        empty = np.flatnonzero((pg != 0) & (fs[1:] == fs[:-1]))
        if len(empty):
            raise ValueError("purge is set on row %d, which has no frames" % empty[0])
    fr = None
    if frames is not None:
        fr = _host_array(frames, np.float64)
        if fr.shape != (F, 47):
            raise ValueError("frames must have the shape [%d, 47], not %s" % (F, list(fr.shape)))
    return fs, m, f, ix, nu, pg, fr


def check_pcm_out(out, n, numSamples, device):
    """The argument checks of LiveGroup.pullTensor's `out`, before any library call: a contiguous torch.int16 or torch.float32 tensor
    [n, >= numSamples] on CUDA device `device`.  Raises TypeError (not a tensor, another dtype, not a CUDA tensor) or ValueError (shape,
    layout, another device).  Returns the export format (0 int16, 1 float32)."""
    import torch
    if not isinstance(out, torch.Tensor):
        raise TypeError("out must be a torch tensor, not %s" % type(out).__name__)
    if out.dtype not in (torch.int16, torch.float32):
        raise TypeError("out must be torch.int16 or torch.float32, not %s" % out.dtype)
    if out.dim() != 2 or out.shape[0] != n or out.shape[1] < numSamples:
        raise ValueError("out must have the shape [%d, >= %d], not %s" % (n, numSamples, list(out.shape)))
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")
    if not out.is_cuda:
        raise TypeError("out must be a CUDA tensor (device memory), not a %s tensor" % out.device.type)
    if out.device.index != device:
        raise ValueError("out is on cuda:%d, the players on cuda:%d" % (out.device.index, device))
    return 1 if out.dtype == torch.float32 else 0


TRACK_MARK, TRACK_FRAME = 47, 48      # SPEECHPLAYER_TRACK_MARK / _FRAME: the columns of trackTensor beyond the frame's 47 parameters
TRACK_COLUMNS = FRAME_FIELDS + ["mark", "frame"]


def _check_columns(what, columns, names, hint, noun="column"):
    """`columns` (a sequence of numbers or of names among `names`; a single one stands for one column) as an int32 array.  Raises KeyError
    (unknown name; `hint` lists the known ones) or ValueError (number out of range, no columns)."""
    if isinstance(columns, (str, int, np.integer)):
        columns = [columns]
    cols = []
    for c in columns:
        if isinstance(c, str):
            if c not in names:
                raise KeyError("%s: no %s named %r (%s)" % (what, noun, c, hint))
            c = names.index(c)
        c = int(c)
        if not 0 <= c < len(names):
            raise ValueError("%s: %s %d is not in 0 .. %d" % (what, noun, c, len(names) - 1))
        cols.append(c)
    if not cols:
        raise ValueError("%s: no %ss" % (what, noun))
    return np.asarray(cols, dtype=np.int32)


def _check_dtype(what, dtype, allowed, default):
    """dtype (None: `default`) one of the two `allowed` (TypeError): -> the export format, 1 for the 4-byte type, 0 for the 8-byte one."""
    import torch
    dtype = default if dtype is None else dtype
    if dtype not in allowed:
        raise TypeError("%s: dtype must be %s or %s, not %s" % (what, allowed[0], allowed[1], dtype))
    return 1 if dtype in (torch.float32, torch.int32) else 0


def _check_hop_phase_dtype(what, hop, phase, dtype, allowed, default):
    """hop >= 1 and phase >= 0 as ints (ValueError) and the dtype (_check_dtype): -> (hop, phase, the export format)."""
    hop, phase = int(hop), int(phase)
    if hop < 1:
        raise ValueError("%s: hop must be at least 1, not %d" % (what, hop))
    if phase < 0:
        raise ValueError("%s: phase must not be negative (%d)" % (what, phase))
    return hop, phase, _check_dtype(what, dtype, allowed, default)


def _float_types():
    import torch
    return (torch.float32, torch.float64), torch.float32


def check_track_request(columns, hop, phase, dtype):
    """The argument checks of BatchPlayer.trackTensor that need no GPU, before any library call: `columns` a non-empty sequence of
    column numbers 0 .. 48 or names (FRAME_FIELDS, "mark", "frame"; a single number or name stands for one column), hop >= 1,
    phase >= 0, dtype None / torch.float32 / torch.float64.  Raises KeyError (unknown name), ValueError (number, hop, phase, no columns)
    or TypeError (dtype).  Returns (columns as an int32 array, hop, phase, the export format: 0 float64, 1 float32)."""
    cols = _check_columns("trackTensor", columns, TRACK_COLUMNS, "FRAME_FIELDS, 'mark', 'frame'")
    return (cols,) + _check_hop_phase_dtype("trackTensor", hop, phase, dtype, *_float_types())


ALIGN_COLUMNS = ["phoneme", "stress", "flags", "unit", "textOffset", "frame", "position", "remaining"]      # SPEECHPLAYER_ALIGN_*
UNIT_COLUMNS = ["phoneme", "flags", "textOffset", "firstSample", "samples", "firstStep", "steps"]              # speechPlayer_batch_exportUnits


def check_alignment_request(columns, hop, phase, dtype):
    """The argument checks of BatchPlayer.alignmentTensor that need no GPU: `columns` a non-empty sequence of column numbers 0 .. 7 or
    names (ALIGN_COLUMNS; a single one stands for one column), hop >= 1, phase >= 0, dtype torch.int64 / torch.int32.  Raises KeyError,
    ValueError or TypeError as check_track_request does.  Returns (columns as an int32 array, hop, phase, the export format: 0 int64, 1 int32)."""
    import torch
    cols = _check_columns("alignmentTensor", columns, ALIGN_COLUMNS, ", ".join(ALIGN_COLUMNS))
    return (cols,) + _check_hop_phase_dtype("alignmentTensor", hop, phase, dtype, (torch.int64, torch.int32), torch.int64)


SOURCE_COLUMNS = ["f0", "phase", "vibratoPhase", "cycle", "open", "wave"]      # SPEECHPLAYER_SOURCE_*
EPOCH_COLUMNS = ["sample", "instant", "f0", "gain"]                             # speechPlayer_batch_exportEpochs


def check_source_request(columns, hop, phase, dtype):
    """The argument checks of BatchPlayer.sourceTensor that need no GPU: `columns` a non-empty sequence of column numbers 0 .. 5 or
    names (SOURCE_COLUMNS; a single one stands for one column), hop >= 1, phase >= 0, dtype None / torch.float32 / torch.float64.  Raises
    KeyError, ValueError or TypeError as check_track_request does.  Returns (columns as an int32 array, hop, phase, the export format:
    0 float64, 1 float32)."""
    cols = _check_columns("sourceTensor", columns, SOURCE_COLUMNS, ", ".join(SOURCE_COLUMNS))
    return (cols,) + _check_hop_phase_dtype("sourceTensor", hop, phase, dtype, *_float_types())


RESPONSE_KINDS = ["cascade_re", "cascade_im", "cascade_mag", "cascade_db",
                  "parallel_re", "parallel_im", "parallel_mag", "parallel_db"]      # SPEECHPLAYER_RESPONSE_*
RESPONSE_MAX_BINS = 4096


def check_response_request(frequencies, kinds, sampleRate, what="responseTensor"):
    """The argument checks of BatchPlayer.responseTensor and frameResponse that need no GPU: `frequencies` an int K (the K bins of
    linspace(0, sampleRate / 2, K)) or an array of 1 .. 4096 finite values in Hz; `kinds` a non-empty sequence of kind numbers 0 .. 7 or
    names (RESPONSE_KINDS; a single one stands for one kind).  Raises KeyError (unknown name) or ValueError.  Returns (frequencies as a
    float64 array, kinds as an int32 array)."""
    if isinstance(frequencies, (int, np.integer)) and not isinstance(frequencies, bool):
        if not 1 <= int(frequencies) <= RESPONSE_MAX_BINS:
            raise ValueError("%s: %d frequencies (1 .. %d)" % (what, int(frequencies), RESPONSE_MAX_BINS))
        freqs = np.linspace(0.0, sampleRate / 2.0, int(frequencies))
    else:
        freqs = np.ascontiguousarray(np.asarray(frequencies, dtype=np.float64).reshape(-1))
    if not 1 <= len(freqs) <= RESPONSE_MAX_BINS:
        raise ValueError("%s: %d frequencies (1 .. %d)" % (what, len(freqs), RESPONSE_MAX_BINS))
    if not np.all(np.isfinite(freqs)):
        raise ValueError("%s: every frequency must be finite" % what)
    return freqs, _check_columns(what, kinds, RESPONSE_KINDS, ", ".join(RESPONSE_KINDS), "kind")


def frameResponse(frames, sampleRate, frequencies, kinds=("cascade_db", "parallel_db"), gain=False):
    """The vocal-tract frequency response of plain frames on the host (speechPlayer_frameResponse; no GPU): frames [n, 47] (or one frame,
    or a Frame) -> float64 [n, len(kinds), K], by the definition in include/speechPlayer_batch.h -- the cascade and the parallel branch
    of the filter network each frame configures, at `frequencies` (an int K: linspace(0, sampleRate / 2, K); or Hz values).  kinds by
    number or name (RESPONSE_KINDS); gain: times preFormantGain * outputGain."""
    if isinstance(frames, Frame):
        frames = frames.as_array()
    fr = np.ascontiguousarray(np.asarray(frames, dtype=np.float64))
    if fr.ndim == 1:
        fr = fr.reshape(1, -1)
    if fr.ndim != 2 or fr.shape[1] != len(FRAME_FIELDS):
        raise ValueError("frameResponse: frames must be [n, %d], not %s" % (len(FRAME_FIELDS), list(fr.shape)))
    if int(sampleRate) <= 0:
        raise ValueError("frameResponse: sampleRate must be positive")
    freqs, ks = check_response_request(frequencies, kinds, int(sampleRate), "frameResponse")
    out = np.zeros((fr.shape[0], len(ks), len(freqs)), np.float64)
    _answer(_native.load().speechPlayer_frameResponse(fr.ctypes.data, fr.shape[0], int(sampleRate), freqs.ctypes.data, len(freqs), ks.ctypes.data, len(ks),
                                                      1 if gain else 0, out.ctypes.data), out.size)
    return out


STEM_COLUMNS = ["voice", "aspiration", "source", "frication", "cascade", "parallel", "output"]      # SPEECHPLAYER_STEM_*


def check_stem_request(columns, dtype):
    """The argument checks of BatchPlayer.stemTensor that need no GPU: `columns` a non-empty sequence of column numbers 0 .. 6 or names
    (STEM_COLUMNS; a single one stands for one column), dtype None / torch.float32 / torch.float64.  Raises KeyError, ValueError or
    TypeError as check_source_request does.  Returns (columns as an int32 array, the export format: 0 float64, 1 float32)."""
    cols = _check_columns("stemTensor", columns, STEM_COLUMNS, ", ".join(STEM_COLUMNS))
    return cols, _check_dtype("stemTensor", dtype, *_float_types())


def resonatorCoefficients(f, bw, sampleRate, anti=False):
    """The resonator coefficients (a, b, c) the synthesiser computes from frequencies `f` and bandwidths `bw` (Hz; scalars or arrays of
    one length) at sampleRate, on the host (speechPlayer_resonatorCoefficients; no GPU): -> float64 [n, 3].  anti: the anti-resonator's
    (inverted unless the frequency is 0).  Inside the range the header documents these are the device's bits."""
    fr = np.ascontiguousarray(np.atleast_1d(np.asarray(f, dtype=np.float64)).reshape(-1))
    bws = np.ascontiguousarray(np.atleast_1d(np.asarray(bw, dtype=np.float64)).reshape(-1))
    if len(fr) != len(bws):
        raise ValueError("resonatorCoefficients: %d frequencies and %d bandwidths" % (len(fr), len(bws)))
    if int(sampleRate) <= 0:
        raise ValueError("resonatorCoefficients: sampleRate must be positive")
    out = np.zeros((len(fr), 3), np.float64)
    _answer(_native.load().speechPlayer_resonatorCoefficients(fr.ctypes.data, bws.ctypes.data, len(fr), 1 if anti else 0, int(sampleRate), out.ctypes.data),
            len(fr))
    return out


SPECTROGRAM_FFT = (64, 4096)      # nFft: a power of two in this range


def check_spectrogram_request(nFft, hop, phase, window, bank, power, log, floor, dtype, what="spectrogramTensor"):
    """The argument checks of BatchPlayer.spectrogramTensor and pcmSpectrogram that need no GPU: nFft a power of two in 64 .. 4096,
    hop >= 1, phase >= 0, `window` None (periodic Hann) or nFft finite values, `bank` None (the bands are the bins) or finite
    [bands >= 1, nFft / 2 + 1], power 1 or 2, `log` None, "db" (10 log10 of a power, 20 log10 of a magnitude), "ln" or a finite
    number (the factor of log10; 0 means linear) with floor > 0 wherever there is a logarithm, dtype None / torch.float32 /
    torch.float64 (pcmSpectrogram passes torch.float64).  Raises ValueError or TypeError.  Returns (nFft, hop, phase, window as a
    float64 array or None, bank as a float64 [bands, nFft / 2 + 1] array or None, bands, power, logScale, floor, the export format:
    0 float64, 1 float32)."""
    if isinstance(nFft, bool) or not isinstance(nFft, (int, np.integer)):
        raise ValueError("%s: nFft must be an integer, not %r" % (what, nFft))
    nFft = int(nFft)
    if not SPECTROGRAM_FFT[0] <= nFft <= SPECTROGRAM_FFT[1] or nFft & (nFft - 1):
        raise ValueError("%s: nFft must be a power of two in %d .. %d, not %d" % ((what,) + SPECTROGRAM_FFT + (nFft,)))
    hop, phase, fmt = _check_hop_phase_dtype(what, hop, phase, dtype, *_float_types())
    if window is not None:
        window = np.ascontiguousarray(_host_array(window, np.float64).reshape(-1))
        if len(window) != nFft:
            raise ValueError("%s: the window needs %d values, not %d" % (what, nFft, len(window)))
        if not np.all(np.isfinite(window)):
            raise ValueError("%s: every window value must be finite" % what)
    bands = nFft // 2 + 1
    if bank is not None:
        bank = np.ascontiguousarray(_host_array(bank, np.float64))
        if bank.ndim != 2 or bank.shape[0] < 1 or bank.shape[1] != nFft // 2 + 1:
            raise ValueError("%s: the bank must be [bands >= 1, %d], not %s" % (what, nFft // 2 + 1, list(bank.shape)))
        if not np.all(np.isfinite(bank)):
            raise ValueError("%s: every bank value must be finite" % what)
        bands = bank.shape[0]
    if power not in (1, 2) or isinstance(power, bool):
        raise ValueError("%s: power must be 1 or 2, not %r" % (what, power))
    if log is None:
        scale = 0.0
    elif isinstance(log, str):
        if log not in ("db", "ln"):
            raise ValueError("%s: log must be None, 'db', 'ln' or a number, not %r" % (what, log))
        scale = math.log(10.0) if log == "ln" else (10.0 if power == 2 else 20.0)
    else:
        scale = float(log)
    floor = float(floor)
    if not math.isfinite(scale) or not math.isfinite(floor):
        raise ValueError("%s: log and floor must be finite (%r, %r)" % (what, log, floor))
    if scale != 0.0 and not floor > 0.0:
        raise ValueError("%s: a logarithm needs floor > 0, not %r" % (what, floor))
    return nFft, hop, phase, window, bank, bands, int(power), scale, floor, fmt


def pcmSpectrogram(pcm, nFft=1024, hop=256, phase=0, window=None, bank=None, power=2, log=None, floor=1e-10):
    """The STFT / band spectrogram of int16 PCM on the host (speechPlayer_pcmSpectrogram; no GPU): -> float64 [steps, bands], by the
    definition in include/speechPlayer_batch.h -- step j centred on sample phase + j * hop, zeros outside the signal, the float32
    transform the device runs.  Arguments as BatchPlayer.spectrogramTensor's."""
    return _spectrogram_statement("pcmSpectrogram", _pcm_samples(pcm, "pcmSpectrogram"), None, nFft, hop, phase, window, bank, power, log, floor)


def _spectrogram_statement(what, s, inFormat, nFft, hop, phase, window, bank, power, log, floor):
    import torch
    nFft, hop, phase, window, bank, bands, power, scale, floor, _ = check_spectrogram_request(nFft, hop, phase, window, bank, power, log, floor,
                                                                                             torch.float64, what)
    return _row_statement(what, s, inFormat, (nFft, hop, phase, _ptr(window), _ptr(bank), bands if bank is not None else 0, power, scale, floor),
                          (int(_step_counts(len(s), hop, phase)), bands), np.float64, counted=False)


def melFilterbank(sampleRate, nFft, nMels, fmin=0.0, fmax=None, norm=None):
    """A mel filterbank for spectrogramTensor / pcmSpectrogram (numpy, no GPU): float64 [nMels, nFft / 2 + 1].  HTK mel,
    2595 log10(1 + f / 700); triangles between nMels + 2 points equally spaced in mel from fmin to fmax (None: sampleRate / 2), each
    rising from 0 at one point to 1 at the next and falling to 0 at the one after, evaluated at the bin frequencies k sampleRate / nFft.
    norm: None, or "slaney": row m times 2 / (f[m + 2] - f[m]), f in Hz."""
    fmax = sampleRate / 2.0 if fmax is None else float(fmax)
    fmin = float(fmin)
    if int(nMels) < 1 or int(nFft) < 2 or not 0.0 <= fmin < fmax:
        raise ValueError("melFilterbank: nMels %r, nFft %r, fmin %r, fmax %r" % (nMels, nFft, fmin, fmax))
    if norm not in (None, "slaney"):
        raise ValueError("melFilterbank: norm must be None or 'slaney', not %r" % (norm,))
    mel = np.linspace(2595.0 * np.log10(1.0 + fmin / 700.0), 2595.0 * np.log10(1.0 + fmax / 700.0), int(nMels) + 2)
    f = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    bins = np.arange(int(nFft) // 2 + 1, dtype=np.float64) * (float(sampleRate) / int(nFft))
    up = (bins[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    down = (f[2:, None] - bins[None, :]) / (f[2:] - f[1:-1])[:, None]
    bank = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        bank = bank * (2.0 / (f[2:] - f[:-2]))[:, None]
    return bank


RESAMPLE_TILE = 1024             # kResampleTile of csrc/klatt_resample.h: consecutive outputs of one row a workgroup takes at a time
RESAMPLE_WINDOWS = ["hann", "kaiser"]
RESAMPLE_LIMITS = (4096, 1024, 1 << 20)      # up, taps, up * taps


def check_resample_request(srcRate, dstRate, zeros, rolloff, window, beta, dtype, what="resampledTensor"):
    """The argument checks of BatchPlayer.resampledTensor, pcmResample and resampleKernel that need no GPU, before any library call:
    both rates integers above 0, zeros an integer >= 1, rolloff finite in (0, 1], window "hann" / "kaiser" (or 0 / 1), the Kaiser beta
    (None: 8.6) finite and not negative, up <= 4096, taps <= 1024 and up * taps <= 2^20 for the ratio up / down the rates reduce to, dtype
    None / torch.float32 / np.float32 (float32) or torch.int16 / np.int16.  Raises ValueError or TypeError.  Returns (srcRate, dstRate,
    zeros, rolloff, the window's number, beta, the export format: 0 int16, 1 float32, up, down, taps)."""
    for name, v in (("srcRate", srcRate), ("dstRate", dstRate), ("zeros", zeros)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("%s: %s must be an integer, not %r" % (what, name, v))
    srcRate, dstRate, zeros = int(srcRate), int(dstRate), int(zeros)
    if srcRate <= 0 or dstRate <= 0 or srcRate >= 1 << 31 or dstRate >= 1 << 31:
        raise ValueError("%s: sample rates must be above 0 (and below 2^31), not %d and %d" % (what, srcRate, dstRate))
    if zeros < 1 or zeros >= 1 << 31:
        raise ValueError("%s: zeros must be at least 1, not %d" % (what, zeros))
    rolloff = float(rolloff)
    if not math.isfinite(rolloff) or not 0.0 < rolloff <= 1.0:
        raise ValueError("%s: rolloff must lie in (0, 1], not %r" % (what, rolloff))
    if isinstance(window, str):
        if window not in RESAMPLE_WINDOWS:
            raise ValueError("%s: window must be 'hann' or 'kaiser', not %r" % (what, window))
        win = RESAMPLE_WINDOWS.index(window)
    elif window in (0, 1) and not isinstance(window, bool):
        win = int(window)
    else:
        raise ValueError("%s: window must be 'hann' or 'kaiser', not %r" % (what, window))
    beta = 8.6 if beta is None else float(beta)
    if win == 1 and (not math.isfinite(beta) or beta < 0.0):
        raise ValueError("%s: the Kaiser beta must be finite and not negative, not %r" % (what, beta))
    if win == 0:
        beta = 0.0
    g = math.gcd(srcRate, dstRate)
    up, down = dstRate // g, srcRate // g
    if up > RESAMPLE_LIMITS[0]:
        raise ValueError("%s: %d to %d Hz is the ratio %d / %d: up must not be above %d" % (what, srcRate, dstRate, up, down, RESAMPLE_LIMITS[0]))
    wd = zeros / (rolloff * min(1.0, up / down))
    if not wd <= RESAMPLE_LIMITS[1] // 2:
        raise ValueError("%s: zeros %d at the ratio %d / %d takes more than %d taps" % (what, zeros, up, down, RESAMPLE_LIMITS[1]))
    taps = 2 * int(math.ceil(wd))
    if up * taps > RESAMPLE_LIMITS[2]:
        raise ValueError("%s: a table of %d phases of %d taps is above %d values" % (what, up, taps, RESAMPLE_LIMITS[2]))
    return srcRate, dstRate, zeros, rolloff, win, beta, _sample_format(dtype, what), up, down, taps


def resampledLength(length, srcRate, dstRate):
    """ceil(length * up / down) for the ratio the rates reduce to (speechPlayer_resampledLength; no GPU)."""
    return _answer(_native.load().speechPlayer_resampledLength(int(length), int(srcRate), int(dstRate)), error=ValueError)


def resampleKernel(srcRate, dstRate, zeros=6, rolloff=0.99, window="hann", beta=None):
    """The polyphase table of the resampler (speechPlayer_resampleKernel; no GPU): -> (table float64 [up, taps], up, down), the float32
    values both sides use, widened.  Row p, column k is the weight of input n0 + k - taps / 2 + 1 for an output of phase p, as
    include/speechPlayer_batch.h defines it.  Arguments as BatchPlayer.resampledTensor's."""
    srcRate, dstRate, zeros, rolloff, win, beta, _, up, down, taps = check_resample_request(srcRate, dstRate, zeros, rolloff, window, beta, None,
                                                                                           "resampleKernel")
    table = np.zeros((up, taps), np.float64)
    u, d, t = c_int(0), c_int(0), c_int(0)
    _answer(_native.load().speechPlayer_resampleKernel(srcRate, dstRate, zeros, rolloff, win, beta, byref(u), byref(d), byref(t), table.ctypes.data,
                                                       table.size), table.size)
    assert (u.value, d.value, t.value) == (up, down, taps), (u.value, d.value, t.value, up, down, taps)
    return table, up, down


def pcmResample(pcm, srcRate, dstRate, zeros=6, rolloff=0.99, window="hann", beta=None, dtype=np.float32):
    """int16 PCM at another sample rate on the host (speechPlayer_pcmResample; no GPU): -> float32 (sample / 32767 scale) or int16
    [ceil(len * up / down)], by the definition in include/speechPlayer_batch.h -- the float32 statement the device runs.  Arguments as
    BatchPlayer.resampledTensor's; dtype np.float32 or np.int16."""
    return _resample_statement("pcmResample", _pcm_samples(pcm, "pcmResample"), None, srcRate, dstRate, zeros, rolloff, window, beta, dtype)


def _resample_statement(what, s, inFormat, srcRate, dstRate, zeros, rolloff, window, beta, dtype):
    srcRate, dstRate, zeros, rolloff, win, beta, fmt, up, down, _ = check_resample_request(srcRate, dstRate, zeros, rolloff, window, beta, dtype, what)
    return _row_statement(what, s, inFormat, (srcRate, dstRate, zeros, rolloff, win, beta, fmt), (len(s) * up + down - 1) // down,
                          np.float32 if fmt else np.int16)


CONVOLVE_TILE = 1024             # kConvolveTile of csrc/klatt_convolve.h: consecutive outputs of one row a workgroup takes at a time
CONVOLVE_BLOCK = 1024            # kConvolveBlock: taps staged at a time
CONVOLVE_MAX_TAPS = 65536        # kConvolveMaxTaps: of one response
CONVOLVE_MAX_TABLE = 1 << 20     # kConvolveMaxTable: of all responses of a call


def check_convolve_request(irs, irOf, nRows, tail, dtype, what="convolvedTensor"):
    """The argument checks of BatchPlayer.convolvedTensor and pcmConvolve that need no GPU, before any library call: irs one
    one-dimensional array of real numbers or a list of them, each of 1 .. 65536 taps, at most 2^20 in all, every tap finite and at most
    2^32 in magnitude once rounded to float32; irOf None (exactly one response) or nRows integers in [0, len(irs)); tail a bool or 0 / 1;
    dtype None / torch.float32 / np.float32 (float32) or torch.int16 / np.int16.  Raises ValueError or TypeError.  Returns (the
    responses back to back: float32, their nIr + 1 starts: int64, irOf: int64 or None, tail: 0 or 1, the export format: 0 int16,
    1 float32)."""
    if isinstance(irs, np.ndarray) and irs.ndim == 1 and irs.dtype != object:
        irs = [irs]
    elif isinstance(irs, (list, tuple)) and len(irs) and all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in irs):
        irs = [irs]
    if not isinstance(irs, (list, tuple)):
        raise TypeError("%s: irs must be a one-dimensional array or a list of them, not %s" % (what, type(irs).__name__))
    if len(irs) < 1:
        raise ValueError("%s: at least one impulse response" % what)
    flat, start = [], [0]
    for j, h in enumerate(irs):
        try:
            a = _as_array(h)
        except Exception:
            raise TypeError("%s: response %d is not an array" % (what, j))
        if a.ndim != 1 or a.dtype.kind not in "fiu":
            raise TypeError("%s: response %d must be a one-dimensional array of real numbers, not %s %s" % (what, j, a.dtype, list(a.shape)))
        if not 1 <= len(a) <= CONVOLVE_MAX_TAPS:
            raise ValueError("%s: response %d has %d taps (1 .. %d)" % (what, j, len(a), CONVOLVE_MAX_TAPS))
        with np.errstate(over="ignore"):
            a = a.astype(np.float32)
        bad = np.flatnonzero(~(np.abs(a) <= np.float32(2.0 ** 32)))
        if len(bad):
            raise ValueError("%s: tap %d of response %d is %r (finite, at most 2^32 in magnitude)" % (what, bad[0], j, float(a[bad[0]])))
        flat.append(a)
        start.append(start[-1] + len(a))
        if start[-1] > CONVOLVE_MAX_TABLE:
            raise ValueError("%s: the responses have more than %d taps in all" % (what, CONVOLVE_MAX_TABLE))
    if irOf is None:
        if len(irs) != 1:
            raise ValueError("%s: irOf is needed with %d impulse responses" % (what, len(irs)))
        of = None
    else:
        of = _as_array(irOf)
        if of.dtype.kind not in "iu" or of.ndim != 1:
            raise TypeError("%s: irOf must be a one-dimensional array of integers, not %s %s" % (what, of.dtype, list(of.shape)))
        if len(of) != nRows:
            raise ValueError("%s: irOf has %d entries for %d rows" % (what, len(of), nRows))
        of = np.ascontiguousarray(of.astype(np.int64))
        if len(of) and (of.min() < 0 or of.max() >= len(irs)):
            raise ValueError("%s: irOf must lie in [0, %d)" % (what, len(irs)))
    if isinstance(tail, (bool, np.bool_)):
        tail = int(tail)
    elif not isinstance(tail, (int, np.integer)) or tail not in (0, 1):
        raise ValueError("%s: tail must be True or False (1 or 0), not %r" % (what, tail))
    return np.ascontiguousarray(np.concatenate(flat)), np.array(start, np.int64), of, int(tail), _sample_format(dtype, what)


def pcmConvolve(pcm, ir, tail=True, dtype=np.float32):
    """int16 PCM convolved with one impulse response on the host (speechPlayer_pcmConvolve; no GPU): -> float32 (sample / 32767 scale)
    or int16, len(pcm) + len(ir) - 1 values (tail) or len(pcm), by the definition in include/speechPlayer_batch.h -- the chain of float32
    fused multiply-adds the device runs, in ascending tap order."""
    return _convolve_statement("pcmConvolve", _pcm_samples(pcm, "pcmConvolve"), None, ir, tail, dtype)


def _convolve_statement(what, s, inFormat, ir, tail, dtype):
    h, start, _, tail, fmt = check_convolve_request(ir, None, 1, tail, dtype, what)
    return _row_statement(what, s, inFormat, (h.ctypes.data, len(h), tail, fmt), len(s) + len(h) - 1 if tail else len(s), np.float32 if fmt else np.int16)


FILTER_TILE = 64                 # kFilterTile of csrc/klatt_filter.h: consecutive samples of each of its 64 rows a wavefront takes at a time
FILTER_MAX_SECTIONS = 16         # kFilterMaxSections: of one filter
FILTER_MAX_TABLE = 1 << 16       # kFilterMaxTable: sections of all filters of a call
FILTER_MAX_TAIL = 1 << 20        # kFilterMaxTail: extra outputs of zero input
BIQUAD_KINDS = ["lowpass", "highpass", "bandpass", "notch", "peaking", "lowshelf", "highshelf"]


def _filter_sections(f, what, name):
    """One filter as float32 [K, 5] = b0 b1 b2 a1 a2: from [K, 5], or from scipy's sos layout [K, 6] = b0 b1 b2 a0 a1 a2, divided by a0
    in binary64 and rounded to float32 once."""
    try:
        a = _as_array(f)
    except Exception:
        raise TypeError("%s: %s is not an array" % (what, name))
    if a.ndim != 2 or a.shape[1] not in (5, 6) or a.dtype.kind not in "fiu":
        raise TypeError("%s: %s must be [K, 5] (b0 b1 b2 a1 a2) or [K, 6] (sos: b0 b1 b2 a0 a1 a2) real numbers, not %s %s" % (what, name, a.dtype, list(a.shape)))
    if not 1 <= a.shape[0] <= FILTER_MAX_SECTIONS:
        raise ValueError("%s: %s has %d sections (1 .. %d)" % (what, name, a.shape[0], FILTER_MAX_SECTIONS))
    if a.shape[1] == 6:
        a = a.astype(np.float64)
        if not np.all(np.isfinite(a[:, 3])) or np.any(a[:, 3] == 0):
            raise ValueError("%s: %s has a section whose a0 is not finite or is 0" % (what, name))
        with np.errstate(over="ignore", invalid="ignore"):
            a = a[:, [0, 1, 2, 4, 5]] / a[:, 3:4]
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a.astype(np.float32))


def check_filter_request(filters, filterOf, nRows, tail, dtype, what="filteredTensor"):
    """The argument checks of BatchPlayer.filteredTensor, pcmFilter and signalFilter that need no GPU, before any library call: filters
    one array of shape [K, 5] or [K, 6] (_filter_sections) or a list of them, each of 1 .. 16 sections, at most 2^16 in all; filterOf
    None (exactly one filter) or nRows integers in [0, len(filters)); tail an integer in 0 .. 2^20; dtype as convolvedTensor's.  The
    values -- finite coefficients, poles strictly inside the unit circle -- are the library's to refuse, with the filter and the section
    in its message.  Raises ValueError or TypeError.  Returns (the sections back to back: float32 [n, 5], their nFilters + 1 starts:
    int64, filterOf: int64 or None, tail, the export format: 0 int16, 1 float32)."""
    if not isinstance(filters, (list, tuple)):
        filters = [filters]
    elif len(filters) and all(isinstance(r, (list, tuple)) and len(r) and all(isinstance(v, (int, float, np.integer, np.floating)) for v in r) for r in filters):
        filters = [filters]      # (one filter given as nested lists of numbers)
    if len(filters) < 1:
        raise ValueError("%s: at least one filter" % what)
    flat, start = [], [0]
    for j, f in enumerate(filters):
        flat.append(_filter_sections(f, what, "filter %d" % j))
        start.append(start[-1] + len(flat[-1]))
        if start[-1] > FILTER_MAX_TABLE:
            raise ValueError("%s: the filters have more than %d sections in all" % (what, FILTER_MAX_TABLE))
    if filterOf is None:
        if len(filters) != 1:
            raise ValueError("%s: filterOf is needed with %d filters" % (what, len(filters)))
        of = None
    else:
        of = _as_array(filterOf)
        if of.dtype.kind not in "iu" or of.ndim != 1:
            raise TypeError("%s: filterOf must be a one-dimensional array of integers, not %s %s" % (what, of.dtype, list(of.shape)))
        if len(of) != nRows:
            raise ValueError("%s: filterOf has %d entries for %d rows" % (what, len(of), nRows))
        of = np.ascontiguousarray(of.astype(np.int64))
        if len(of) and (of.min() < 0 or of.max() >= len(filters)):
            raise ValueError("%s: filterOf must lie in [0, %d)" % (what, len(filters)))
    if isinstance(tail, (bool, np.bool_)) or not isinstance(tail, (int, np.integer)) or not 0 <= tail <= FILTER_MAX_TAIL:
        raise ValueError("%s: tail must be an integer in 0 .. %d, not %r" % (what, FILTER_MAX_TAIL, tail))
    return np.ascontiguousarray(np.concatenate(flat)), np.array(start, np.int64), of, int(tail), _sample_format(dtype, what)


def pcmFilter(pcm, sections, tail=0, dtype=np.float32):
    """int16 PCM through one cascade of biquad sections on the host (speechPlayer_pcmFilter; no GPU): sections [K, 5] = b0 b1 b2 a1 a2
    or scipy's sos layout [K, 6]; -> float32 (sample / 32767 scale) or int16, len(pcm) + tail values, by the definition in
    include/speechPlayer_batch.h -- transposed direct form II in float32, five correctly rounded operations per section and sample,
    the statement the device equals bit for bit."""
    return _filter_statement("pcmFilter", _pcm_samples(pcm, "pcmFilter"), None, sections, tail, dtype)


def _filter_statement(what, s, inFormat, sections, tail, dtype):
    sec, start, _, tail, fmt = check_filter_request(sections, None, 1, tail, dtype, what)
    return _row_statement(what, s, inFormat, (sec.ctypes.data, len(sec), tail, fmt), len(s) + tail, np.float32 if fmt else np.int16)


def biquad(kind, rate, f0, q=np.sqrt(0.5), gainDb=0.0):
    """One second-order section by the Audio-EQ-Cookbook (host numpy, binary64): kind one of BIQUAD_KINDS -- "lowpass", "highpass",
    "bandpass" (0 dB at f0), "notch", "peaking", "lowshelf", "highshelf" --, f0 in Hz below rate / 2, q the quality (shelves: the shelf
    slope's Q), gainDb for the last three.  -> float64 [1, 6] in scipy's sos layout with a0 = 1; stack sections with np.concatenate."""
    if kind not in BIQUAD_KINDS:
        raise KeyError("biquad: kind %r (%s)" % (kind, ", ".join(BIQUAD_KINDS)))
    rate, f0, q, gainDb = float(rate), float(f0), float(q), float(gainDb)
    if not (rate > 0 and 0 < f0 < rate / 2 and q > 0 and np.isfinite(gainDb)):
        raise ValueError("biquad: rate %r, f0 %r (0 .. rate / 2, exclusive), q %r (positive), gainDb %r" % (rate, f0, q, gainDb))
    w0 = 2.0 * np.pi * f0 / rate
    cs, alpha, A = np.cos(w0), np.sin(w0) / (2.0 * q), 10.0 ** (gainDb / 40.0)
    if kind == "lowpass":
        b, a = [(1 - cs) / 2, 1 - cs, (1 - cs) / 2], [1 + alpha, -2 * cs, 1 - alpha]
    elif kind == "highpass":
        b, a = [(1 + cs) / 2, -(1 + cs), (1 + cs) / 2], [1 + alpha, -2 * cs, 1 - alpha]
    elif kind == "bandpass":
        b, a = [alpha, 0.0, -alpha], [1 + alpha, -2 * cs, 1 - alpha]
    elif kind == "notch":
        b, a = [1.0, -2 * cs, 1.0], [1 + alpha, -2 * cs, 1 - alpha]
    elif kind == "peaking":
        b, a = [1 + alpha * A, -2 * cs, 1 - alpha * A], [1 + alpha / A, -2 * cs, 1 - alpha / A]
    else:
        sq = 2.0 * np.sqrt(A) * alpha
        if kind == "lowshelf":
            b = [A * ((A + 1) - (A - 1) * cs + sq), 2 * A * ((A - 1) - (A + 1) * cs), A * ((A + 1) - (A - 1) * cs - sq)]
            a = [(A + 1) + (A - 1) * cs + sq, -2 * ((A - 1) + (A + 1) * cs), (A + 1) + (A - 1) * cs - sq]
        else:
            b = [A * ((A + 1) + (A - 1) * cs + sq), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - sq)]
            a = [(A + 1) - (A - 1) * cs + sq, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - sq]
    b, a = np.array(b, np.float64), np.array(a, np.float64)
    return np.concatenate([b / a[0], [1.0], a[1:] / a[0]]).reshape(1, 6)


def preEmphasis(c=0.97):
    """y[n] = x[n] - c x[n-1] as one section: float64 [1, 6] (sos)."""
    return np.array([[1.0, -float(c), 0.0, 1.0, 0.0, 0.0]], np.float64)


def dcBlock(r=0.995):
    """The DC blocker y[n] = x[n] - x[n-1] + r y[n-1] as one section: float64 [1, 6] (sos)."""
    return np.array([[1.0, -1.0, 0.0, 1.0, -float(r), 0.0]], np.float64)


def resonatorSections(frequency, bandwidth, rate):
    """The synthesiser's resonators as sections (resonatorCoefficients: y = a x + b y1 + c y2, so b0 = a, a1 = -b, a2 = -c), one per
    (frequency, bandwidth) pair in Hz: float64 [K, 6] (sos)."""
    abc = resonatorCoefficients(frequency, bandwidth, rate)
    out = np.zeros((len(abc), 6), np.float64)
    out[:, 0], out[:, 3], out[:, 4], out[:, 5] = abc[:, 0], 1.0, -abc[:, 1], -abc[:, 2]
    return out


SIGNAL_MAX_LENGTH = 1 << 44      # kSignalMaxLength of csrc/klatt_tiles.h: samples of one row
# speechPlayer_signal_t (include/speechPlayer_batch.h)
_signalDtype = np.dtype([("data", np.uint64), ("format", np.int32), ("reserved", np.int32), ("nRows", np.int64), ("rowStride", np.int64),
                         ("extent", np.uint64)], align=True)
assert _signalDtype.itemsize == 40


def check_signal_request(signal, device=None, what="signal"):
    """The argument checks of the `signal=` of BatchPlayer.spectrogramTensor, resampledTensor and convolvedTensor that need no GPU:
    `signal` is the (tensor, second) pair the exports return -- a contiguous torch tensor of dtype torch.int16 or torch.float32, 2-D
    [n, width] with `second` the n row lengths (0 .. width each), or 1-D with `second` the n + 1 ascending offsets from 0 (the last at
    most the tensor's length) --, rows of at most 2^44 samples, and (device not None) on CUDA device `device`.  Raises ValueError or
    TypeError.  Returns (the tensor, its format: 0 int16 / 1 float32, n, rowStride: the width or 0, `second` as an int64 array, the n
    row lengths)."""
    import torch
    if not isinstance(signal, (tuple, list)) or len(signal) != 2:
        raise TypeError("%s: a signal is the (tensor, lengths or offsets) pair an export returns, not %s" % (what, type(signal).__name__))
    tensor, second = signal
    if not isinstance(tensor, torch.Tensor):
        raise TypeError("%s: the samples must be a torch tensor, not %s" % (what, type(tensor).__name__))
    if tensor.dtype not in (torch.int16, torch.float32):
        raise TypeError("%s: the samples must be torch.int16 or torch.float32, not %s" % (what, tensor.dtype))
    if tensor.dim() not in (1, 2):
        raise TypeError("%s: the samples must be [n, width] (padded) or one-dimensional (packed), not %s" % (what, list(tensor.shape)))
    if second is None or isinstance(second, str):
        raise TypeError("%s: the row lengths (padded) or offsets (packed) are missing" % what)
    try:
        ext = _as_array(second)
    except Exception:
        raise TypeError("%s: the row lengths or offsets are not an array" % what)
    if ext.size == 0:
        ext = ext.astype(np.int64)
    if ext.dtype.kind not in "iu":
        raise TypeError("%s: the row lengths or offsets must be integers, not %s" % (what, ext.dtype))
    if ext.ndim != 1:
        raise ValueError("%s: the row lengths or offsets must be one-dimensional, not %s" % (what, list(ext.shape)))
    ext = np.ascontiguousarray(ext.astype(np.int64))
    if not tensor.is_contiguous():
        raise ValueError("%s: the samples must be contiguous" % what)
    if tensor.dim() == 2:
        n, stride = int(tensor.shape[0]), int(tensor.shape[1])
        if len(ext) != n:
            raise ValueError("%s: %d row lengths for %d rows" % (what, len(ext), n))
        bad = np.flatnonzero((ext < 0) | (ext > stride))
        if len(bad):
            raise ValueError("%s: row %d has %d samples (0 .. the width, %d)" % (what, bad[0], ext[bad[0]], stride))
        lens = ext
        if stride == 0:      # rows of nothing: rowStride 0 would mean packed
            ext, stride = np.zeros(n + 1, np.int64), 0
    else:
        if len(ext) < 1:
            raise ValueError("%s: a packed signal comes with its n + 1 offsets" % what)
        n, stride = len(ext) - 1, 0
        if ext[0] != 0:
            raise ValueError("%s: row 0 of a packed signal starts at 0, not %d" % (what, ext[0]))
        lens = np.diff(ext)
        bad = np.flatnonzero(lens < 0)
        if len(bad):
            raise ValueError("%s: row %d ends (%d) before it starts (%d)" % (what, bad[0], ext[bad[0] + 1], ext[bad[0]]))
        if ext[-1] > tensor.shape[0]:
            raise ValueError("%s: the rows take %d samples, the tensor has %d" % (what, ext[-1], tensor.shape[0]))
    bad = np.flatnonzero(lens > SIGNAL_MAX_LENGTH)
    if len(bad):
        raise ValueError("%s: row %d has more than 2^44 samples" % (what, bad[0]))
    if device is not None and (not tensor.is_cuda or tensor.device.index != int(device)):
        raise ValueError("%s: the samples must be on the batch's device, cuda:%d, not %s" % (what, int(device), tensor.device))
    return tensor, 1 if tensor.dtype == torch.float32 else 0, n, stride, ext, np.ascontiguousarray(lens.astype(np.int64))


class RowSource(object):
    """What an export reads and the rows chosen from it, without a GPU: `count` rows called `noun`s ("utterance": the batch's PCM pool;
    "row": a signal) of `lengths` -- an array, or a function that gives one, called when the lengths are first asked for: the pool's
    cost a library call -- and `utterances`, indices in any order, repeats allowed (None: all, in order; ValueError for one outside
    [0, count), in the words of `what`).  sel: the choice as an int64 array, or None; n: the rows chosen; idx: their numbers; lengths:
    their lengths, int64.  lead and suffix: what an entry point over this source takes between the batch and the selection, and what
    its name ends in -- nothing over the pool; of_signal: the speechPlayer_signal_t record, and "Of"."""
    lead, suffix = (), ""

    def __init__(self, what, noun, count, lengths, utterances):
        self.count, self._lengths = count, lengths
        self.sel = None if utterances is None else _host_array(utterances, np.int64).reshape(-1)
        self.n = count if self.sel is None else len(self.sel)
        self.idx = np.arange(self.n) if self.sel is None else self.sel
        if self.n and (self.idx.min() < 0 or self.idx.max() >= count):
            raise ValueError("%s: %s numbers must lie in [0, %d)" % (what, noun, count))

    @property
    def lengths(self):
        lens = self._lengths() if callable(self._lengths) else self._lengths
        return lens[self.idx].astype(np.int64)

    @classmethod
    def of_signal(cls, what, signal, device, utterances):
        """The rows chosen from a signal= argument (check_signal_request; device None: wherever it is).  `record` is the
        speechPlayer_signal_t the entry point reads; it, the tensor and the extents it points to live as long as the source."""
        tensor, fmt, rows, stride, extent, lens = check_signal_request(signal, device, what)
        src = cls(what, "row", rows, lens, utterances)
        src.record = np.zeros(1, _signalDtype)
        src.record["data"], src.record["format"], src.record["nRows"], src.record["rowStride"], src.record["extent"] = (
            tensor.data_ptr(), fmt, rows, stride, extent.ctypes.data)
        src.held = (tensor, extent)
        src.lead, src.suffix = (src.record.ctypes.data,), "Of"
        return src


def _signal_samples(x, what):
    s = x if isinstance(x, np.ndarray) else None
    if s is None or s.ndim != 1 or s.dtype not in (np.int16, np.float32):
        raise TypeError("%s: the samples must be a one-dimensional int16 or float32 array, not %s" % (
            what, "%s %s" % (s.dtype, list(s.shape)) if s is not None else type(x).__name__))
    return np.ascontiguousarray(s), 1 if s.dtype == np.float32 else 0


def signalSpectrogram(x, nFft=1024, hop=256, phase=0, window=None, bank=None, power=2, log=None, floor=1e-10):
    """pcmSpectrogram on a signal's row (speechPlayer_signalSpectrogram; no GPU): x is a one-dimensional int16 array (pcmSpectrogram's
    bits) or a float32 one, taken as it is -- every sample finite and at most 2^16 in magnitude.  -> float64 [steps, bands]: the
    statement BatchPlayer.spectrogramTensor(signal=...) is held to."""
    return _spectrogram_statement("signalSpectrogram", *_signal_samples(x, "signalSpectrogram"), nFft, hop, phase, window, bank, power, log, floor)


def signalResample(x, srcRate, dstRate, zeros=6, rolloff=0.99, window="hann", beta=None, dtype=np.float32):
    """pcmResample on a signal's row (speechPlayer_signalResample; no GPU): x as signalSpectrogram's.  -> float32 or int16
    [ceil(len * up / down)]; equal rates give the samples themselves.  The statement BatchPlayer.resampledTensor(signal=...) is held to."""
    return _resample_statement("signalResample", *_signal_samples(x, "signalResample"), srcRate, dstRate, zeros, rolloff, window, beta, dtype)


def signalConvolve(x, ir, tail=True, dtype=np.float32):
    """pcmConvolve on a signal's row (speechPlayer_signalConvolve; no GPU): x as signalSpectrogram's.  -> float32 or int16, len(x) +
    len(ir) - 1 values (tail) or len(x).  The statement BatchPlayer.convolvedTensor(signal=...) is held to."""
    return _convolve_statement("signalConvolve", *_signal_samples(x, "signalConvolve"), ir, tail, dtype)


def signalFilter(x, sections, tail=0, dtype=np.float32):
    """pcmFilter on a signal's row (speechPlayer_signalFilter; no GPU): x as signalSpectrogram's.  -> float32 or int16, len(x) + tail
    values.  The statement BatchPlayer.filteredTensor(signal=...) is held to."""
    return _filter_statement("signalFilter", *_signal_samples(x, "signalFilter"), sections, tail, dtype)


CODECS = ["ulaw", "alaw", "adpcm"]      # the codec ids of include/speechPlayer_batch.h: G.711 mu-law, G.711 A-law, IMA/DVI ADPCM
CODE_TILE = 1024                 # kCodeTile of csrc/klatt_codec.h: consecutive samples of one row a workgroup of the G.711 kernel takes at a time


def _int16_format(dtype, what):
    """_sample_format with int16 for None: a codec's output is integer."""
    return _sample_format(np.int16 if dtype is None else dtype, what)


def check_codec_request(codec, codes, decoded, dtype, what="codedTensor"):
    """The argument checks of BatchPlayer.codedTensor, pcmCode and signalCode that need no GPU, before any library call: codec a name of
    CODECS or its number; codes and decoded bools, not both False; dtype None / torch.int16 / np.int16 (int16) or torch.float32 /
    np.float32.  Raises KeyError (the codec), ValueError or TypeError.  Returns (the codec's id, codes, decoded, the format of the decoded
    samples: 0 int16, 1 float32)."""
    if isinstance(codec, str):
        if codec not in CODECS:
            raise KeyError("%s: codec %r (%s)" % (what, codec, ", ".join(CODECS)))
        codec = CODECS.index(codec)
    elif isinstance(codec, (bool, np.bool_)) or not isinstance(codec, (int, np.integer)) or not 0 <= codec < len(CODECS):
        raise KeyError("%s: codec %r (%s, or 0 .. %d)" % (what, codec, ", ".join(CODECS), len(CODECS) - 1))
    for name, v in (("codes", codes), ("decoded", decoded)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("%s: %s must be True or False, not %r" % (what, name, v))
    if not codes and not decoded:
        raise ValueError("%s: codes, decoded or both" % what)
    return int(codec), bool(codes), bool(decoded), _int16_format(dtype, what)


def _code_statement(what, s, inFormat, codec, codes, decoded, dtype, state):
    codec, codes, decoded, fmt = check_codec_request(codec, codes, decoded, dtype, what)
    d = np.zeros(len(s), np.float32 if fmt else np.int16) if decoded else None
    c = np.zeros(len(s), np.uint8) if codes else None
    st = np.zeros(2, np.int32)
    lead = (s.ctypes.data if len(s) else None,) + (() if inFormat is None else (inFormat,))
    fn = getattr(_native.load(), "speechPlayer_" + what)
    _answer(fn(*lead, len(s), codec, fmt, _ptr(d) if len(s) else None, _ptr(c) if len(s) else None, len(s), st.ctypes.data), len(s))
    out = tuple(a for a in (d, c) if a is not None)
    out = out if len(out) > 1 else out[0]
    return (out, (int(st[0]), int(st[1]))) if state else out


def pcmCode(pcm, codec, codes=False, decoded=True, dtype=None, state=False):
    """int16 PCM through a codec on the host (speechPlayer_pcmCode; no GPU): codec "ulaw", "alaw" or "adpcm" (CODECS).  -> the decoded
    samples (int16, or dtype np.float32: sample / 32767), the codes (uint8, one per sample: 0 .. 255 for G.711, 0 .. 15 for ADPCM;
    codes[0::2] << 4 | codes[1::2] packs ADPCM nibbles in the usual byte order) or the pair (decoded, codes), by the definition in
    include/speechPlayer_batch.h -- the integer statement the device equals bit for bit.  state: -> (that, (val, idx)), the ADPCM
    encoder's state behind the last sample."""
    return _code_statement("pcmCode", _pcm_samples(pcm, "pcmCode"), None, codec, codes, decoded, dtype, state)


def signalCode(x, codec, codes=False, decoded=True, dtype=None, state=False):
    """pcmCode on a signal's row (speechPlayer_signalCode; no GPU): x as signalSpectrogram's, a float32 sample clipped and rounded to
    nearest even.  The statement BatchPlayer.codedTensor(signal=...) is held to."""
    return _code_statement("signalCode", *_signal_samples(x, "signalCode"), codec, codes, decoded, dtype, state)


def codecDecode(codes, codec, dtype=None, state=False):
    """The decoder alone on the host (speechPlayer_codecDecode; no GPU): codes a one-dimensional uint8 array, one code per sample -> int16
    (or dtype np.float32) samples; for "adpcm" the recursion driven by the codes, each 0 .. 15.  state as pcmCode's."""
    c = codes if isinstance(codes, np.ndarray) else None
    if c is None or c.ndim != 1 or c.dtype != np.uint8:
        raise TypeError("codecDecode: the codes must be a one-dimensional uint8 array, not %s" % (
            "%s %s" % (c.dtype, list(c.shape)) if c is not None else type(codes).__name__))
    c = np.ascontiguousarray(c)
    codec, _, _, fmt = check_codec_request(codec, True, True, dtype, "codecDecode")
    out = np.zeros(len(c), np.float32 if fmt else np.int16)
    st = np.zeros(2, np.int32)
    _answer(_native.load().speechPlayer_codecDecode(_ptr(c) if len(c) else None, len(c), codec, fmt, _ptr(out) if len(c) else None, len(c), st.ctypes.data), len(c))
    return (out, (int(st[0]), int(st[1]))) if state else out


def codecTable(codec):
    """The 256-entry int16 decode table of a G.711 law ("ulaw" or "alaw"): table[codes.long()] decodes on any device."""
    if check_codec_request(codec, True, True, None, "codecTable")[0] == CODECS.index("adpcm"):
        raise ValueError("codecTable: adpcm has no table (its decoder is a recursion: codecDecode)")
    return codecDecode(np.arange(256, dtype=np.uint8), codec)


LPC_FIELDS = ["autocorr", "lpc", "reflection", "error", "stages"]      # bit 1 << i of `what` (include/speechPlayer_batch.h); the fields come in this order
LPC_MAX_ORDER = 32               # kLpcMaxOrder of csrc/klatt_lpc.h
LPC_MAX_WIN = 4096               # kLpcMaxWin
LPC_TILE = 1024                  # kLpcTile: consecutive outputs of one row a workgroup of the residual kernel takes at a time
LPC_WHAT = ["residual", "prediction"]


def lpcColumns(fields, order):
    """Where each of `fields` (names of LPC_FIELDS, any order) lies in a step's values: -> ({name: (first column, count)}, the total)."""
    what = check_lpc_fields(fields, "lpcColumns")
    at, col = {}, 0
    for i, name in enumerate(LPC_FIELDS):
        if what >> i & 1:
            n = order + 1 if name == "autocorr" else order if name in ("lpc", "reflection") else 1
            at[name] = (col, n)
            col += n
    return at, col


def check_lpc_fields(fields, what="lpcTensor"):
    """fields: a name of LPC_FIELDS or a non-empty sequence of them (KeyError for another, ValueError for none), or the bit set itself,
    1 .. 31: -> the bit set."""
    if isinstance(fields, (int, np.integer)) and not isinstance(fields, (bool, np.bool_)):
        if not 1 <= int(fields) < 1 << len(LPC_FIELDS):
            raise ValueError("%s: fields %d (a set of the bits 1 .. %d)" % (what, fields, 1 << len(LPC_FIELDS) - 1))
        return int(fields)
    names = [fields] if isinstance(fields, str) else list(fields)
    bits = 0
    for name in names:
        if name not in LPC_FIELDS:
            raise KeyError("%s: field %r (%s)" % (what, name, ", ".join(LPC_FIELDS)))
        bits |= 1 << LPC_FIELDS.index(name)
    if not bits:
        raise ValueError("%s: no fields" % what)
    return bits


def _check_lpc_grid(hop, phase, what):
    """hop an integer >= 1 and phase an integer >= 0 (ValueError; a float is refused, not truncated: 2.5 is no hop): -> (hop, phase)."""
    for name, v, least in (("hop", hop, 1), ("phase", phase, 0)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < least:
            raise ValueError("%s: %s must be an integer >= %d, not %r" % (what, name, least, v))
    return int(hop), int(phase)


def _check_order(order, what):
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or not 1 <= order <= LPC_MAX_ORDER:
        raise ValueError("%s: order must be an integer in 1 .. %d, not %r" % (what, LPC_MAX_ORDER, order))
    return int(order)


def check_lpc_request(order, nWin, hop, phase, window, lagWindow, fields, dtype, what="lpcTensor"):
    """The argument checks of BatchPlayer.lpcTensor, pcmLpc and signalLpc that need no GPU: order in 1 .. 32, nWin an integer in
    order + 1 .. 4096, hop >= 1, phase >= 0, `window` None (periodic Hann) or nWin finite values, `lagWindow` None or order + 1 finite
    values, `fields` as check_lpc_fields', dtype None / torch.float32 / torch.float64.  Raises ValueError, KeyError or TypeError.
    Returns (order, nWin, hop, phase, window as a float64 array or None, lagWindow likewise, the bit set, the values per step, the
    export format: 0 float64, 1 float32)."""
    order = _check_order(order, what)
    if isinstance(nWin, (bool, np.bool_)) or not isinstance(nWin, (int, np.integer)) or not order < nWin <= LPC_MAX_WIN:
        raise ValueError("%s: nWin must be an integer in order + 1 = %d .. %d, not %r" % (what, order + 1, LPC_MAX_WIN, nWin))
    nWin = int(nWin)
    hop, phase = _check_lpc_grid(hop, phase, what)
    fmt = _check_dtype(what, dtype, *_float_types())
    arrays = []
    for name, a, n in (("window", window, nWin), ("lagWindow", lagWindow, order + 1)):
        if a is not None:
            a = np.ascontiguousarray(_host_array(a, np.float64).reshape(-1))
            if len(a) != n:
                raise ValueError("%s: the %s needs %d values, not %d" % (what, name, n, len(a)))
            if not np.all(np.isfinite(a)):
                raise ValueError("%s: every %s value must be finite" % (what, name))
        arrays.append(a)
    bits = check_lpc_fields(fields, what)
    return order, nWin, hop, phase, arrays[0], arrays[1], bits, lpcColumns(bits, order)[1], fmt


def _lpc_statement(what, s, inFormat, order, nWin, hop, phase, window, lagWindow, fields):
    import torch
    order, nWin, hop, phase, window, lagWindow, bits, cols, _ = check_lpc_request(order, nWin, hop, phase, window, lagWindow, fields, torch.float64, what)
    return _row_statement(what, s, inFormat, (order, nWin, hop, phase, _ptr(window), _ptr(lagWindow), bits),
                          (int(_step_counts(len(s), hop, phase)), cols), np.float64, counted=False)


def pcmLpc(pcm, order=16, nWin=512, hop=256, phase=0, window=None, lagWindow=None, fields=("lpc", "error")):
    """The linear-prediction analysis of int16 PCM on the host (speechPlayer_pcmLpc; no GPU): -> float64 [steps, values], by the
    definition in include/speechPlayer_batch.h -- step j centred on sample phase + j * hop, zeros outside the signal, the
    autocorrelation by exact binary64 products and one fixed tree, the Levinson-Durbin recursion in binary64.  Arguments as
    BatchPlayer.lpcTensor's; lpcColumns(fields, order) says where each field lies."""
    return _lpc_statement("pcmLpc", _pcm_samples(pcm, "pcmLpc"), None, order, nWin, hop, phase, window, lagWindow, fields)


def signalLpc(x, order=16, nWin=512, hop=256, phase=0, window=None, lagWindow=None, fields=("lpc", "error")):
    """pcmLpc on a signal's row (speechPlayer_signalLpc; no GPU): x as signalSpectrogram's.  The statement
    BatchPlayer.lpcTensor(signal=...) is held to."""
    return _lpc_statement("signalLpc", *_signal_samples(x, "signalLpc"), order, nWin, hop, phase, window, lagWindow, fields)


PITCH_FIELDS = ["f0", "period", "lag", "aperiodicity", "voiced", "cmnd"]      # bit 1 << i of `what` (include/speechPlayer_batch.h); the fields come in this order
PITCH_MIN_WIN = 32               # csrc/klatt_pitch.h
PITCH_MAX_WIN = 2048             # kPitchMaxWin
PITCH_MAX_LAG = 1024             # kPitchMaxLag
PITCH_GROUP = 16                 # kPitchGroup: consecutive steps of the output a workgroup of the kernel takes at a time


def pitchLags(sampleRate, fmin=60.0, fmax=500.0):
    """The lags that hold the periods of fmin .. fmax Hz at sampleRate: -> (floor(sampleRate / fmax), ceil(sampleRate / fmin)), clamped to
    2 <= lagMin < lagMax <= 1024 (22050 Hz, 60 .. 500 Hz: 44 .. 368)."""
    if not (sampleRate > 0 and 0 < fmin < fmax and math.isfinite(fmax)):
        raise ValueError("pitchLags: sampleRate %r, fmin %r, fmax %r (sampleRate > 0, 0 < fmin < fmax)" % (sampleRate, fmin, fmax))
    lagMin = max(2, min(int(math.floor(sampleRate / fmax)), PITCH_MAX_LAG - 1))
    lagMax = min(PITCH_MAX_LAG, max(int(min(math.ceil(sampleRate / fmin), PITCH_MAX_LAG)), lagMin + 1))
    return lagMin, lagMax


def check_pitch_fields(fields, what="pitchTensor"):
    """fields: a name of PITCH_FIELDS or a non-empty sequence of them (KeyError for another, ValueError for none), or the bit set itself,
    1 .. 63: -> the bit set."""
    if isinstance(fields, (int, np.integer)) and not isinstance(fields, (bool, np.bool_)):
        if not 1 <= int(fields) < 1 << len(PITCH_FIELDS):
            raise ValueError("%s: fields %d (a set of the bits 1 .. %d)" % (what, fields, 1 << len(PITCH_FIELDS) - 1))
        return int(fields)
    names = [fields] if isinstance(fields, str) else list(fields)
    bits = 0
    for name in names:
        if name not in PITCH_FIELDS:
            raise KeyError("%s: field %r (%s)" % (what, name, ", ".join(PITCH_FIELDS)))
        bits |= 1 << PITCH_FIELDS.index(name)
    if not bits:
        raise ValueError("%s: no fields" % what)
    return bits


def pitchColumns(fields, lagMin, lagMax):
    """Where each of `fields` (names of PITCH_FIELDS, any order) lies in a step's values: -> ({name: (first column, count)}, the total)."""
    what = check_pitch_fields(fields, "pitchColumns")
    at, col = {}, 0
    for i, name in enumerate(PITCH_FIELDS):
        if what >> i & 1:
            n = lagMax - lagMin + 1 if name == "cmnd" else 1
            at[name] = (col, n)
            col += n
    return at, col


def check_pitch_request(sampleRate, fmin, fmax, lagMin, lagMax, nWin, hop, phase, threshold, fields, dtype, what="pitchTensor"):
    """The argument checks of BatchPlayer.pitchTensor, pcmPitch and signalPitch that need no GPU: sampleRate an integer > 0; the lags from
    fmin and fmax (pitchLags) unless lagMin and lagMax are both given, integers with 2 <= lagMin < lagMax <= 1024; nWin an integer in
    32 .. 2048; hop >= 1; phase >= 0; threshold a finite number in [0, 1]; `fields` as check_pitch_fields'; dtype None / torch.float32 /
    torch.float64.  Raises ValueError, KeyError or TypeError.  Returns (sampleRate, nWin, lagMin, lagMax, threshold, hop, phase, the bit
    set, the values per step, the export format: 0 float64, 1 float32)."""
    def whole(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if not whole(sampleRate) or not 0 < sampleRate < 1 << 31:
        raise ValueError("%s: sampleRate must be an integer > 0, not %r" % (what, sampleRate))
    if (lagMin is None) != (lagMax is None):
        raise ValueError("%s: lagMin and lagMax come together (or neither: fmin and fmax give them)" % what)
    if lagMin is None:
        lagMin, lagMax = pitchLags(sampleRate, fmin, fmax)
    if not whole(lagMin) or not whole(lagMax) or not 2 <= lagMin < lagMax <= PITCH_MAX_LAG:
        raise ValueError("%s: lagMin and lagMax must be integers with 2 <= lagMin < lagMax <= %d, not %r and %r" % (what, PITCH_MAX_LAG, lagMin, lagMax))
    if not whole(nWin) or not PITCH_MIN_WIN <= nWin <= PITCH_MAX_WIN:
        raise ValueError("%s: nWin must be an integer in %d .. %d, not %r" % (what, PITCH_MIN_WIN, PITCH_MAX_WIN, nWin))
    hop, phase = _check_lpc_grid(hop, phase, what)
    if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0.0 <= threshold <= 1.0:
        raise ValueError("%s: threshold must be a number in 0 .. 1, not %r" % (what, threshold))
    fmt = _check_dtype(what, dtype, *_float_types())
    bits = check_pitch_fields(fields, what)
    return (int(sampleRate), int(nWin), int(lagMin), int(lagMax), float(threshold), hop, phase, bits, pitchColumns(bits, int(lagMin), int(lagMax))[1], fmt)


def _pitch_statement(what, s, inFormat, sampleRate, fmin, fmax, lagMin, lagMax, nWin, hop, phase, threshold, fields):
    import torch
    sampleRate, nWin, lagMin, lagMax, threshold, hop, phase, bits, cols, _ = check_pitch_request(sampleRate, fmin, fmax, lagMin, lagMax, nWin, hop, phase,
                                                                                                 threshold, fields, torch.float64, what)
    return _row_statement(what, s, inFormat, (sampleRate, nWin, lagMin, lagMax, threshold, hop, phase, bits),
                          (int(_step_counts(len(s), hop, phase)), cols), np.float64, counted=False)


def pcmPitch(pcm, sampleRate, fmin=60.0, fmax=500.0, nWin=1024, hop=256, phase=0, threshold=0.1, fields=("f0", "aperiodicity"), lagMin=None, lagMax=None):
    """The pitch of int16 PCM estimated from the signal on the host (speechPlayer_pcmPitch; no GPU): -> float64 [steps, values], by the
    definition in include/speechPlayer_batch.h -- step j centred on sample phase + j * hop, a frame of nWin + lagMax samples, zeros outside
    the signal, the YIN difference by exact binary64 squares in four chains, its cumulative mean normalised form, the first dip below the
    threshold and a parabolic refinement.  Arguments as BatchPlayer.pitchTensor's; pitchColumns(fields, lagMin, lagMax) says where each
    field lies."""
    return _pitch_statement("pcmPitch", _pcm_samples(pcm, "pcmPitch"), None, sampleRate, fmin, fmax, lagMin, lagMax, nWin, hop, phase, threshold, fields)


def signalPitch(x, sampleRate, fmin=60.0, fmax=500.0, nWin=1024, hop=256, phase=0, threshold=0.1, fields=("f0", "aperiodicity"), lagMin=None, lagMax=None):
    """pcmPitch on a signal's row (speechPlayer_signalPitch; no GPU): x as signalSpectrogram's.  The statement
    BatchPlayer.pitchTensor(signal=...) is held to."""
    return _pitch_statement("signalPitch", *_signal_samples(x, "signalPitch"), sampleRate, fmin, fmax, lagMin, lagMax, nWin, hop, phase, threshold, fields)


def lpcFromAutocorrelation(r):
    """The Levinson-Durbin recursion alone (speechPlayer_lpcFromAutocorrelation; no GPU) on r[0 .. order], order = len(r) - 1 in
    1 .. 32: -> (a float64 [order]: a_1 .., k float64 [order]: the reflection coefficients, the error E, the stages done).  It stops
    -- the later values +0 -- as soon as E is not positive and finite or a reflection coefficient is not below 1 in magnitude."""
    r = np.ascontiguousarray(_host_array(r, np.float64).reshape(-1))
    order = _check_order(len(r) - 1, "lpcFromAutocorrelation")
    a, k, e, st = np.zeros(order), np.zeros(order), np.zeros(1), np.zeros(1, np.int32)
    _answer(_native.load().speechPlayer_lpcFromAutocorrelation(r.ctypes.data, order, a.ctypes.data, k.ctypes.data, e.ctypes.data, st.ctypes.data), order)
    return a, k, float(e[0]), int(st[0])


def lagWindow(order, sampleRate, bandwidth=60.0, whiteNoise=2.0 ** -30):
    """A lag window for lpcTensor / pcmLpc (numpy, no GPU): float64 [order + 1], the Gaussian exp(-0.5 (2 pi bandwidth k / sampleRate)^2)
    with element 0 multiplied by 1 + whiteNoise (white-noise correction)."""
    order = _check_order(order, "lagWindow")
    if not sampleRate > 0 or not bandwidth >= 0 or not whiteNoise >= 0 or not all(math.isfinite(float(v)) for v in (sampleRate, bandwidth, whiteNoise)):
        raise ValueError("lagWindow: sampleRate > 0, bandwidth >= 0, whiteNoise >= 0, all finite (%r, %r, %r)" % (sampleRate, bandwidth, whiteNoise))
    w = np.exp(-0.5 * (2.0 * np.pi * float(bandwidth) * np.arange(order + 1, dtype=np.float64) / float(sampleRate)) ** 2)
    w[0] *= 1.0 + float(whiteNoise)
    return w


def check_lpc_residual_request(order, hop, phase, column, what_, dtype, what="lpcResidualTensor"):
    """The argument checks of BatchPlayer.lpcResidualTensor, pcmLpcResidual and signalLpcResidual that need no GPU: order in 1 .. 32,
    hop >= 1, phase >= 0, column >= 0 (where a_1 lies in a step's values), what_ "residual" / "prediction" or 0 / 1, dtype None /
    torch.float32 / np.float32 or torch.int16 / np.int16.  Raises ValueError, KeyError or TypeError.  Returns (order, hop, phase,
    column, 0 residual or 1 prediction, the format of the samples: 0 int16, 1 float32)."""
    order = _check_order(order, what)
    hop, phase = _check_lpc_grid(hop, phase, what)
    if isinstance(column, (bool, np.bool_)) or not isinstance(column, (int, np.integer)) or column < 0:
        raise ValueError("%s: column must be an integer >= 0, not %r" % (what, column))
    if isinstance(what_, str):
        if what_ not in LPC_WHAT:
            raise KeyError("%s: what %r (%s)" % (what, what_, ", ".join(LPC_WHAT)))
        what_ = LPC_WHAT.index(what_)
    elif isinstance(what_, (bool, np.bool_)) or not isinstance(what_, (int, np.integer)) or what_ not in (0, 1):
        raise KeyError("%s: what %r (%s, or 0 / 1)" % (what, what_, ", ".join(LPC_WHAT)))
    return order, hop, phase, int(column), int(what_), _sample_format(dtype, what)


def _lpc_residual_statement(name, s, inFormat, coeff, hop, phase, what, dtype):
    c = np.ascontiguousarray(_host_array(coeff, np.float64))
    if c.ndim != 2:
        raise ValueError("%s: the coefficients must be [steps, order], not %s" % (name, list(c.shape)))
    order, hop, phase, _, which, fmt = check_lpc_residual_request(c.shape[1], hop, phase, 0, what, dtype, name)
    steps = int(_step_counts(len(s), hop, phase))
    if c.shape[0] != steps:
        raise ValueError("%s: %d rows of coefficients for %d steps" % (name, c.shape[0], steps))
    return _row_statement(name, s, inFormat, (order, hop, phase, c.ctypes.data if steps else None, which, fmt), (len(s),), np.float32 if fmt else np.int16)


def pcmLpcResidual(pcm, coeff, hop=256, phase=0, what="residual", dtype=np.float32):
    """int16 PCM through the inverse filter of its frames' coefficients on the host (speechPlayer_pcmLpcResidual; no GPU): coeff float64
    [steps, order], a_1 .. a_order of every step of pcmLpc's grid for the same hop and phase; sample t takes the row of the nearest
    centre (ties upward).  -> float32 or int16 [len(pcm)]: the residual e(t) = x(t) + sum a_m x(t - m), or (what "prediction")
    p(t) = -sum a_m x(t - m), one binary64 fma chain per sample."""
    return _lpc_residual_statement("pcmLpcResidual", _pcm_samples(pcm, "pcmLpcResidual"), None, coeff, hop, phase, what, dtype)


def signalLpcResidual(x, coeff, hop=256, phase=0, what="residual", dtype=np.float32):
    """pcmLpcResidual on a signal's row (speechPlayer_signalLpcResidual; no GPU): x as signalSpectrogram's.  The statement
    BatchPlayer.lpcResidualTensor(signal=...) is held to."""
    return _lpc_residual_statement("signalLpcResidual", *_signal_samples(x, "signalLpcResidual"), coeff, hop, phase, what, dtype)


LPC_SYNTH_HISTORIES = (8, 16, 32)      # the register rings of csrc/klatt_lpcsynth.h: a request runs in the smallest that holds its order


def check_lpc_synthesis_request(order, hop, phase, column, dtype, what="lpcSynthesisTensor"):
    """The argument checks of BatchPlayer.lpcSynthesisTensor, pcmLpcSynthesis and signalLpcSynthesis that need no GPU: order in 1 .. 32,
    hop >= 1, phase >= 0, column >= 0 (where a_1 lies in a step's values), dtype None / torch.float32 / np.float32 or torch.int16 /
    np.int16.  Raises ValueError or TypeError.  Returns (order, hop, phase, column, the format of the samples: 0 int16, 1 float32)."""
    order = _check_order(order, what)
    hop, phase = _check_lpc_grid(hop, phase, what)
    if isinstance(column, (bool, np.bool_)) or not isinstance(column, (int, np.integer)) or column < 0:
        raise ValueError("%s: column must be an integer >= 0, not %r" % (what, column))
    return order, hop, phase, int(column), _sample_format(dtype, what)


def _lpc_synthesis_statement(name, s, inFormat, coeff, hop, phase, dtype):
    c = np.ascontiguousarray(_host_array(coeff, np.float64))
    if c.ndim != 2:
        raise ValueError("%s: the coefficients must be [steps, order], not %s" % (name, list(c.shape)))
    order, hop, phase, _, fmt = check_lpc_synthesis_request(c.shape[1], hop, phase, 0, dtype, name)
    steps = int(_step_counts(len(s), hop, phase))
    if c.shape[0] != steps:
        raise ValueError("%s: %d rows of coefficients for %d steps" % (name, c.shape[0], steps))
    return _row_statement(name, s, inFormat, (order, hop, phase, c.ctypes.data if steps else None, fmt), (len(s),), np.float32 if fmt else np.int16)


def pcmLpcSynthesis(pcm, coeff, hop=256, phase=0, dtype=np.float32):
    """int16 PCM, taken as an excitation, through the recursive filter 1 / A(z) of its frames' coefficients on the host
    (speechPlayer_pcmLpcSynthesis; no GPU): coeff float64 [steps, order] as pcmLpcResidual's; sample t takes the row of the nearest
    centre (ties upward).  -> float32 or int16 [len(pcm)]: y(t) = e(t) - sum a_m y(t - m), one binary64 fma chain per sample from
    y(t) = +0 for t < 0, the history the float32 y."""
    return _lpc_synthesis_statement("pcmLpcSynthesis", _pcm_samples(pcm, "pcmLpcSynthesis"), None, coeff, hop, phase, dtype)


def signalLpcSynthesis(x, coeff, hop=256, phase=0, dtype=np.float32):
    """pcmLpcSynthesis on a signal's row (speechPlayer_signalLpcSynthesis; no GPU): x as signalSpectrogram's.  The statement
    BatchPlayer.lpcSynthesisTensor(signal=...) is held to."""
    return _lpc_synthesis_statement("signalLpcSynthesis", *_signal_samples(x, "signalLpcSynthesis"), coeff, hop, phase, dtype)


def lpcFromReflection(k):
    """The step-up recursion (speechPlayer_lpcFromReflection; no GPU): the reflection coefficients k_1 .. k_order, order = len(k) in
    1 .. 32 -> a float64 [order]: a_1 .. a_order, bit for bit the `a` lpcFromAutocorrelation gives beside these k.  |k_i| < 1 for every i
    gives a stable 1 / A(z): quantise or modify the k, not the a."""
    k = np.ascontiguousarray(_host_array(k, np.float64).reshape(-1))
    order = _check_order(len(k), "lpcFromReflection")
    a = np.zeros(order)
    _answer(_native.load().speechPlayer_lpcFromReflection(k.ctypes.data, order, a.ctypes.data), order)
    return a


def lpcBandwidthExpand(a, gamma):
    """Bandwidth expansion of prediction coefficients (numpy, no GPU): a float64 [..., order] -> a_j * g_j with g_0 = 1 and
    g_j = g_(j-1) * gamma in binary64, the poles of 1 / A(z) drawn towards the origin by the factor gamma."""
    a = _host_array(a, np.float64)
    gamma = float(gamma)
    if a.ndim < 1 or not math.isfinite(gamma):
        raise ValueError("lpcBandwidthExpand: a [..., order] and a finite gamma (%s, %r)" % (list(a.shape), gamma))
    g, w = 1.0, np.zeros(a.shape[-1])
    for j in range(a.shape[-1]):
        g = g * gamma
        w[j] = g
    return a * w


TEMPO_MIN_WIN = 64               # kTempoMinWin of csrc/klatt_tempo.h
TEMPO_MAX_WIN = 2048             # kTempoMaxWin
TEMPO_MAX_SEARCH = 1024          # kTempoMaxSearch
TEMPO_TILE = 1024                # kTempoTile: consecutive outputs of one row a workgroup of the render takes at a time
TEMPO_RANGE = (0.25, 4.0)


def check_tempo_request(tempo, nWin, search, dtype, rows=None, what="tempoTensor"):
    """The argument checks of BatchPlayer.tempoTensor, tempoPositionsTensor, pcmTempo and signalTempo that need no GPU: tempo a finite number
    in 0.25 .. 4 -- or, with `rows` given, one per row (a scalar stands for all of them) --, nWin an even integer in 64 .. 2048, search
    an integer in 0 .. 1024, dtype None / float32 or int16 (torch's or numpy's).  Raises ValueError or TypeError; the message names the
    row.  Returns (tempo as a float -- with `rows`: a float64 array [rows] --, nWin, search, the format of the samples: 0 int16,
    1 float32)."""
    if isinstance(nWin, (bool, np.bool_)) or not isinstance(nWin, (int, np.integer)) or not TEMPO_MIN_WIN <= nWin <= TEMPO_MAX_WIN or nWin % 2:
        raise ValueError("%s: nWin must be an even integer in %d .. %d, not %r" % (what, TEMPO_MIN_WIN, TEMPO_MAX_WIN, nWin))
    if isinstance(search, (bool, np.bool_)) or not isinstance(search, (int, np.integer)) or not 0 <= search <= TEMPO_MAX_SEARCH:
        raise ValueError("%s: search must be an integer in 0 .. %d, not %r" % (what, TEMPO_MAX_SEARCH, search))
    fmt = _sample_format(dtype, what)
    try:
        t = np.array(_as_array(tempo), dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("%s: tempo must be a number%s, not %r" % (what, "" if rows is None else " or one per row", tempo))
    if rows is None:
        if t.ndim != 0:
            raise ValueError("%s: tempo must be one number, not %s values" % (what, list(t.shape)))
        t = t.reshape(1)
    elif t.ndim == 0:
        t = np.full(rows, float(t), np.float64)
    elif t.ndim != 1 or len(t) != rows:
        raise ValueError("%s: tempo must be a number or one per row (%d), not %s values" % (what, rows, list(t.shape)))
    bad = np.flatnonzero(~(np.isfinite(t) & (t >= TEMPO_RANGE[0]) & (t <= TEMPO_RANGE[1])))
    if len(bad):
        raise ValueError("%s: the tempo of row %d is %r (finite, %g .. %g)" % (what, bad[0], float(t[bad[0]]), TEMPO_RANGE[0], TEMPO_RANGE[1]))
    return (float(t[0]) if rows is None else np.ascontiguousarray(t)), int(nWin), int(search), fmt


def _tempo_lengths(lens, tempo):
    """Lout = ceil(L / tempo), one binary64 division, of each length (speechPlayer_tempoLength's value): int64."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens > 0, np.ceil(lens.astype(np.float64) / tempo), 0).astype(np.int64)


def _tempo_frames(outLens, nWin):
    """K = ceil(Lout / Hs) + 1, or 0 for Lout = 0 (speechPlayer_tempoFrames' value): int64."""
    outLens, hs = np.asarray(outLens, dtype=np.int64), nWin // 2
    return np.where(outLens > 0, (outLens + hs - 1) // hs + 1, 0).astype(np.int64)


def tempoLength(length, tempo):
    """The samples a row of `length` samples has at `tempo` (speechPlayer_tempoLength; no GPU): ceil(length / tempo)."""
    return int(_answer(_native.load().speechPlayer_tempoLength(int(length), float(tempo)), error=ValueError))


def tempoFrames(length, tempo, nWin=512):
    """The frames -- positions -- of a row of `length` samples at `tempo` (speechPlayer_tempoFrames; no GPU): ceil(Lout / (nWin / 2)) + 1,
    0 for an empty row."""
    return int(_answer(_native.load().speechPlayer_tempoFrames(int(length), float(tempo), int(nWin)), error=ValueError))


def _tempo_statement(what, s, inFormat, tempo, nWin, search, positions, dtype, returnPositions):
    tempo, nWin, search, fmt = check_tempo_request(tempo, nWin, search, dtype, None, what)
    Lout = int(_tempo_lengths(len(s), tempo))
    K = int(_tempo_frames(Lout, nWin))
    given = None
    if positions is not None:
        given = np.ascontiguousarray(_host_array(positions, np.int64).reshape(-1))
        if len(given) != K:
            raise ValueError("%s: %d positions for %d frames" % (what, len(given), K))
    got = np.zeros(K, np.int64)
    y = _row_statement(what, s, inFormat, (tempo, nWin, search, given.ctypes.data if given is not None and K else None, got.ctypes.data if K else None, fmt),
                       (Lout,), np.float32 if fmt else np.int16)
    return (y, got) if returnPositions else y


def pcmTempo(pcm, tempo, nWin=512, search=160, positions=None, dtype=np.float32, returnPositions=False):
    """int16 PCM at another tempo by WSOLA on the host (speechPlayer_pcmTempo; no GPU), by the definition in include/speechPlayer_batch.h:
    -> float32 or int16 [ceil(len / tempo)], with returnPositions (y, positions int64 [K]).  A tempo above 1 is faster speech; the pitch
    stays.  nWin is the (Hann) window, its half the hop of the output; `search` the lags either side of the nominal position among which
    frame k takes the one whose segment correlates best with the natural continuation of frame k - 1 (0: plain overlap-add).
    positions: render these (K = tempoFrames(len, tempo, nWin) of them) instead of searching."""
    return _tempo_statement("pcmTempo", _pcm_samples(pcm, "pcmTempo"), None, tempo, nWin, search, positions, dtype, returnPositions)


def signalTempo(x, tempo, nWin=512, search=160, positions=None, dtype=np.float32, returnPositions=False):
    """pcmTempo on a signal's row (speechPlayer_signalTempo; no GPU): x as signalSpectrogram's.  The statement
    BatchPlayer.tempoTensor(signal=...) is held to."""
    return _tempo_statement("signalTempo", *_signal_samples(x, "signalTempo"), tempo, nWin, search, positions, dtype, returnPositions)


def tempoMap(positions, nWin, outLength):
    """The time map of a tempo export (numpy, no GPU): int64 [outLength], per output sample m the input sample of the segment with the
    larger window weight -- with q = m // Hs and i = m - q * Hs, positions[q] + i for i < Hs / 2, else positions[q + 1] - Hs + i.  It
    carries the label grids of the other exports across: labels_at_tempo = labels[np.clip(tempoMap(...), 0, L - 1)]."""
    p = np.ascontiguousarray(_host_array(positions, np.int64).reshape(-1))
    if isinstance(nWin, (bool, np.bool_)) or not isinstance(nWin, (int, np.integer)) or nWin < 2 or nWin % 2:
        raise ValueError("tempoMap: nWin must be an even integer, not %r" % (nWin,))
    hs, outLength = int(nWin) // 2, int(outLength)
    need = int(_tempo_frames(max(outLength, 0), nWin))
    if outLength < 0 or len(p) < need:
        raise ValueError("tempoMap: %d outputs take %d positions, not %d" % (outLength, need, len(p)))
    m = np.arange(outLength, dtype=np.int64)
    q, i = m // hs, m % hs
    return np.where(2 * i < hs, p[q] + i, p[q + 1] - hs + i) if outLength else m


MIX_TILE = 1024                  # kMixTile of csrc/klatt_mix.h: consecutive outputs of one row a workgroup takes at a time
MIX_MAX_TERMS = 64               # kMixMaxTerms: of one row
MIX_MAX_CALL_TERMS = 1 << 22     # kMixMaxCallTerms: of one call
MIX_MAX_CLIPS = 1 << 20          # kMixMaxClips: of a noise bank
MIX_MAX_BANK = 1 << 28           # kMixMaxBank: samples of a noise bank
SIGNAL_POWER_BLOCK = 2048        # kSigPowerBlock of csrc/klatt_sigpower.h: consecutive samples of one block of a float32 row's power
SIGNAL_POWER_MAX_BLOCKS = 1 << 24    # kSigPowerMaxBlocks: block partials of one call
# speechPlayer_mixTerm_t and speechPlayer_mixSource_t (include/speechPlayer_batch.h)
mixTermDtype = np.dtype([("kind", np.int32), ("levelKind", np.int32), ("source", np.int64), ("offset", np.int64), ("level", np.float64),
                         ("loop", np.int32), ("reserved", np.int32)], align=True)
_mixSourceDtype = np.dtype([("data", np.uint64), ("length", np.int64), ("format", np.int32), ("reserved", np.int32)], align=True)
assert mixTermDtype.itemsize == 40 and _mixSourceDtype.itemsize == 24


class MixTerm(object):
    """One term of a mixture (speechPlayer_mixTerm_t): a clip of the noise bank (noise=k) or an utterance of the batch (utterance=u), at
    a signal-to-noise ratio in dB against the row's own utterance (snr=) or at a linear gain (gain=), placed at `offset`: looped
    (src[(offset + m) mod N], 0 <= offset < N) or, loop=False, once (src[m - offset], silence outside; a negative offset skips the
    source's beginning)."""
    __slots__ = ("kind", "levelKind", "source", "offset", "level", "loop")

    def __init__(self, noise=None, utterance=None, snr=None, gain=None, offset=0, loop=True):
        if (noise is None) == (utterance is None):
            raise ValueError("MixTerm: exactly one of noise= and utterance=")
        if (snr is None) == (gain is None):
            raise ValueError("MixTerm: exactly one of snr= and gain=")
        for name, v in (("noise", noise), ("utterance", utterance), ("offset", offset)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise TypeError("MixTerm: %s must be an integer, not %r" % (name, v))
        if not isinstance(loop, (bool, np.bool_)) and loop not in (0, 1):
            raise ValueError("MixTerm: loop must be True or False, not %r" % (loop,))
        self.kind, self.source = (0, int(noise)) if utterance is None else (1, int(utterance))
        self.levelKind, self.level = (0, float(snr)) if gain is None else (1, float(gain))
        self.offset, self.loop = int(offset), int(bool(loop))

    def record(self):
        return (self.kind, self.levelKind, self.source, self.offset, self.level, self.loop, 0)

    def __repr__(self):
        return "MixTerm(%s=%d, %s=%r, offset=%d, loop=%r)" % ("utterance" if self.kind else "noise", self.source, "gain" if self.levelKind else "snr",
                                                              self.level, self.offset, bool(self.loop))


def _mix_terms(terms, what):
    """A list of MixTerm or a structured array of mixTermDtype -> a contiguous array of mixTermDtype."""
    if isinstance(terms, np.ndarray):
        if terms.dtype != mixTermDtype or terms.ndim != 1:
            raise TypeError("%s: an array of terms must be one-dimensional, of mixTermDtype, not %s %s" % (what, terms.dtype, list(terms.shape)))
        return np.ascontiguousarray(terms)
    if isinstance(terms, MixTerm):
        terms = [terms]
    if not isinstance(terms, (list, tuple)) or not all(isinstance(t, MixTerm) for t in terms):
        raise TypeError("%s: terms must be MixTerm objects or an array of mixTermDtype" % what)
    return np.array([t.record() for t in terms], dtype=mixTermDtype).reshape(-1)


def _sample_format(dtype, what):
    """dtype None / torch.float32 / np.float32 / "float32" or torch.int16 / np.int16 / "int16" (TypeError): -> the format of exported
    samples, 1 float32 or 0 int16."""
    names = {"float32": 1, "int16": 0}
    key = "float32" if dtype is None else (str(dtype).replace("torch.", "") if type(dtype).__module__.startswith("torch") else None)
    if key is None:
        try:
            key = np.dtype(dtype).name
        except TypeError:
            key = repr(dtype)
    if key not in names:
        raise TypeError("%s: dtype must be float32 or int16, not %s" % (what, dtype))
    return names[key]


def check_mix_request(terms, nRows, speechGain, dtype, what="mixedTensor", signalRows=None):
    """The argument checks of BatchPlayer.mixedTensor that need no GPU, before any library call: terms a list of nRows lists of MixTerm
    (a row with no terms: an empty list) or a pair (array of mixTermDtype, termStart: nRows + 1 integers from 0, not decreasing, the last
    the array's length); at most 64 terms in a row and 2^22 in all; speechGain None, one number or nRows of them; dtype None /
    torch.float32 / np.float32 (float32) or torch.int16 / np.int16.  The values of the terms are the library's to refuse.  signalRows:
    the mix is made onto a signal of that many rows (mixedTensor(signal=...)): MixTerm(utterance=k) names row k of it, and one outside
    0 .. signalRows - 1 is refused here, by row and term.  Raises ValueError or TypeError.  Returns (the terms: mixTermDtype, termStart: int64, speechGain: float32 [nRows] or None, the export format:
    0 int16, 1 float32)."""
    if isinstance(terms, tuple) and len(terms) == 2 and isinstance(terms[0], np.ndarray):
        flat = _mix_terms(terms[0], what)
        start = _as_array(terms[1])
        if start.dtype.kind not in "iu" or start.ndim != 1:
            raise TypeError("%s: termStart must be a one-dimensional array of integers, not %s %s" % (what, start.dtype, list(start.shape)))
        start = np.ascontiguousarray(start.astype(np.int64))
        if len(start) != nRows + 1:
            raise ValueError("%s: termStart has %d entries for %d rows (one more than the rows)" % (what, len(start), nRows))
        if start[0] != 0 or np.any(np.diff(start) < 0) or start[-1] != len(flat):
            raise ValueError("%s: termStart must start at 0, not decrease and end at the number of terms (%d)" % (what, len(flat)))
    else:
        if not isinstance(terms, (list, tuple)):
            raise TypeError("%s: terms must be a list of one list of MixTerm per row, or (array of mixTermDtype, termStart)" % what)
        if len(terms) != nRows:
            raise ValueError("%s: terms has %d entries for %d rows" % (what, len(terms), nRows))
        rows = [_mix_terms([] if row is None else row, what) for row in terms]
        start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        flat = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros(0, mixTermDtype)
    counts = np.diff(start)
    if len(counts) and counts.max() > MIX_MAX_TERMS:
        raise ValueError("%s: row %d has %d terms (at most %d)" % (what, int(counts.argmax()), int(counts.max()), MIX_MAX_TERMS))
    if len(flat) > MIX_MAX_CALL_TERMS:
        raise ValueError("%s: %d terms in all (at most %d)" % (what, len(flat), MIX_MAX_CALL_TERMS))
    if signalRows is not None:
        if isinstance(signalRows, bool) or not isinstance(signalRows, (int, np.integer)) or signalRows < 0:
            raise TypeError("%s: signalRows must be a count of rows, not %r" % (what, signalRows))
        bad = np.flatnonzero((flat["kind"] == 1) & ((flat["source"] < 0) | (flat["source"] >= signalRows)))
        if len(bad):
            row = int(np.searchsorted(start, bad[0], side="right")) - 1
            raise ValueError("%s: row %d, term %d: source %d is not a row of the signal (%d)" % (what, row, bad[0] - start[row], flat["source"][bad[0]], signalRows))
    sg = None
    if speechGain is not None:
        sg = _as_array(speechGain)
        if sg.dtype.kind not in "fiu" or sg.ndim > 1:
            raise TypeError("%s: speechGain must be a number or a one-dimensional array of them, not %s %s" % (what, sg.dtype, list(sg.shape)))
        if sg.ndim == 1 and len(sg) != nRows:
            raise ValueError("%s: speechGain has %d entries for %d rows" % (what, len(sg), nRows))
        with np.errstate(over="ignore"):
            sg = np.ascontiguousarray(np.broadcast_to(sg.astype(np.float32), (nRows,)))
    return flat, start, sg, _sample_format(dtype, what)


def _mix_clip(a, what, name):
    a = _as_array(a)
    if a.ndim != 1 or a.dtype.kind != "f":
        raise TypeError("%s: %s must be a one-dimensional array of floats, not %s %s" % (what, name, a.dtype, list(a.shape)))
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a.astype(np.float32))


def pcmMix(pcm, sources, terms, speechGain=1.0, dtype=np.float32, gains=False):
    """int16 PCM mixed with other signals on the host (speechPlayer_pcmMix; no GPU): -> float32 (sample / 32767 scale) or int16
    [len(pcm)], by the definition in include/speechPlayer_batch.h -- the statement the device is held to bit for bit.  sources: a list
    of one-dimensional arrays, float32 (a noise clip) or int16 (an utterance); terms: MixTerm objects (or an array of mixTermDtype) whose
    noise= / utterance= index `sources` -- noise= a float32 source, utterance= an int16 one.  An SNR is taken against the whole-signal
    mean square of `pcm` at gain 1.  gains=True: -> (mixed, the float32 gains applied, one per term)."""
    return _mix_statement("pcmMix", _pcm_samples(pcm, "pcmMix"), None, sources, terms, speechGain, dtype, gains)


def _mix_statement(what, s, inFormat, sources, terms, speechGain, dtype, gains):
    if not isinstance(sources, (list, tuple)):
        raise TypeError("%s: sources must be a list of one-dimensional arrays" % what)
    held, table = [], np.zeros(max(len(sources), 1), _mixSourceDtype)
    for k, a in enumerate(sources):
        a = _as_array(a)
        a = np.ascontiguousarray(a) if a.dtype == np.int16 and a.ndim == 1 else _mix_clip(a, what, "source %d" % k)
        held.append(a)
        table[k] = (a.ctypes.data if len(a) else 0, len(a), 0 if a.dtype == np.int16 else 1, 0)
    flat = _mix_terms(terms, what)
    fmt = _sample_format(dtype, what)
    g = np.zeros(max(len(flat), 1), np.float32)
    out = _row_statement(what, s, inFormat, (float(np.float32(speechGain)), table.ctypes.data if len(sources) else None, len(sources),
                                             flat.ctypes.data if len(flat) else None, len(flat), g.ctypes.data, fmt), len(s), np.float32 if fmt else np.int16)
    return (out, g[:len(flat)]) if gains else out


def signalMix(x, sources, terms, speechGain=1.0, dtype=np.float32, gains=False):
    """pcmMix on a signal's row (speechPlayer_signalMix; no GPU): x is a one-dimensional int16 array (pcmMix's bits) or a float32 one,
    taken as it is -- every sample finite and at most 2^16 in magnitude.  sources and terms as pcmMix's, but utterance= names a ROW: a
    source of either dtype, whose power is signalPower's; noise= names a float32 clip.  An SNR is taken against signalPower(x).  The
    statement BatchPlayer.mixedTensor(signal=...) is held to."""
    return _mix_statement("signalMix", *_signal_samples(x, "signalMix"), sources, terms, speechGain, dtype, gains)


def signalPower(x):
    """The power of a signal's row (speechPlayer_signalPower; no GPU): x as signalMix's.  int16: the exact integer sum of squares over
    the length over 32767^2; float32: the squares in binary64 through the fixed tree of csrc/klatt_sigpower.h -- leaves of 8 samples in
    ascending order, a balanced tree over the 256 leaves of a block of 2048, the blocks in ascending order -- over the length.  Whole-signal
    mean squares, silences included; 0.0 for no samples.  The statement BatchPlayer.powerTensor(signal=...) is held to."""
    s, inFormat = _signal_samples(x, "signalPower")
    power = np.zeros(1, np.float64)
    _answer(_native.load().speechPlayer_signalPower(s.ctypes.data if len(s) else None, inFormat, len(s), power.ctypes.data))
    return float(power[0])


def check_option_value(name, value):
    """speechPlayer_batch_setOption takes a C int: a value outside its range would wrap without a word (2 ** 40 arrives as 0).  Returns
    int(value), or raises ValueError."""
    value = int(value)
    if not -2 ** 31 <= value < 2 ** 31:
        raise ValueError("setOption(%r): %d does not fit the option's C int (-2**31 .. 2**31 - 1)" % (name, value))
    return value


def _ptr(a):
    return None if a is None else a.ctypes.data


def _ready_stream(owner, dev):
    """The hipStream_t a device-frames call is ordered behind: torch's current stream on `dev`.  torch's default stream is the NULL stream,
    which the engine reads as "ready now": a stream of `owner`'s own that waits for it on the device carries the order instead."""
    import torch
    cur = torch.cuda.current_stream(dev)
    if cur.cuda_stream:
        return cur.cuda_stream
    if getattr(owner, "_ready", None) is None:
        owner._ready = torch.cuda.Stream(dev)
    owner._ready.wait_stream(cur)
    return owner._ready.cuda_stream


# kStageResample, kStageFilter, kStageCode, kStageConvolve, kStageSpectrogram of csrc/klatt_stage.h
STAGE_KINDS = ["resample", "filter", "code", "convolution", "spectrogram"]
# kStageLpc, kStagePitch: the kinds on the step grid beside the spectrogram (csrc/klatt_stage_frames.h); kind number len(STAGE_KINDS) + index
STAGE_FRAME_KINDS = ["lpc", "pitch"]
STAGE_MAKERS = {"convolution": "convolveStage", "spectrogram": "spectrogramStage"}      # (the others: kind + "Stage")
STAGE_MAX_ROWS = 1 << 20                          # kStageMaxRows
STAGE_MAX_HISTORY = 1 << 27                       # kStageMaxHistory: float32 of history per buffer, all rows of a stage together


def check_stage_request(kind, nRows, *args, **kw):
    """The argument checks of BatchPlayer.resampleStage, filterStage, codeStage, convolveStage and spectrogramStage that need no GPU,
    before any library call: kind a name of STAGE_KINDS; nRows an integer in 1 .. 2^20; then, by kind, the arguments of the whole-row
    export and its checks -- "resample": (srcRate, rate, zeros=6, rolloff=0.99, window="hann", beta=None) through
    check_resample_request; "filter": (filters, filterOf=None, tail=0) through check_filter_request, filterOf per row of the stage;
    "code": (codec) through check_codec_request; "convolution": (irs, irOf=None, tail=True) through check_convolve_request, irOf per
    row of the stage; "spectrogram": (nFft=1024, hop=256, phase=0, window=None, bank=None, power=2, log=None, floor=1e-10) through
    check_spectrogram_request -- and, for the last two, the rows' histories (taps - 1 each; nFft - 1 each) within 2^27 samples in all.
    A name of STAGE_FRAME_KINDS likewise -- "lpc": (order=16, nWin=512, hop=256, phase=0, window=None, lagWindow=None,
    fields=("lpc", "error")) through check_lpc_request; "pitch": (sampleRate, fmin=60.0, fmax=500.0, nWin=1024, hop=256, phase=0,
    threshold=0.1, fields=("f0", "aperiodicity"), lagMin=None, lagMax=None) through check_pitch_request --, the histories nWin - 1 and
    nWin + lagMax - 1 a row.  Raises KeyError (the kind, the codec, a field), ValueError or TypeError.  Returns (kind's number, nRows, what
    the kind's check returns)."""
    kinds = STAGE_KINDS + STAGE_FRAME_KINDS
    what = STAGE_MAKERS.get(kind, "%sStage" % kind) if kind in kinds else "stage"
    if kind not in kinds:
        raise KeyError("%s: kind %r (%s)" % (what, kind, ", ".join(kinds)))
    if isinstance(nRows, (bool, np.bool_)) or not isinstance(nRows, (int, np.integer)):
        raise TypeError("%s: nRows must be an integer, not %r" % (what, nRows))
    if not 1 <= nRows <= STAGE_MAX_ROWS:
        raise ValueError("%s: nRows must lie in 1 .. 2^20, not %d" % (what, nRows))
    nRows = int(nRows)
    if kind == "resample":
        def plan(srcRate, rate, zeros=6, rolloff=0.99, window="hann", beta=None):
            return check_resample_request(srcRate, rate, zeros, rolloff, window, beta, None, what)
    elif kind == "filter":
        def plan(filters, filterOf=None, tail=0):
            return check_filter_request(filters, filterOf, nRows, tail, None, what)
    elif kind == "convolution":
        def plan(irs, irOf=None, tail=True):
            got = check_convolve_request(irs, irOf, nRows, tail, None, what)
            taps = np.diff(got[1])
            history = int((taps[got[2]] - 1).sum()) if got[2] is not None else int(taps[0] - 1) * nRows
            if history > STAGE_MAX_HISTORY:
                raise ValueError("%s: the rows' histories take %d samples in all (at most 2^27)" % (what, history))
            return got
    elif kind == "spectrogram":
        def plan(nFft=1024, hop=256, phase=0, window=None, bank=None, power=2, log=None, floor=1e-10):
            got = check_spectrogram_request(nFft, hop, phase, window, bank, power, log, floor, None, what)
            if (got[0] - 1) * nRows > STAGE_MAX_HISTORY:
                raise ValueError("%s: the rows' histories take %d samples in all (at most 2^27)" % (what, (got[0] - 1) * nRows))
            return got
    elif kind == "lpc":
        def plan(order=16, nWin=512, hop=256, phase=0, window=None, lagWindow=None, fields=("lpc", "error")):
            got = check_lpc_request(order, nWin, hop, phase, window, lagWindow, fields, None, what)
            if (got[1] - 1) * nRows > STAGE_MAX_HISTORY:
                raise ValueError("%s: the rows' histories take %d samples in all (at most 2^27)" % (what, (got[1] - 1) * nRows))
            return got
    elif kind == "pitch":
        def plan(sampleRate, fmin=60.0, fmax=500.0, nWin=1024, hop=256, phase=0, threshold=0.1, fields=("f0", "aperiodicity"), lagMin=None, lagMax=None):
            got = check_pitch_request(sampleRate, fmin, fmax, lagMin, lagMax, nWin, hop, phase, threshold, fields, None, what)
            if (got[1] + got[3] - 1) * nRows > STAGE_MAX_HISTORY:
                raise ValueError("%s: the rows' histories take %d samples in all (at most 2^27)" % (what, (got[1] + got[3] - 1) * nRows))
            return got
    else:
        def plan(codec):
            return check_codec_request(codec, True, True, None, what)
    return kinds.index(kind), nRows, plan(*args, **kw)


def check_stage_push(kind, nRows, signal, end=None, dtype=None, codes=False, decoded=True, device=None, what="SignalStage.push"):
    """The argument checks of SignalStage.push that need no GPU: signal as check_signal_request's, of exactly nRows rows; end None, a bool
    or nRows bools; dtype as the kind's export takes it (None: float32, a code stage's int16; a spectrogram, lpc or pitch stage takes
    torch.float32 or torch.float64); codes and decoded bools that only a code stage takes otherwise than (False, True), not both False.  Raises ValueError
    or TypeError.  Returns (check_signal_request's answer, end: uint8 [nRows] or None, the output format: 0 int16, 1 float32 -- a
    spectrogram stage's: 0 float64, 1 float32 --, codes, decoded)."""
    if kind not in STAGE_KINDS + STAGE_FRAME_KINDS:
        raise KeyError("%s: kind %r (%s)" % (what, kind, ", ".join(STAGE_KINDS + STAGE_FRAME_KINDS)))
    sig = check_signal_request(signal, device, what)
    if sig[2] != nRows:
        raise ValueError("%s: a chunk of %d rows for a stage of %d" % (what, sig[2], nRows))
    if end is None:
        flags = None
    elif isinstance(end, (bool, np.bool_)):
        flags = np.full(nRows, 1 if end else 0, np.uint8)
    else:
        a = _as_array(end)
        if a.dtype.kind != "b" or a.ndim != 1:
            raise TypeError("%s: end must be None, True, False or a one-dimensional array of bools, not %s %s" % (what, a.dtype, list(a.shape)))
        if len(a) != nRows:
            raise ValueError("%s: end has %d entries for %d rows" % (what, len(a), nRows))
        flags = np.ascontiguousarray(a.astype(np.uint8))
    for name, v in (("codes", codes), ("decoded", decoded)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError("%s: %s must be True or False, not %r" % (what, name, v))
    if kind != "code":
        if codes or not decoded:
            raise ValueError("%s: codes and decoded belong to a code stage" % what)
        fmt = _check_dtype(what, dtype, *_float_types()) if kind == "spectrogram" or kind in STAGE_FRAME_KINDS else _sample_format(dtype, what)
    else:
        if not codes and not decoded:
            raise ValueError("%s: codes, decoded or both" % what)
        fmt = _int16_format(dtype, what)
    return sig, flags, fmt, bool(codes), bool(decoded)


def resampleEmitted(consumed, srcRate, dstRate, zeros=6, rolloff=0.99, ended=False):
    """The outputs a resampler stage has emitted for a row after `consumed` samples, open or ended (speechPlayer_resampleEmitted; no GPU):
    open, ceil(max(consumed - Z, 0) * up / down) -- the outputs whose taps all lie at or before the last sample consumed --; ended,
    ceil(consumed * up / down), pcmResample's length.  Equal rates: consumed.  The difference of two is what a push emits."""
    srcRate, dstRate, zeros, rolloff = check_resample_request(srcRate, dstRate, zeros, rolloff, "hann", None, None, "resampleEmitted")[:4]
    return _answer(_native.load().speechPlayer_resampleEmitted(int(consumed), srcRate, dstRate, zeros, rolloff, 1 if ended else 0), error=ValueError)


def spectrogramEmitted(consumed, nFft=1024, hop=256, phase=0, ended=False):
    """The steps a spectrogram stage has emitted for a row after `consumed` samples, open or ended (speechPlayer_spectrogramEmitted; no
    GPU): open, the steps j whose whole frame lies at or before the last sample consumed, phase + j * hop + nFft / 2 - 1 <= consumed - 1;
    ended, ceil((consumed - phase) / hop), pcmSpectrogram's count.  The difference of two is what a push emits."""
    return _answer(_native.load().speechPlayer_spectrogramEmitted(int(consumed), int(nFft), int(hop), int(phase), 1 if ended else 0), error=ValueError)


def lpcEmitted(consumed, nWin=512, hop=256, phase=0, ended=False):
    """The steps an LPC stage has emitted for a row after `consumed` samples, open or ended (speechPlayer_lpcEmitted; no GPU): open, the
    steps j whose whole frame lies at or before the last sample consumed, phase + j * hop - nWin // 2 + nWin - 1 <= consumed - 1; ended,
    ceil((consumed - phase) / hop), pcmLpc's count.  The difference of two is what a push emits."""
    return _answer(_native.load().speechPlayer_lpcEmitted(int(consumed), int(nWin), int(hop), int(phase), 1 if ended else 0), error=ValueError)


def pitchEmitted(consumed, nWin=1024, lagMax=368, hop=256, phase=0, ended=False):
    """The steps a pitch stage has emitted for a row after `consumed` samples, open or ended (speechPlayer_pitchEmitted; no GPU): as
    lpcEmitted with the frame of nWin + lagMax samples (lagMax 368: 60 Hz at 22050 Hz, pitchLags); ended, pcmPitch's count."""
    return _answer(_native.load().speechPlayer_pitchEmitted(int(consumed), int(nWin), int(lagMax), int(hop), int(phase), 1 if ended else 0), error=ValueError)


class SignalStage(object):
    """The per-row state of one sequential export -- the resampler, the biquad filter, a codec, the convolution, the spectrogram, the LPC
    analysis or the pitch -- on a BatchPlayer's device, fed chunk by chunk (include/speechPlayer_batch.h, "Signal stages", "Signal stages
    that keep a window" and "Signal stages on the step grid"): what a live handle's pulls go through.  Made by BatchPlayer.resampleStage,
    filterStage, codeStage, convolveStage, spectrogramStage, lpcStage and pitchStage; freed by close() or with the player."""

    def __init__(self, player, kind, nRows, handle, bands=None, columns=None):
        self._bp, self.kind, self.nRows, self._h = player, kind, nRows, handle
        self.bands = bands      # a spectrogram stage's values per step
        self.columns = bands if columns is None else columns      # the values per step of any kind on the step grid
        self._dll = player._dll

    def _handle(self):
        if not getattr(self, "_h", None) or not getattr(self._bp, "_h", None):
            raise RuntimeError("SignalStage: the stage was closed, or its player was")
        return self._h

    def plan(self, lengths, end=None):
        """What a push of rows of these lengths with these end flags would emit per row (speechPlayer_stage_plan; host only, changes
        nothing): -> int64 [nRows]."""
        lens = _host_array(lengths, np.int64).reshape(-1)
        if len(lens) != self.nRows:
            raise ValueError("SignalStage.plan: %d lengths for %d rows" % (len(lens), self.nRows))
        flags = None if end is None else np.ascontiguousarray(np.broadcast_to(_as_array(end), (self.nRows,)).astype(np.uint8))
        out = np.zeros(self.nRows, np.int64)
        _answer(self._dll.speechPlayer_stage_plan(self._handle(), lens.ctypes.data, _ptr(flags), out.ctypes.data), error=ValueError)
        return out

    def push(self, signal, end=None, dtype=None, padded=True, codes=False, decoded=True):
        """Feed every row its next chunk (speechPlayer_stage_push), on torch's current stream without a host wait: signal the (tensor,
        lengths or offsets) pair an export, a pull or another stage returns, of exactly nRows rows -- a row of length 0 is untouched --;
        end None, a bool or nRows bools: the rows this push ends (a resampler then emits its last outputs, a filter its tail, and the
        row is fresh afterwards).  -> (tensor, lengths), as the whole-row export returns them -- dtype torch.float32 (default) or
        torch.int16; padded [nRows, most] with +0 past each row's outputs, or packed with the nRows + 1 offsets --; a code stage
        -> (decoded, lengths), (decoded, codes, lengths) or (codes, lengths) as codedTensor, dtype torch.int16 by default; a
        spectrogram stage -> (tensor [nRows, most steps, bands], steps) or, packed, ([total steps, bands], the nRows + 1 offsets), dtype
        torch.float32 (default) or torch.float64, and takes neither codes nor decoded; an lpc or pitch stage likewise, -> (tensor [nRows,
        most steps, columns], steps) or the packed form.  The outputs of a row's pushes, concatenated, are bit for bit signalResample /
        signalFilter / signalCode / signalConvolve / signalLpc / signalPitch of its chunks concatenated, and signalSpectrogram's (its
        linear values bit for bit, a logarithm's within the spectrogram export's bar)."""
        import torch
        h, dev = self._handle(), self._bp.device
        sig, flags, fmt, codes, decoded = check_stage_push(self.kind, self.nRows, signal, end, dtype, codes, decoded, dev)
        tensor, inFormat, rows, stride, extent, lens = sig
        counts = np.zeros(self.nRows, np.int64)
        _answer(self._dll.speechPlayer_stage_plan(h, lens.ctypes.data, _ptr(flags), counts.ctypes.data), error=ValueError)
        if padded:
            outStride = max(int(counts.max()), 1)      # (rowStride 0 would mean packed)
            shape, second = (self.nRows, outStride), counts
        else:
            outStride, second = 0, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            shape = (int(second[-1]),)
        record = np.zeros(1, _signalDtype)
        record["data"], record["format"], record["nRows"], record["rowStride"], record["extent"] = tensor.data_ptr(), inFormat, rows, stride, extent.ctypes.data
        name = "cuda:%d" % dev
        if self.kind == "spectrogram" or self.kind in STAGE_FRAME_KINDS:
            shape, low = shape + (self.columns,), torch.float64
        else:
            low = torch.int16
        d = torch.empty(shape, dtype=torch.float32 if fmt else low, device=name) if decoded else None
        c = torch.empty(shape, dtype=torch.uint8, device=name) if codes else None
        numel = int(np.prod(shape))
        got = self._dll.speechPlayer_stage_push(h, record.ctypes.data, _ptr(flags), d.data_ptr() if decoded and numel else None, fmt,
                                                c.data_ptr() if codes and numel else None, outStride, None, torch.cuda.current_stream(dev).cuda_stream)
        if got < 0:
            raise RuntimeError("SignalStage.push failed: %s" % _native.last_error())
        assert got == numel, (got, numel)
        if padded and not counts.max():      # (rows of nothing: the width the whole-row exports give)
            d, c = (None if t is None else t[:, :0] for t in (d, c))
        return tuple(t for t in (d, c) if t is not None) + (torch.from_numpy(second),)

    def reset(self, rows=None):
        """Make rows fresh again -- nothing consumed, nothing emitted, the state +0 -- behind the stage's last push: rows None (all) or
        nRows bools."""
        import torch
        flags = None
        if rows is not None:
            a = _as_array(rows)
            if a.dtype.kind != "b" or a.shape != (self.nRows,):
                raise TypeError("SignalStage.reset: rows must be None or %d bools" % self.nRows)
            flags = np.ascontiguousarray(a.astype(np.uint8))
        dev = self._bp.device
        if self._dll.speechPlayer_stage_reset(self._handle(), _ptr(flags), torch.cuda.current_stream(dev).cuda_stream) < 0:
            raise RuntimeError("SignalStage.reset failed: %s" % _native.last_error())

    def _counts(self, which):
        out = np.zeros(self.nRows, np.int64)
        if self._dll.speechPlayer_stage_counts(self._handle(), *((out.ctypes.data, None) if which == 0 else (None, out.ctypes.data))) < 0:
            raise RuntimeError("SignalStage: %s" % _native.last_error())
        return out

    @property
    def consumed(self):
        """The samples every row has consumed since its start (its creation, its last end or its last reset): int64 [nRows]."""
        return self._counts(0)

    @property
    def emitted(self):
        """The outputs every row has emitted since its start: int64 [nRows]."""
        return self._counts(1)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._bp, "_h", None):      # (a stage goes with its player)
                self._dll.speechPlayer_stage_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SignalChain(object):
    """Stages one behind the other: push feeds each stage's (tensor, lengths) pair to the next as its chunk, and `end` travels with it --
    pcm, produced = group.pullTensor(8192); y = chain.push((pcm, produced)).  A code stage or a spectrogram stage comes last: what it
    gives is not a signal, and so does an lpc or a pitch stage.  The last element may be a tuple or a list of such terminal stages, a fan:
    SignalChain([filterStage, resampleStage, (lpcStage, pitchStage, codeStage)]) feeds the chunk that arrives there to each of them."""

    def __init__(self, stages):
        stages = list(stages)
        if any(isinstance(s, (tuple, list)) for s in stages[:-1]):
            raise ValueError("SignalChain: a fan of stages comes last")
        self.fan = None
        if stages and isinstance(stages[-1], (tuple, list)):
            self.fan = list(stages.pop())
            if not self.fan:
                raise TypeError("SignalChain: a fan holds one stage at least")
        self.stages = stages + (self.fan or [])
        if not self.stages or not all(isinstance(s, SignalStage) for s in self.stages):
            raise TypeError("SignalChain: a list of SignalStage objects, at least one")
        for kind in ("code", "spectrogram") + tuple(STAGE_FRAME_KINDS):
            if any(s.kind == kind for s in stages[:-1 if self.fan is None else len(stages)]):
                raise ValueError("SignalChain: %s stage comes last" % ("an lpc" if kind == "lpc" else "a " + kind))
        if len({s.nRows for s in self.stages}) != 1:
            raise ValueError("SignalChain: the stages have %s rows" % sorted({s.nRows for s in self.stages}))

    def push(self, signal, end=None, **last):
        """The chunk through every stage; the keywords (dtype, padded, codes, decoded) are the last stage's push's, the stages between
        hand on float32 padded rows.  With a fan at the end: -> a tuple of its stages' results, in order, each with its defaults (no
        keywords)."""
        if self.fan is not None:
            if last:
                raise TypeError("SignalChain.push: a fan's stages take their defaults, not %s" % ", ".join(sorted(last)))
            for s in self.stages[:len(self.stages) - len(self.fan)]:
                signal = s.push(signal, end)
            return tuple(s.push(signal, end) for s in self.fan)
        for s in self.stages[:-1]:
            signal = s.push(signal, end)
        return self.stages[-1].push(signal, end, **last)

    def reset(self, rows=None):
        for s in self.stages:
            s.reset(rows)


class BatchPlayer(object):
    """N independent utterances per launch (include/speechPlayer_batch.h)."""

    def __init__(self, sampleRate, device=-1, mode=0, layout=None):
        """mode: SPEECHPLAYER_MODE_EXACT (0) or _FAST (1); layout: None / -1 = chosen per batch (default),
        1 = stage-parallel workgroups, 0 = one wavefront per 64 utterances."""
        self.sampleRate = sampleRate
        self._dll = _native.load()
        self._h = self._dll.speechPlayer_batch_create(sampleRate, device)
        if not self._h:
            raise RuntimeError("speechPlayer_batch_create failed: %s" % _native.last_error())
        self._check(self._dll.speechPlayer_batch_setOption(self._h, b"mode", mode))
        if layout is not None:
            self._check(self._dll.speechPlayer_batch_setOption(self._h, b"layout", layout))
        self.nUtterances = 0

    def _check(self, rc):
        if rc is None or rc < 0:
            raise RuntimeError("speechPlayer batch call failed: %s" % _native.last_error())
        return rc

    def setOption(self, name, value):
        self._check(self._dll.speechPlayer_batch_setOption(self._h, name.encode(), check_option_value(name, value)))

    def setUtterances(self, frameStart, frames, minSamples, fadeSamples, userIndex=None, isNull=None, noiseSeed=None):
        fs = np.ascontiguousarray(frameStart, dtype=np.int64)
        fr = np.ascontiguousarray(frames, dtype=np.float64).reshape(-1, 47)
        m = np.ascontiguousarray(minSamples, dtype=np.uint32)
        f = np.ascontiguousarray(fadeSamples, dtype=np.uint32)
        n_utt = len(fs) - 1
        assert fs[-1] == len(fr) == len(m) == len(f)
        ix = None if userIndex is None else np.ascontiguousarray(userIndex, dtype=np.int32)
        nu = None if isNull is None else np.ascontiguousarray(isNull, dtype=np.uint8)
        sd = None if noiseSeed is None else np.ascontiguousarray(noiseSeed, dtype=np.uint32)
        p = lambda a: None if a is None else a.ctypes.data
        self._check(self._dll.speechPlayer_batch_setUtterances(self._h, n_utt, p(fs), p(fr), p(m), p(f), p(ix), p(nu), p(sd)))
        self.nUtterances = n_utt

    @property
    def nUtterances(self):
        return self._n_utt

    @nUtterances.setter
    def nUtterances(self, n):      # (every set call assigns it: the lengths cached for pcmTensor belong to the batch before)
        self._n_utt, self._lens = n, None

    def _lengths(self):
        """Every utterance's sample count, in one call (speechPlayer_batch_lengths), kept until the next set call."""
        if self._lens is None:
            lens = np.zeros(max(self.nUtterances, 1), dtype=np.int64)
            n = self._check(self._dll.speechPlayer_batch_lengths(self._h, lens.ctypes.data, len(lens)))
            self._lens = lens[:n]
        return self._lens

    @property
    def device(self):
        """The HIP (= torch CUDA) device index the batch is bound to."""
        return self._check(self._dll.speechPlayer_batch_device(self._h))

    def setUtterancesTensor(self, frameStart, frames, minSamples, fadeSamples, userIndex=None, isNull=None, noiseSeed=None):
        """setUtterances with the frames in a torch tensor on the batch's device (speechPlayer_batch_setUtterancesDevice): `frames` a
        contiguous torch.float64 CUDA tensor [F, 47]; nothing is converted (check_frames_tensor says what is refused).  The engine copies
        it device to device behind the work queued so far on torch's current stream (the default stream too: the NULL stream, which the C
        entry reads as "ready now", is waited for by a stream of the player's own) -- no host synchronisation of it -- and the
        tensor may be freed or overwritten once the call returns.  The other arguments are numpy arrays, sequences or tensors; a CUDA
        tensor among them is copied to the host, which synchronises."""
        dev = self.device
        fs = check_frames_tensor(frames, frameStart, dev)
        m = _host_array(minSamples, np.uint32)
        f = _host_array(fadeSamples, np.uint32)
        n_frames = int(fs[-1])
        if len(m) != n_frames or len(f) != n_frames:
            raise ValueError("minSamples and fadeSamples need %d entries" % n_frames)
        ix = None if userIndex is None else _host_array(userIndex, np.int32)
        nu = None if isNull is None else _host_array(isNull, np.uint8)
        sd = None if noiseSeed is None else _host_array(noiseSeed, np.uint32)
        if (ix is not None and len(ix) != n_frames) or (nu is not None and len(nu) != n_frames) or (sd is not None and len(sd) != len(fs) - 1):
            raise ValueError("userIndex / isNull need %d entries, noiseSeed %d" % (n_frames, len(fs) - 1))
        p = lambda a: None if a is None else a.ctypes.data
        self._check(self._dll.speechPlayer_batch_setUtterancesDevice(self._h, len(fs) - 1, p(fs), frames.data_ptr() if n_frames else None,
                                                                     p(m), p(f), p(ix), p(nu), p(sd), _ready_stream(self, dev)))
        self.nUtterances = len(fs) - 1

    def pcmTensor(self, utterances=None, dtype=None, padded=True):
        """The PCM as a torch tensor on the batch's device (speechPlayer_batch_exportPcm), filled on torch's current stream behind the
        synthesis without a host wait: -> (pcm, lengths).  utterances: indices in any order, repeats allowed (None: all, in order);
        dtype torch.float32 (default: sample / 32767, as readFloat) or torch.int16.  padded: pcm is [n, longest], zero past each
        utterance's end, and lengths the n lengths; else pcm is the utterances back to back and lengths the n + 1 offsets (int64 CPU tensors)."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.int16):
            raise TypeError("pcmTensor: dtype must be torch.float32 or torch.int16, not %s" % dtype)
        src = self._rows("pcmTensor", None, utterances)

        def call(out, stride, numel, stream):
            return self._dll.speechPlayer_batch_exportPcm(self._h, _ptr(src.sel), src.n, out, 1 if dtype == torch.float32 else 0, stride, stream)
        return self._export_rows(src.lengths, (), dtype, padded, call)

    def timeline(self, u):
        """When utterance u's requests are dequeued (speechPlayer_batch_timeline): -> (firstSample int64 [n + 1], userIndex int32 [n]);
        request k takes effect on sample firstSample[k], firstSample[n] is the utterance's length."""
        n = self._check(self._dll.speechPlayer_batch_timeline(self._h, u, None, None, 0))
        first = np.zeros(n + 1, np.int64); ix = np.zeros(n, np.int32)
        self._check(self._dll.speechPlayer_batch_timeline(self._h, u, first.ctypes.data, ix.ctypes.data, n))
        return first, ix

    def marks(self, u):
        """The index marks of utterance u: -> (sample int64 [m], index int32 [m]) of the requests that carry one; getLastIndex answers
        index[i] once sample[i] + 1 samples have been produced."""
        first, ix = self.timeline(u)
        keep = ix != -1
        return first[:-1][keep], ix[keep]

    def trackTensor(self, columns, hop=1, phase=0, utterances=None, dtype=None, padded=True):
        """Per-sample parameter tracks and timelines as a torch tensor on the batch's device (speechPlayer_batch_exportTracks), filled on
        torch's current stream without a host wait and without a synthesis launch: -> (tracks, steps).  Step j of an utterance is its
        sample phase + j * hop; element [.., j, q] is column columns[q] of the frame the synthesiser used on that sample (columns by
        number or by name: FRAME_FIELDS, "mark" = getLastIndex after that sample, "frame" = the request in effect).  utterances:
        indices in any order, repeats allowed (None: all, in order); dtype torch.float32 (default) or torch.float64 (the values
        themselves).  padded: tracks is [n, most steps, len(columns)], zero past each utterance's end, and steps the n step counts;
        else tracks is [total steps, len(columns)] and steps the n + 1 offsets (int64 CPU tensors)."""
        import torch
        cols, hop, phase, fmt = check_track_request(columns, hop, phase, dtype)
        sel, n, steps = self._steps("trackTensor", utterances, hop, phase)

        def call(out, stride, numel, stream):
            return self._dll.speechPlayer_batch_exportTracks(self._h, _ptr(sel), n, cols.ctypes.data, len(cols), hop, phase, out, fmt, stride, stream)
        return self._export_rows(steps, (len(cols),), torch.float32 if fmt else torch.float64, padded, call)

    @property
    def hasLabels(self):
        """True when the batch carries phoneme labels: set by setIpa, setText or setRecords(..., labels=...); any other set call drops them."""
        return self._check(self._dll.speechPlayer_batch_hasLabels(self._h)) == 1

    def _rows(self, what, signal, utterances):
        """The RowSource an export reads: `utterances` of the batch's PCM pool, or (signal not None) rows of that signal on the batch's device."""
        if signal is None:
            return RowSource(what, "utterance", self.nUtterances, self._lengths, utterances)
        return RowSource.of_signal(what, signal, self.device, utterances)

    def _entry(self, name, src):
        """The entry point speechPlayer_batch_export<name> over `src`, the pool's or the signal's (...Of), taking what follows the selection."""
        fn = getattr(self._dll, "speechPlayer_batch_export" + name + src.suffix)
        return lambda *args: fn(self._h, *src.lead, _ptr(src.sel), src.n, *args)

    def _steps(self, what, utterances, hop, phase):
        """The selection and its rows' step counts: the samples phase + j * hop below each utterance's length."""
        src = self._rows(what, None, utterances)
        return src.sel, src.n, _step_counts(src.lengths, hop, phase)

    def _export_rows(self, counts, tail_shape, dtype, padded, call, always=False):
        """The output of an export of len(counts) rows of counts[i] entries of shape tail_shape: [n, most, ...] (padded) or [total, ...],
        filled by call(pointer, rowStride, elements, stream) on torch's current stream -- not made for an empty tensor unless `always`
        (then with a null pointer) -- which answers the elements written.  -> (out, counts or, packed, the n + 1 offsets: int64 CPU tensors).
        tests/test_gpu_far_offsets.py replaces this method on a player (into_guarded) to aim the exports at buffers of its own: a change
        of the signature is a change there."""
        import torch
        dev = self.device
        if padded:
            stride = int(counts.max()) if len(counts) else 0
            lead, second = (len(counts), stride), counts
        else:
            stride, second = 0, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            lead = (int(second[-1]),)
        out = torch.empty(lead + tuple(tail_shape), dtype=dtype, device="cuda:%d" % dev)
        if out.numel() or always:
            got = self._check(call(out.data_ptr() if out.numel() else None, stride, out.numel(), torch.cuda.current_stream(dev).cuda_stream))
            assert got == out.numel(), (got, out.numel())
        return out, torch.from_numpy(second)

    def alignmentTensor(self, columns, hop=1, phase=0, utterances=None, dtype=None, padded=True, pad=-1):
        """Framewise phoneme labels of a batch set from IPA text, as a torch tensor on the batch's device
        (speechPlayer_batch_exportAlignment), filled on torch's current stream without a host wait and without a synthesis launch:
        -> (labels, steps).  Step j of an utterance is its sample phase + j * hop; element [.., j, q] is column columns[q] (by number or
        by name, ALIGN_COLUMNS) of the frame in effect on that sample: "phoneme" (index into ipa.phonemeSymbols()), "stress", "flags"
        (ipa.LABEL_*), "unit", "textOffset", "frame" (as trackTensor's), "position" (samples since the unit began) and "remaining" (until
        the next begins).  utterances: indices in any order, repeats allowed (None: all); dtype torch.int64 (default) or torch.int32.
        padded: labels is [n, most steps, len(columns)], `pad` past each utterance's end, and steps the n step counts; else labels is
        [total steps, len(columns)] and steps the n + 1 offsets (int64 CPU tensors).  RuntimeError when the batch has no labels."""
        import torch
        cols, hop, phase, fmt = check_alignment_request(columns, hop, phase, dtype)
        sel, n, steps = self._steps("alignmentTensor", utterances, hop, phase)

        def call(out, stride, numel, stream):
            return self._dll.speechPlayer_batch_exportAlignment(self._h, _ptr(sel), n, cols.ctypes.data, len(cols), hop, phase, out, fmt, stride,
                                                                int(pad), numel, stream)
        return self._export_rows(steps, (len(cols),), torch.int32 if fmt else torch.int64, padded, call, always=not self.hasLabels)

    def unitCounts(self, utterances=None, by="unit"):
        """Units (by="frame": frames) of the chosen utterances (speechPlayer_batch_unitCounts): an int64 array."""
        if by not in ("unit", "frame"):
            raise ValueError("by must be 'unit' or 'frame', not %r" % (by,))
        src = self._rows("unitCounts", None, utterances)
        counts = np.zeros(max(src.n, 1), np.int64)
        self._check(self._dll.speechPlayer_batch_unitCounts(self._h, _ptr(src.sel), src.n, int(by == "frame"), counts.ctypes.data))
        return counts[:src.n]

    def unitTensor(self, hop=1, phase=0, utterances=None, by="unit", padded=True, pad=-1):
        """The segment table of a batch set from IPA text (speechPlayer_batch_exportUnits), an int64 torch tensor on the batch's device
        filled on torch's current stream: -> (units, counts).  One entry per text symbol of an utterance (by="unit": an inserted gap counts
        to the stop after it, an aspiration to the stop before it, silence is an entry of its own) or per frame (by="frame"), with the columns
        UNIT_COLUMNS: phoneme, flags (ORed over the unit; LABEL_GAP / LABEL_PUFF: it has one), textOffset, firstSample, samples, and firstStep,
        steps: the steps phase + j * hop inside the entry (a row's steps sum to alignmentTensor's step count: duration targets at that hop).
        padded: units is [n, most entries, 7], `pad` past each row's count, and counts the n counts; else [total entries, 7] and the n + 1 offsets."""
        import torch
        hop, phase = int(hop), int(phase)
        if hop < 1 or phase < 0:
            raise ValueError("unitTensor: hop must be at least 1 and phase not negative (%d, %d)" % (hop, phase))
        src = self._rows("unitTensor", None, utterances)

        def call(out, stride, numel, stream):
            return self._dll.speechPlayer_batch_exportUnits(self._h, _ptr(src.sel), src.n, hop, phase, int(by == "frame"), out, stride, int(pad), numel, stream)
        return self._export_rows(self.unitCounts(utterances, by), (len(UNIT_COLUMNS),), torch.int64, padded, call)

    def sourceTensor(self, columns, hop=1, phase=0, utterances=None, dtype=None, padded=True):
        """The glottal source as a torch tensor on the batch's device (speechPlayer_batch_exportSource), filled on torch's current stream
        without a host wait and without a synthesis launch: -> (source, steps).  Step j of an utterance is its sample phase + j * hop;
        element [.., j, q] is column columns[q] (by number or by name, SOURCE_COLUMNS) on that sample: "f0" (the fundamental after
        vibrato, Hz), "phase" (the glottal phase in [0, 1)), "vibratoPhase", "cycle" (glottal cycles begun so far), "open" (1 while the
        glottis is open) and "wave" (the glottal wave before noise) -- the values behind the PCM, not a re-derivation.  utterances,
        dtype and padded as trackTensor's: source is [n, most steps, len(columns)], zero past each utterance's end, and steps the n step
        counts; or [total steps, len(columns)] and the n + 1 offsets (int64 CPU tensors)."""
        import torch
        cols, hop, phase, fmt = check_source_request(columns, hop, phase, dtype)
        sel, n, steps = self._steps("sourceTensor", utterances, hop, phase)

        def call(out, stride, numel, stream):
            return self._dll.speechPlayer_batch_exportSource(self._h, _ptr(sel), n, cols.ctypes.data, len(cols), hop, phase, out, fmt, stride, stream)
        return self._export_rows(steps, (len(cols),), torch.float32 if fmt else torch.float64, padded, call)

    def responseTensor(self, frequencies, kinds=("cascade_db", "parallel_db"), hop=1, phase=0, utterances=None, dtype=None, padded=True, gain=False):
        """The vocal-tract frequency response (the spectral envelope) as a torch tensor on the batch's device
        (speechPlayer_batch_exportResponse), filled on torch's current stream without a host wait and without a synthesis launch:
        -> (response, steps).  Step j of an utterance is its sample phase + j * hop; element [.., j, q, k] is kind kinds[q] (by number or
        name, RESPONSE_KINDS: real part, imaginary part, magnitude or dB of the cascade or the parallel branch) of the filter network
        the synthesiser configured on that sample, at frequency k of `frequencies`: an int K (linspace(0, sampleRate / 2, K)) or Hz
        values (at most 4096).  gain: times preFormantGain * outputGain of the sample.  utterances, dtype and padded as trackTensor's:
        response is [n, most steps, len(kinds), K], zero past each utterance's end, and steps the n step counts; or
        [total steps, len(kinds), K] and the n + 1 offsets (int64 CPU tensors)."""
        import torch
        freqs, ks = check_response_request(frequencies, kinds, self.sampleRate)
        hop, phase, fmt = _check_hop_phase_dtype("responseTensor", hop, phase, dtype, *_float_types())
        sel, n, steps = self._steps("responseTensor", utterances, hop, phase)

        def call(out, stride, numel, stream):
            return self._dll.speechPlayer_batch_exportResponse(self._h, _ptr(sel), n, freqs.ctypes.data, len(freqs), ks.ctypes.data, len(ks),
                                                               1 if gain else 0, hop, phase, out, fmt, stride, stream)
        return self._export_rows(steps, (len(ks), len(freqs)), torch.float32 if fmt else torch.float64, padded, call)

    def spectrogramTensor(self, nFft=1024, hop=256, phase=0, window=None, bank=None, power=2, log=None, floor=1e-10, utterances=None, dtype=None,
                          padded=True, signal=None):
        """The STFT or band (mel) spectrogram of the batch's PCM as a torch tensor on the batch's device
        (speechPlayer_batch_exportSpectrogram), filled on torch's current stream behind the synthesis without a host wait:
        -> (spectrogram, steps).  Step j of an utterance is centred on its sample phase + j * hop -- the grid of trackTensor, row for row
        -- with zeros outside the utterance; element [.., j, b] is band b of |X|^power: the nFft / 2 + 1 bins, or the rows of `bank`
        ([bands, nFft / 2 + 1], e.g. melFilterbank).  window: nFft values (None: periodic Hann).  log: None (linear), "db", "ln" or the
        factor of log10, applied to max(value, floor).  utterances, dtype and padded as trackTensor's: spectrogram is
        [n, most steps, bands], zero past each utterance's end, and steps the n step counts; or [total steps, bands] and the n + 1
        offsets (int64 CPU tensors).  The batch must have been synthesised since it was set; pcmSpectrogram is the same definition on
        the host.
        signal: the (tensor, lengths or offsets) pair another export returned (check_signal_request), read in place of the batch's PCM
        (speechPlayer_batch_exportSpectrogramOf): `utterances` then chooses rows of the signal, the steps are those of the signal's
        lengths, no synthesis is needed and signalSpectrogram is the host's statement.  The signal is read on torch's current stream."""
        import torch
        nFft, hop, phase, window, bank, bands, power, scale, floor, fmt = check_spectrogram_request(nFft, hop, phase, window, bank, power, log, floor, dtype)
        src = self._rows("spectrogramTensor", signal, utterances)
        export = self._entry("Spectrogram", src)

        def call(out, stride, numel, stream):
            return export(nFft, hop, phase, _ptr(window), _ptr(bank), bands if bank is not None else 0, power, scale, floor, out, fmt, stride, stream)
        return self._export_rows(_step_counts(src.lengths, hop, phase), (bands,), torch.float32 if fmt else torch.float64, padded, call)

    def resampledTensor(self, rate, zeros=6, rolloff=0.99, window="hann", beta=None, utterances=None, dtype=None, padded=True, signal=None,
                        signalRate=None):
        """The batch's PCM at `rate` Hz as a torch tensor on the batch's device (speechPlayer_batch_exportResampled), filled on torch's
        current stream behind the synthesis without a host wait: -> (pcm, lengths).  A polyphase windowed-sinc resampler: `zeros` zero
        crossings of the sinc either side, cut-off `rolloff` times the lower of the two Nyquist frequencies, window "hann" or "kaiser"
        (beta: None is 8.6).  Output sample m of an utterance lies at its source sample m * down / up; an utterance of L samples gives
        ceil(L * up / down).  utterances, padded and the (pcm, lengths) pair as pcmTensor's; dtype torch.float32 (default) or
        torch.int16 (clipped, rounded to nearest even).  rate == sampleRate gives pcmTensor's values.  The batch must have been
        synthesised since it was set; pcmResample is the same definition on the host.
        signal: the (tensor, lengths or offsets) pair another export returned (check_signal_request), read in place of the batch's PCM
        (speechPlayer_batch_exportResampledOf) at signalRate Hz (None: the batch's rate): `utterances` then chooses rows of the signal, no
        synthesis is needed, equal rates give the signal's samples and signalResample is the host's statement."""
        import torch
        if signal is None and signalRate is not None:
            raise ValueError("resampledTensor: signalRate comes with a signal")
        srcRate, rate, zeros, rolloff, win, beta, fmt, up, down, _ = check_resample_request(self.sampleRate if signalRate is None else signalRate, rate, zeros,
                                                                                            rolloff, window, beta, dtype)
        src = self._rows("resampledTensor", signal, utterances)
        export = self._entry("Resampled", src)
        rates = (rate,) if signal is None else (srcRate, rate)      # (the pool's rate is the batch's)

        def call(out, stride, numel, stream):
            return export(*rates, zeros, rolloff, win, beta, out, fmt, stride, stream)
        return self._export_rows((src.lengths * up + down - 1) // down, (), torch.float32 if fmt else torch.int16, padded, call)

    def convolvedTensor(self, irs, irOf=None, tail=True, utterances=None, dtype=None, padded=True, signal=None):
        """The batch's PCM convolved with impulse responses as a torch tensor on the batch's device
        (speechPlayer_batch_exportConvolved), filled on torch's current stream behind the synthesis without a host wait:
        -> (pcm, lengths).  irs: one 1-D array of float32 taps (a room, a channel, a microphone) or a list of them; irOf: the response of
        each ROW (None: the one response) -- with repeats in `utterances`, one utterance goes through several rooms in one call.  tail:
        a row of L samples and K taps gives L + K - 1 values (the full convolution) or, tail=False, the first L, on the grid of the
        other exports.  utterances, padded and the (pcm, lengths) pair as pcmTensor's; dtype torch.float32 (default) or torch.int16
        (clipped, rounded to nearest even).  The batch must have been synthesised since it was set; pcmConvolve is the same definition
        on the host, which the device equals bit for bit.
        signal: the (tensor, lengths or offsets) pair another export returned (check_signal_request), read in place of the batch's PCM
        (speechPlayer_batch_exportConvolvedOf): `utterances` then chooses rows of the signal, irOf stays per output row, no synthesis is
        needed and signalConvolve is the host's statement."""
        import torch
        src = self._rows("convolvedTensor", signal, utterances)
        export = self._entry("Convolved", src)
        h, start, of, tail, fmt = check_convolve_request(irs, irOf, src.n, tail, dtype)
        taps = np.diff(start)[of if of is not None else np.zeros(src.n, np.int64)]

        def call(out, stride, numel, stream):
            return export(h.ctypes.data, start.ctypes.data, len(start) - 1, _ptr(of), tail, out, fmt, stride, stream)
        return self._export_rows(src.lengths + (taps - 1 if tail else 0), (), torch.float32 if fmt else torch.int16, padded, call)

    def filteredTensor(self, filters, filterOf=None, tail=0, utterances=None, dtype=None, padded=True, signal=None):
        """The batch's PCM through cascades of biquad (IIR) sections as a torch tensor on the batch's device
        (speechPlayer_batch_exportFiltered), filled on torch's current stream behind the synthesis without a host wait:
        -> (pcm, lengths).  filters: one array of shape [K, 5] (b0 b1 b2 a1 a2) or [K, 6] (scipy's sos layout: divided by a0 in binary64,
        then rounded to float32 once) or a list of them, 1 .. 16 sections each -- biquad, preEmphasis, dcBlock and resonatorSections
        design them; filterOf: the filter of each ROW (None: the one filter) -- with repeats in `utterances`, one utterance goes through
        several filters in one call.  tail: extra outputs of zero input, the same for every row (0: the grid of the other exports).
        utterances, padded and the (pcm, lengths) pair as pcmTensor's; dtype torch.float32 (default) or torch.int16 (clipped, rounded to
        nearest even).  The batch must have been synthesised since it was set; pcmFilter is the same definition on the host, which the
        device equals bit for bit.  The result feeds the next stage as its signal=.
        signal: the (tensor, lengths or offsets) pair another export returned (check_signal_request), read in place of the batch's PCM
        (speechPlayer_batch_exportFilteredOf): `utterances` then chooses rows of the signal, filterOf stays per output row, no synthesis
        is needed and signalFilter is the host's statement."""
        import torch
        src = self._rows("filteredTensor", signal, utterances)
        export = self._entry("Filtered", src)
        sec, start, of, tail, fmt = check_filter_request(filters, filterOf, src.n, tail, dtype)

        def call(out, stride, numel, stream):
            return export(sec.ctypes.data, start.ctypes.data, len(start) - 1, _ptr(of), tail, out, fmt, stride, stream)
        return self._export_rows(src.lengths + tail, (), torch.float32 if fmt else torch.int16, padded, call)

    def codedTensor(self, codec, codes=False, decoded=True, utterances=None, dtype=None, padded=True, signal=None):
        """The batch's PCM through a speech codec as torch tensors on the batch's device (speechPlayer_batch_exportCoded), filled on
        torch's current stream behind the synthesis without a host wait: codec "ulaw" or "alaw" (G.711) or "adpcm" (IMA/DVI, 4 bits a
        sample; CODECS).  -> (decoded, lengths), (decoded, codes, lengths) or (codes, lengths): decoded is what a decoder makes of the
        codes, dtype torch.int16 (default: a codec's output is integer) or torch.float32 (sample / 32767); codes a torch.uint8 tensor of
        the same layout, one code per sample (0 .. 255 for G.711 -- the mu-law code is the class label vocoders train on --, 0 .. 15
        for ADPCM; nibble packing is the caller's).  Row lengths are unchanged.  utterances, padded and the lengths as pcmTensor's: +0
        and code 0 past each row's end.  The batch must have been synthesised since it was set; pcmCode is the same definition on the
        host, which the device equals bit for bit.  (decoded, lengths) feeds the next stage as its signal=.
        signal: the (tensor, lengths or offsets) pair another export returned (check_signal_request), read in place of the batch's PCM
        (speechPlayer_batch_exportCodedOf): `utterances` then chooses rows of the signal, no synthesis is needed and signalCode is the
        host's statement."""
        import torch
        codec, codes, decoded, fmt = check_codec_request(codec, codes, decoded, dtype)
        src = self._rows("codedTensor", signal, utterances)
        export = self._entry("Coded", src)
        lengths = src.lengths
        # two outputs of one layout (_export_rows makes one): [n, most] (padded) or [total]
        if padded:
            stride = int(lengths.max()) if len(lengths) else 0
            shape, second = (len(lengths), stride), lengths
        else:
            stride, second = 0, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
            shape = (int(second[-1]),)
        dev = "cuda:%d" % self.device
        d = torch.empty(shape, dtype=torch.float32 if fmt else torch.int16, device=dev) if decoded else None
        c = torch.empty(shape, dtype=torch.uint8, device=dev) if codes else None
        numel = int(np.prod(shape))
        if numel:
            got = self._check(export(codec, d.data_ptr() if decoded else None, fmt, c.data_ptr() if codes else None, stride,
                                     torch.cuda.current_stream(self.device).cuda_stream))
            assert got == numel, (got, numel)
        return tuple(t for t in (d, c) if t is not None) + (torch.from_numpy(second),)

    def lpcTensor(self, order=16, nWin=512, hop=256, phase=0, window=None, lagWindow=None, fields=("lpc", "error"), utterances=None, dtype=None,
                  padded=True, signal=None):
        """The linear-prediction analysis of the batch's PCM as a torch tensor on the batch's device (speechPlayer_batch_exportLpc), filled
        on torch's current stream behind the synthesis without a host wait: -> (lpc, steps).  Step j of an utterance is centred on its
        sample phase + j * hop -- the grid of spectrogramTensor and trackTensor, row for row -- over a frame of nWin samples (any
        integer in order + 1 .. 4096), zeros outside the utterance.  window: nWin values (None: periodic Hann); lagWindow: order + 1
        values that multiply the autocorrelation (None: none; lagWindow() designs one).  fields: names of LPC_FIELDS; a step's values
        come in that list's order whatever the order asked for (lpcColumns): "autocorr" r[0 .. order], "lpc" a_1 .. a_order of
        A(z) = 1 + sum a_j z^-j, "reflection" k_1 .. k_order, "error" E, "stages" the stages of the recursion that ran (order, unless the
        frame is silent or not positive definite: the later values are +0).  utterances, dtype and padded as spectrogramTensor's.
        The batch must have been synthesised since it was set; pcmLpc is the same definition on the host, which the device equals bit
        for bit.
        signal: the (tensor, lengths or offsets) pair another export returned (check_signal_request), read in place of the batch's PCM
        (speechPlayer_batch_exportLpcOf): `utterances` then chooses rows of the signal, no synthesis is needed and signalLpc is the
        host's statement."""
        import torch
        order, nWin, hop, phase, window, lagWindow, bits, cols, fmt = check_lpc_request(order, nWin, hop, phase, window, lagWindow, fields, dtype)
        src = self._rows("lpcTensor", signal, utterances)
        export = self._entry("Lpc", src)

        def call(out, stride, numel, stream):
            return export(order, nWin, hop, phase, _ptr(window), _ptr(lagWindow), bits, out, fmt, stride, stream)
        return self._export_rows(_step_counts(src.lengths, hop, phase), (cols,), torch.float32 if fmt else torch.float64, padded, call)

    def pitchTensor(self, fmin=60.0, fmax=500.0, nWin=1024, hop=256, phase=0, threshold=0.1, fields=("f0", "aperiodicity"), utterances=None, dtype=None,
                    padded=True, signal=None, sampleRate=None, lagMin=None, lagMax=None):
        """The pitch of the batch's PCM ESTIMATED FROM THE SIGNAL (YIN) as a torch tensor on the batch's device
        (speechPlayer_batch_exportPitch), filled on torch's current stream behind the synthesis without a host wait: -> (pitch, steps).
        Step j of an utterance is centred on its sample phase + j * hop -- the grid of spectrogramTensor and lpcTensor, row for row -- over
        a frame of nWin + lagMax samples (nWin any integer in 32 .. 2048), zeros outside the utterance.  The lags searched are
        pitchLags(sampleRate, fmin, fmax), or lagMin= and lagMax= (2 <= lagMin < lagMax <= 1024); threshold in 0 .. 1 is YIN's.  fields:
        names of PITCH_FIELDS; a step's values come in that list's order whatever the order asked for (pitchColumns): "f0" in Hz, +0 where
        unvoiced; "period" in samples, refined by a parabola; "lag" the integer lag chosen; "aperiodicity" the normalised difference
        there; "voiced" 0 or 1; "cmnd" the whole normalised difference over lagMin .. lagMax for a tracker of the caller's own.  sourceTensor
        gives the TRUE fundamental of the clean synthesis; this is what a front end would estimate from the row.  utterances, dtype and
        padded as lpcTensor's.  The batch must have been synthesised since it was set; pcmPitch is the same definition on the host,
        which the device equals bit for bit.
        signal: the (tensor, lengths or offsets) pair another export returned, read in place of the batch's PCM
        (speechPlayer_batch_exportPitchOf) at sampleRate=, which is then required (a signal has no rate of its own: resampledTensor's is
        the rate asked for); signalPitch is the host's statement."""
        import torch
        if signal is None and sampleRate is not None:
            raise ValueError("pitchTensor: sampleRate comes with a signal")
        if signal is not None and sampleRate is None:
            raise ValueError("pitchTensor: a signal needs its sampleRate")
        rate, nWin, lagMin, lagMax, threshold, hop, phase, bits, cols, fmt = check_pitch_request(int(self.sampleRate) if signal is None else sampleRate, fmin, fmax,
                                                                                                 lagMin, lagMax, nWin, hop, phase, threshold, fields, dtype)
        src = self._rows("pitchTensor", signal, utterances)
        export = self._entry("Pitch", src)

        def call(out, stride, numel, stream):
            return export(*(() if signal is None else (rate,)), nWin, lagMin, lagMax, threshold, hop, phase, bits, out, fmt, stride, stream)
        return self._export_rows(_step_counts(src.lengths, hop, phase), (cols,), torch.float32 if fmt else torch.float64, padded, call)

    def lpcResidualTensor(self, lpc, order=16, hop=256, phase=0, column=0, what="residual", utterances=None, dtype=None, padded=True, signal=None):
        """The batch's PCM through the inverse filter of its own frames' prediction coefficients as a torch tensor on the batch's device
        (speechPlayer_batch_exportLpcResidual): -> (pcm, lengths).  lpc: a torch.float64 or torch.float32 tensor on the batch's device,
        [n, most steps, values] (padded) or [total steps, values] (packed) for the rows chosen here and the same hop and phase -- what
        lpcTensor returned, or the caller's own coefficients --, a_1 .. a_order at columns column .. column + order - 1
        (lpcColumns(fields, order)["lpc"][0]); it is read on torch's current stream.  Sample t takes the coefficients of the nearest
        step's centre, ties upward.  what: "residual", e(t) = x(t) + sum a_m x(t - m), or "prediction", p(t) = -sum a_m x(t - m).
        utterances, padded and the (pcm, lengths) pair as pcmTensor's; dtype torch.float32 (default) or torch.int16 (clipped, rounded
        to nearest even).  pcmLpcResidual is the same definition on the host, which the device equals bit for bit.  The result feeds
        the next stage as its signal=.
        signal: as lpcTensor's (speechPlayer_batch_exportLpcResidualOf; signalLpcResidual is the host's statement)."""
        import torch
        order, hop, phase, column, which, fmt = check_lpc_residual_request(order, hop, phase, column, what, dtype)
        src = self._rows("lpcResidualTensor", signal, utterances)
        export = self._entry("LpcResidual", src)
        steps = _step_counts(src.lengths, hop, phase)
        if not isinstance(lpc, torch.Tensor) or lpc.dtype not in (torch.float32, torch.float64) or lpc.dim() not in (2, 3) or not lpc.is_contiguous():
            raise TypeError("lpcResidualTensor: the coefficients must be a contiguous torch.float32 or torch.float64 tensor, [rows, steps, values] or [steps, values]")
        if not lpc.is_cuda or lpc.device.index != self.device:
            raise ValueError("lpcResidualTensor: the coefficients must be on the batch's device, cuda:%d, not %s" % (self.device, lpc.device))
        cols = int(lpc.shape[-1])
        if column + order > cols:
            raise ValueError("lpcResidualTensor: a_1 .. a_%d at columns %d .. %d of %d" % (order, column, column + order - 1, cols))
        most = int(steps.max()) if len(steps) else 0
        if lpc.dim() == 3:
            if lpc.shape[0] != src.n or lpc.shape[1] < most:
                raise ValueError("lpcResidualTensor: coefficients %s for %d rows of at most %d steps" % (list(lpc.shape), src.n, most))
            cstride = int(lpc.shape[1])
            if cstride == 0:      # (no row has a step: nothing is read)
                cstride = 1
        else:
            if lpc.shape[0] < int(steps.sum()):
                raise ValueError("lpcResidualTensor: coefficients %s for %d steps" % (list(lpc.shape), int(steps.sum())))
            cstride = 0

        def call(out, stride, numel, stream):
            return export(order, hop, phase, lpc.data_ptr() if lpc.numel() else None, 1 if lpc.dtype == torch.float32 else 0, cols, column, cstride, which, out, fmt,
                          stride, stream)
        return self._export_rows(src.lengths, (), torch.float32 if fmt else torch.int16, padded, call)

    def lpcSynthesisTensor(self, lpc, order=16, hop=256, phase=0, column=0, utterances=None, dtype=None, padded=True, signal=None):
        """The batch's PCM, taken as an excitation, through the recursive filter 1 / A(z) of its frames' prediction coefficients as a
        torch tensor on the batch's device (speechPlayer_batch_exportLpcSynthesis): -> (pcm, lengths).  lpc, order, hop, phase and column
        as lpcResidualTensor's: the coefficients lpcTensor returned for the same rows, or the caller's own (lpcBandwidthExpand,
        lpcFromReflection of quantised reflection coefficients, another row's).  y(t) = e(t) - sum a_m y(t - m) from y(t) = +0 for
        t < 0, one binary64 fma chain per sample; the history is the float32 y.  utterances, padded and the (pcm, lengths) pair as
        pcmTensor's; dtype torch.float32 (default) or torch.int16 (clipped, rounded to nearest even).  pcmLpcSynthesis is the same
        definition on the host, which the device equals bit for bit while the row's values are finite; unstable coefficients are not
        refused.  The usual excitation is a signal: lpcResidualTensor's result, changed or not.
        signal: as lpcTensor's (speechPlayer_batch_exportLpcSynthesisOf; signalLpcSynthesis is the host's statement)."""
        import torch
        order, hop, phase, column, fmt = check_lpc_synthesis_request(order, hop, phase, column, dtype)
        src = self._rows("lpcSynthesisTensor", signal, utterances)
        export = self._entry("LpcSynthesis", src)
        steps = _step_counts(src.lengths, hop, phase)
        if not isinstance(lpc, torch.Tensor) or lpc.dtype not in (torch.float32, torch.float64) or lpc.dim() not in (2, 3) or not lpc.is_contiguous():
            raise TypeError("lpcSynthesisTensor: the coefficients must be a contiguous torch.float32 or torch.float64 tensor, [rows, steps, values] or [steps, values]")
        if not lpc.is_cuda or lpc.device.index != self.device:
            raise ValueError("lpcSynthesisTensor: the coefficients must be on the batch's device, cuda:%d, not %s" % (self.device, lpc.device))
        cols = int(lpc.shape[-1])
        if column + order > cols:
            raise ValueError("lpcSynthesisTensor: a_1 .. a_%d at columns %d .. %d of %d" % (order, column, column + order - 1, cols))
        most = int(steps.max()) if len(steps) else 0
        if lpc.dim() == 3:
            if lpc.shape[0] != src.n or lpc.shape[1] < most:
                raise ValueError("lpcSynthesisTensor: coefficients %s for %d rows of at most %d steps" % (list(lpc.shape), src.n, most))
            cstride = int(lpc.shape[1])
            if cstride == 0:      # (no row has a step: nothing is read)
                cstride = 1
        else:
            if lpc.shape[0] < int(steps.sum()):
                raise ValueError("lpcSynthesisTensor: coefficients %s for %d steps" % (list(lpc.shape), int(steps.sum())))
            cstride = 0

        def call(out, stride, numel, stream):
            return export(order, hop, phase, lpc.data_ptr() if lpc.numel() else None, 1 if lpc.dtype == torch.float32 else 0, cols, column, cstride, out, fmt,
                          stride, stream)
        return self._export_rows(src.lengths, (), torch.float32 if fmt else torch.int16, padded, call)

    def _tempo_rows(self, what, tempo, nWin, search, dtype, signal, utterances):
        """What the tempo exports share: the row source, the rows' tempos, output lengths and frame counts."""
        src = self._rows(what, signal, utterances)
        tempo, nWin, search, fmt = check_tempo_request(tempo, nWin, search, dtype, src.n, what)
        outLens = _tempo_lengths(src.lengths, tempo) if src.n else np.zeros(0, np.int64)
        return src, tempo, nWin, search, fmt, outLens, _tempo_frames(outLens, nWin)

    def tempoPositionsTensor(self, tempo, nWin=512, search=160, utterances=None, padded=True, signal=None):
        """The time map of the batch's PCM at another tempo as a torch.int64 tensor on the batch's device
        (speechPlayer_batch_exportTempoPositions), filled on torch's current stream behind the synthesis without a host wait:
        -> (positions, counts).  Row i has K = tempoFrames(length, tempo, nWin) positions: positions[k] is the input sample that lies at
        output sample k * nWin / 2 (pcmTempo says how it is chosen; tempoMap gives the map per sample).  tempo: a number, or one per ROW
        -- with repeats in `utterances` one utterance comes at several tempos.  padded: [n, most frames], 0 past a row's count, and the
        n counts; else [total frames] and the n + 1 offsets (int64 CPU tensors).  The batch must have been synthesised since it was set.
        signal: the (tensor, lengths or offsets) pair another export returned, read in place of the batch's PCM
        (speechPlayer_batch_exportTempoPositionsOf): `utterances` then chooses rows of the signal and no synthesis is needed."""
        import torch
        src, tempo, nWin, search, _, _, frames = self._tempo_rows("tempoPositionsTensor", tempo, nWin, search, None, signal, utterances)
        export = self._entry("TempoPositions", src)

        def call(out, stride, numel, stream):
            return export(tempo.ctypes.data, nWin, search, out, stride, stream)
        return self._export_rows(frames, (), torch.int64, padded, call)

    def tempoTensor(self, tempo, nWin=512, search=160, positions=None, utterances=None, dtype=None, padded=True, signal=None, returnPositions=False):
        """The batch's PCM at another tempo by WSOLA as a torch tensor on the batch's device (speechPlayer_batch_exportTempo), filled on
        torch's current stream behind the synthesis without a host wait: -> (pcm, lengths), with returnPositions (pcm, lengths, positions,
        counts).  A row of L samples gives ceil(L / tempo): a tempo above 1 is faster speech, and the pitch and the formants stay where
        they are (resampledTensor moves them; this export followed by it shifts the pitch alone).  tempo, nWin, search and the positions
        as tempoPositionsTensor's, which runs first when `positions` is None; else positions is a contiguous torch.int64 tensor on the
        batch's device, [n, at least the most frames] or [total frames], of any values: the caller's own time map.  utterances, padded
        and the (pcm, lengths) pair as pcmTensor's; dtype torch.float32 (default) or torch.int16 (clipped, rounded to nearest even).
        pcmTempo is the same definition on the host, which the device equals bit for bit.  (pcm, lengths) feeds the next stage as its
        signal=.
        signal: as tempoPositionsTensor's (speechPlayer_batch_exportTempoOf; signalTempo is the host's statement)."""
        import torch
        src, tempo, nWin, search, fmt, outLens, frames = self._tempo_rows("tempoTensor", tempo, nWin, search, dtype, signal, utterances)
        counts = None
        if positions is None:
            positions, counts = self.tempoPositionsTensor(tempo, nWin, search, utterances, padded, signal)
        if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int64 or positions.dim() not in (1, 2) or not positions.is_contiguous():
            raise TypeError("tempoTensor: the positions must be a contiguous torch.int64 tensor, [rows, frames] or [frames]")
        if not positions.is_cuda or positions.device.index != self.device:
            raise ValueError("tempoTensor: the positions must be on the batch's device, cuda:%d, not %s" % (self.device, positions.device))
        most = int(frames.max()) if len(frames) else 0
        if positions.dim() == 2:
            if positions.shape[0] != src.n or positions.shape[1] < most:
                raise ValueError("tempoTensor: positions %s for %d rows of at most %d frames" % (list(positions.shape), src.n, most))
            pstride = max(int(positions.shape[1]), 1)      # (0: no row has a frame, nothing is read)
        else:
            if positions.shape[0] < int(frames.sum()):
                raise ValueError("tempoTensor: positions %s for %d frames" % (list(positions.shape), int(frames.sum())))
            pstride = 0
        export = self._entry("Tempo", src)

        def call(out, stride, numel, stream):
            return export(tempo.ctypes.data, nWin, positions.data_ptr() if positions.numel() else None, pstride, out, fmt, stride, stream)
        y, lengths = self._export_rows(outLens, (), torch.float32 if fmt else torch.int16, padded, call)
        if not returnPositions:
            return y, lengths
        if counts is None:
            counts = torch.from_numpy(frames if positions.dim() == 2 else np.concatenate([[0], np.cumsum(frames)]).astype(np.int64))
        return y, lengths, positions, counts

    def setNoiseBank(self, clips):
        """The batch's noise bank (speechPlayer_batch_setNoiseBank): a list of one-dimensional float arrays (kept as float32), every value
        finite and at most 2^16 in magnitude; None or an empty list frees it.  The bank stays on the device across set calls and
        synthesis launches until it is replaced; replacing it waits for the exports that still read the old one."""
        if clips is None:
            clips = []
        if isinstance(clips, np.ndarray) and clips.ndim == 1 and clips.dtype != object:
            clips = [clips]
        if not isinstance(clips, (list, tuple)):
            raise TypeError("setNoiseBank: clips must be a list of one-dimensional float arrays, not %s" % type(clips).__name__)
        held = [_mix_clip(c, "setNoiseBank", "clip %d" % k) for k, c in enumerate(clips)]
        start = np.concatenate([[0], np.cumsum([len(c) for c in held])]).astype(np.int64)
        flat = np.ascontiguousarray(np.concatenate(held)) if held else np.zeros(1, np.float32)
        self._check(self._dll.speechPlayer_batch_setNoiseBank(self._h, flat.ctypes.data if held else None, start.ctypes.data if held else None, len(held)))

    def noiseBankPowers(self):
        """The whole-clip mean squares P_c of the noise bank's clips (speechPlayer_batch_noiseBank): a float64 array, empty without a bank."""
        n = self._check(self._dll.speechPlayer_batch_noiseBank(self._h, None, None, 0))
        power = np.zeros(max(n, 1), np.float64)
        self._check(self._dll.speechPlayer_batch_noiseBank(self._h, power.ctypes.data, None, n))
        return power[:n]

    def powerTensor(self, utterances=None, signal=None):
        """The exact sums of squares S_u = sum s(n)^2 of the chosen utterances' int16 PCM (speechPlayer_batch_exportPower), filled on torch's
        current stream behind the synthesis without a host wait: -> (sums, lengths), int64 tensors [n] on the batch's device.  The mean
        square on the sample / 32767 scale is sums / lengths / 32767^2: the number every SNR starts from.
        signal: the (tensor, lengths or offsets) pair another export returned (check_signal_request), read in place of the batch's PCM
        (speechPlayer_batch_exportPowerOf): `utterances` then chooses rows of the signal and the result is (powers, lengths), the
        float64 mean squares themselves -- of a wet signal, say --, which signalPower states on the host; no synthesis is needed."""
        import torch
        src = self._rows("powerTensor", signal, utterances)
        dev = self.device
        out = torch.zeros(src.n, dtype=torch.int64 if signal is None else torch.float64, device="cuda:%d" % dev)      # (sums, or powers)
        if src.n:
            got = self._check(self._entry("Power", src)(out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            assert got == src.n, (got, src.n)
        return out, torch.from_numpy(src.lengths).to("cuda:%d" % dev)

    def mixedTensor(self, terms, speechGain=None, utterances=None, dtype=None, padded=True, gains=False, signal=None):
        """The batch's PCM mixed with noise clips and other utterances as a torch tensor on the batch's device
        (speechPlayer_batch_exportMixed), filled on torch's current stream behind the synthesis without a host wait: -> (mixed, lengths).
        terms: one list of MixTerm per ROW (an empty list: the speech alone) -- with repeats in `utterances`, one utterance gets several
        mixtures in one call -- or, for large batches, a pair (array of mixTermDtype, termStart).  MixTerm(noise=k) names clip k of the
        bank (setNoiseBank), MixTerm(utterance=u) an utterance of the batch; snr= is in dB against the row's whole-utterance mean square,
        gain= linear.  speechGain: None (1), one number or one per row.  A row keeps its length; utterances, padded and the
        (mixed, lengths) pair as pcmTensor's; dtype torch.float32 (default) or torch.int16 (clipped, rounded to nearest even).
        gains=True: -> (mixed, lengths, the float32 gains applied: a device tensor, one per term, termStart: an int64 CPU tensor).  The
        batch must have been synthesised since it was set; pcmMix is the same definition on the host, which the device equals bit for bit.
        signal: the (tensor, lengths or offsets) pair another export returned (check_signal_request), mixed onto in place of the batch's
        PCM (speechPlayer_batch_exportMixedOf) -- the speech after a room, say, so that an SNR is measured against the reverberant
        speech: `utterances` then chooses rows of the signal, MixTerm(utterance=k) means row k of the signal (any row, the row's own
        included), an SNR is against the row's signalPower, no synthesis is needed and signalMix is the host's statement."""
        import torch
        dev = self.device
        src = self._rows("mixedTensor", signal, utterances)
        export = self._entry("Mixed", src)
        flat, start, sg, fmt = check_mix_request(terms, src.n, speechGain, dtype, signalRows=None if signal is None else src.count)
        applied = torch.zeros(len(flat), dtype=torch.float32, device="cuda:%d" % dev) if gains else None

        def call(out, stride, numel, stream):
            return export(flat.ctypes.data if len(flat) else None, start.ctypes.data, _ptr(sg), applied.data_ptr() if gains and len(flat) else None, out, fmt,
                          stride, stream)
        # (always: the library refuses a bad term even where the chosen rows have no samples to write)
        out, second = self._export_rows(src.lengths, (), torch.float32 if fmt else torch.int16, padded, call, always=True)
        return (out, second, applied, torch.from_numpy(start)) if gains else (out, second)

    def stemTensor(self, columns, utterances=None, dtype=None, padded=True):
        """The signal stems as a torch tensor on the batch's device (speechPlayer_batch_exportStems), filled on torch's current stream
        without a host wait and without a synthesis launch: -> (stems, lengths).  columns by number or by name (STEM_COLUMNS): "voice"
        (the glottal wave with its turbulence), "aspiration", "source" (their sum: the excitation of the cascade), "frication" (the
        excitation of the parallel bank), "cascade" and "parallel" (the outputs of the two filter branches) and "output" (the mixed sample
        before it is clipped and truncated: int16 PCM is trunc(clip(output))) -- the values behind the MODE_EXACT PCM, whatever the batch's
        mode.  utterances: indices in any order, repeats allowed (None: all, in order); dtype torch.float32 (default) or torch.float64
        (the values themselves).  padded: stems is [n, len(columns), longest], zero past each utterance's end, and lengths the n
        lengths; else stems is flat, row i holding its columns one after the other, each of its utterance's length, and lengths the
        n + 1 element offsets (int64 CPU tensors)."""
        import torch
        cols, fmt = check_stem_request(columns, dtype)
        src = self._rows("stemTensor", None, utterances)
        n, lens = src.n, src.lengths
        dev = self.device
        tdtype = torch.float32 if fmt else torch.float64
        if padded:
            width = int(lens.max()) if n else 0
            out = torch.empty((n, len(cols), width), dtype=tdtype, device="cuda:%d" % dev)
            stride = width
        else:
            offsets = np.concatenate([[0], np.cumsum(lens * len(cols))]).astype(np.int64)
            out = torch.empty(int(offsets[-1]), dtype=tdtype, device="cuda:%d" % dev)
            stride = 0
        if out.numel():
            got = self._check(self._entry("Stems", src)(cols.ctypes.data, len(cols), out.data_ptr(), fmt, stride, torch.cuda.current_stream(dev).cuda_stream))
            assert got == out.numel(), (got, out.numel())
        return out, torch.from_numpy(lens if padded else offsets)

    def epochCounts(self, utterances=None):
        """Glottal cycles begun (pitch marks) in each of the chosen utterances (speechPlayer_batch_epochCounts): an int64 array.  The first
        call after a set call waits for a counting walk on the device."""
        src = self._rows("epochCounts", None, utterances)
        sel, n = src.sel, src.n
        if n == 0:
            return np.zeros(0, np.int64)
        counts = np.zeros(n, np.int64)
        self._check(self._dll.speechPlayer_batch_epochCounts(self._h, _ptr(sel), n, counts.ctypes.data))
        return counts[:n]

    def epochTensor(self, utterances=None, padded=True, pad=-1.0):
        """The pitch marks of the chosen utterances (speechPlayer_batch_exportEpochs), a float64 torch tensor on the batch's device filled on
        torch's current stream: -> (epochs, counts).  One entry per sample on which the glottal phase wraps, in time order, with the columns
        EPOCH_COLUMNS: sample, instant (the sub-sample time of the wrap), f0 and gain (voiceAmplitude * preFormantGain: zero means the
        cycle is inaudible).  padded: epochs is [n, most entries, 4], `pad` past each row's count, and counts the n counts; else
        [total entries, 4] and the n + 1 offsets (int64 CPU tensors).  The first call after a set call is not free of host waits: the
        counts come from a walk over EVERY list of the batch on the engine's own stream (however few utterances are chosen), which
        queues behind a synthesize(wait=False) in flight and is waited for on the host; later calls are ordered by events alone."""
        import torch
        src = self._rows("epochTensor", None, utterances)

        def call(out, stride, numel, stream):
            return self._dll.speechPlayer_batch_exportEpochs(self._h, _ptr(src.sel), src.n, out, stride, float(pad), numel, stream)
        return self._export_rows(self.epochCounts(utterances), (len(EPOCH_COLUMNS),), torch.float64, padded, call)

    def setUtterancesShared(self, listStart, frames, minSamples, fadeSamples, listOf, userIndex=None, isNull=None, noiseSeed=None):
        """Frame lists that utterances share (speechPlayer_batch_setUtterancesShared): `listStart`/frames/... describe the lists as
        setUtterances describes utterances; utterance u speaks list listOf[u] with noise seed noiseSeed[u]."""
        ls = np.ascontiguousarray(listStart, dtype=np.int64)
        fr = np.ascontiguousarray(frames, dtype=np.float64).reshape(-1, 47)
        m = np.ascontiguousarray(minSamples, dtype=np.uint32)
        f = np.ascontiguousarray(fadeSamples, dtype=np.uint32)
        lo = np.ascontiguousarray(listOf, dtype=np.uint32)
        assert ls[-1] == len(fr) == len(m) == len(f)
        ix = None if userIndex is None else np.ascontiguousarray(userIndex, dtype=np.int32)
        nu = None if isNull is None else np.ascontiguousarray(isNull, dtype=np.uint8)
        sd = None if noiseSeed is None else np.ascontiguousarray(noiseSeed, dtype=np.uint32)
        p = lambda a: None if a is None else a.ctypes.data
        self._check(self._dll.speechPlayer_batch_setUtterancesShared(self._h, len(ls) - 1, p(ls), p(fr), p(m), p(f), p(ix), p(nu), len(lo), p(lo), p(sd)))
        self.nUtterances = len(lo)

    def setRecords(self, shapes, listStart, records, listOf=None, noiseSeed=None, labels=None):
        """The batch in compact form (speechPlayer_batch_setRecords): `shapes` [nShapes, 47] f64, `records` a structured array of
        nvspeechplayer_amd.ipa.RECORD_DTYPE (32 bytes per frame), lists and listOf as in setUtterancesShared (None: utterance u = list u).
        labels: a structured array of ipa.LABEL_DTYPE parallel to records (speechPlayer_batch_setRecordsLabelled): the batch then carries
        phoneme labels (alignmentTensor, unitTensor)."""
        from .ipa import LABEL_DTYPE, RECORD_DTYPE
        sh = np.ascontiguousarray(shapes, dtype=np.float64).reshape(-1, 47)
        ls = np.ascontiguousarray(listStart, dtype=np.int64)
        rc = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        assert ls[-1] == len(rc)
        lo = None if listOf is None else np.ascontiguousarray(listOf, dtype=np.uint32)
        n_utt = len(ls) - 1 if lo is None else len(lo)
        sd = None if noiseSeed is None else np.ascontiguousarray(noiseSeed, dtype=np.uint32)
        p = lambda a: None if a is None else a.ctypes.data
        if labels is None:
            self._check(self._dll.speechPlayer_batch_setRecords(self._h, len(sh), p(sh), len(ls) - 1, p(ls), p(rc), n_utt, p(lo), p(sd)))
        else:
            lb = np.ascontiguousarray(labels, dtype=LABEL_DTYPE)
            if len(lb) != len(rc):
                raise ValueError("setRecords: %d labels for %d records" % (len(lb), len(rc)))
            lb = lb if len(lb) else np.zeros(1, LABEL_DTYPE)
            self._check(self._dll.speechPlayer_batch_setRecordsLabelled(self._h, len(sh), p(sh), len(ls) - 1, p(ls), p(rc), p(lb), n_utt, p(lo), p(sd)))
        self.nUtterances = n_utt

    def frames(self, u):
        """The frames of utterance u as they are resident in HBM (speechPlayer_batch_frames): -> (frames[n, 47], min[n], fade[n], index[n], isnull[n])."""
        n = self._check(self._dll.speechPlayer_batch_frames(self._h, u, None, None, None, None, None, 0))
        fr = np.zeros((n, 47)); m = np.zeros(n, np.uint32); f = np.zeros(n, np.uint32); ix = np.zeros(n, np.int32); nu = np.zeros(n, np.uint8)
        if n:
            self._check(self._dll.speechPlayer_batch_frames(self._h, u, fr.ctypes.data, m.ctypes.data, f.ctypes.data, ix.ctypes.data, nu.ctypes.data, n))
        return fr, m, f, ix, nu

    def setIpa(self, texts, speed=1, basePitch=100, inflection=0.5, clauseType=None, noiseSeed=None, voice=None,
               trailing_silence_ms=150.0, textOf=None):
        """Text in, batch ready (speechPlayer_batch_setIpa / _setIpaVoices): every IPA string becomes one utterance through the native
        frame producer followed by 150 ms of silence, as reference test_speakIpa.py:24-27 queues them.  basePitch and
        clauseType may be sequences (one per utterance); voice: one of nvspeechplayer_amd.ipa.voices() (or a voice defined with
        ipa.defineVoice), or a sequence of voice INDICES, one per utterance (-1: none).  textOf: utterance u speaks texts[textOf[u]]
        (a batch that repeats few sentences hands them over once)."""
        from .ipa import _text_pointers
        ptrs, n, keep = _text_pointers(texts, textOf)
        pitch = np.ascontiguousarray(np.broadcast_to(np.asarray(basePitch, dtype=np.float64), (n,)))
        code = lambda c: 0 if not c else ord(c[0])
        clauses = bytes([code(clauseType)]) * n if (clauseType is None or isinstance(clauseType, str)) else bytes(code(c) for c in clauseType)
        sd = None if noiseSeed is None else np.ascontiguousarray(noiseSeed, dtype=np.uint32)
        tail = -1.0 if trailing_silence_ms is None else float(trailing_silence_ms)
        if voice is None or isinstance(voice, str):
            self._check(self._dll.speechPlayer_batch_setIpa(self._h, n, ptrs.ctypes.data, float(speed), pitch.ctypes.data, float(inflection), clauses + b"\0",
                                                            None if not voice else voice.encode("utf8"), tail, None if sd is None else sd.ctypes.data))
        else:
            vo = np.ascontiguousarray(np.broadcast_to(np.asarray(voice, dtype=np.int32), (n,)))
            self._check(self._dll.speechPlayer_batch_setIpaVoices(self._h, n, ptrs.ctypes.data, float(speed), pitch.ctypes.data, float(inflection), clauses + b"\0",
                                                                  vo.ctypes.data, tail, None if sd is None else sd.ctypes.data))
        del keep
        self.nUtterances = n

    def setText(self, texts, speed=1, basePitch=100, inflection=0.5, noiseSeed=None, voice=None, espeakVoice="en"):
        """Plain text in (speechPlayer_batch_setText): each text becomes one utterance the way the NVDA driver speaks it -- clauses
        through eSpeak NG's text-to-IPA, the frame producer per clause, the pause after the last clause.  Needs libespeak-ng at
        run time (nvspeechplayer_amd.ipa.textAvailable()); raises RuntimeError with the reason when it is not there."""
        import ctypes
        n = len(texts)
        enc = [t.encode("utf8") for t in texts]
        ptrs = (ctypes.c_char_p * max(n, 1))(*enc)
        pitch = np.ascontiguousarray(np.broadcast_to(np.asarray(basePitch, dtype=np.float64), (n,)))
        sd = None if noiseSeed is None else np.ascontiguousarray(noiseSeed, dtype=np.uint32)
        self._check(self._dll.speechPlayer_batch_setText(self._h, n, ptrs, None if not espeakVoice else espeakVoice.encode("utf8"), float(speed),
                                                         pitch.ctypes.data, float(inflection), None if not voice else voice.encode("utf8"),
                                                         None if sd is None else sd.ctypes.data))
        self.nUtterances = n

    @property
    def totalSamples(self):
        return self._dll.speechPlayer_batch_totalSamples(self._h)

    @property
    def totalFrames(self):
        return self._dll.speechPlayer_batch_totalFrames(self._h)

    def utteranceSamples(self, u):
        return self._dll.speechPlayer_batch_utteranceSamples(self._h, u)

    def synthesize(self, wait=True):
        self._check(self._dll.speechPlayer_batch_synthesize(self._h))
        if wait:
            self._check(self._dll.speechPlayer_batch_wait(self._h))

    def wait(self):
        self._check(self._dll.speechPlayer_batch_wait(self._h))

    def read(self, u):
        n = self.utteranceSamples(u)
        buf = np.zeros(max(n, 1), dtype=np.int16)
        got = self._check(self._dll.speechPlayer_batch_read(self._h, u, buf.ctypes.data, n))
        return buf[:got]

    def readFloat(self, u):
        """Utterance u as float32 in [-1, 1] (int16 / 32767, converted on the device)."""
        n = self.utteranceSamples(u)
        buf = np.zeros(max(n, 1), dtype=np.float32)
        got = self._check(self._dll.speechPlayer_batch_readFloat(self._h, u, buf.ctypes.data, n))
        return buf[:got]

    def writeWav(self, u, path):
        """Utterance u as a 16-bit mono WAV file at the batch's sample rate."""
        import wave
        pcm = self.read(u)
        with wave.open(path, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(self.sampleRate)
            w.writeframes(pcm.astype("<i2").tobytes())

    def readAll(self, out=None):
        """All utterances' PCM, concatenated, and the nUtterances + 1 start offsets.  `out`: an int16 array of at
        least totalSamples to fill instead of a new one (a reused buffer avoids the page faults of a fresh one)."""
        total = self.totalSamples
        if out is not None:
            if out.dtype != np.int16 or not out.flags["C_CONTIGUOUS"] or out.size < total:
                raise ValueError("readAll: out must be a contiguous int16 array of at least %d samples" % total)
            buf = out
        else:
            buf = np.empty(max(total, 1), dtype=np.int16)
        starts = np.zeros(self.nUtterances + 1, dtype=np.int64)
        got = self._check(self._dll.speechPlayer_batch_readAll(self._h, buf.ctypes.data, total, starts.ctypes.data))
        return buf[:got], starts

    def readAllAsync(self, out):
        """readAll without waiting (speechPlayer_batch_readAllAsync): `out` must be page-locked (nvspeechplayer_amd.host_array); the
        compaction and the copy are queued behind the synthesis and run beside whatever is launched next.  Returns (view of `out`, starts);
        the samples are there after readWait()."""
        total = self.totalSamples
        if out.dtype != np.int16 or not out.flags["C_CONTIGUOUS"] or out.size < total:
            raise ValueError("readAllAsync: out must be a contiguous int16 array of at least %d samples" % total)
        starts = np.zeros(self.nUtterances + 1, dtype=np.int64)
        got = self._check(self._dll.speechPlayer_batch_readAllAsync(self._h, out.ctypes.data, out.size, starts.ctypes.data))
        return out[:got], starts

    def readWait(self):
        self._check(self._dll.speechPlayer_batch_readWait(self._h))

    def digest(self, per_utterance=False):
        """Digest of the whole PCM pool, computed on the device (speechPlayer_batch_digest); with per_utterance also the
        array of per-utterance digests.  `pcm_digest` below is the same formula on a host array."""
        import ctypes
        whole = ctypes.c_ulonglong(0)
        per = np.zeros(max(self.nUtterances, 1), dtype=np.uint64) if per_utterance else None
        self._check(self._dll.speechPlayer_batch_digest(self._h, None if per is None else per.ctypes.data, ctypes.byref(whole)))
        return (int(whole.value), per[:self.nUtterances]) if per_utterance else int(whole.value)

    def getLastIndex(self, u):
        return self._dll.speechPlayer_batch_getLastIndex(self._h, u)

    def time(self, launches):
        ms = np.zeros(launches, dtype=np.float32)
        self._check(self._dll.speechPlayer_batch_time(self._h, launches, ms.ctypes.data))
        return ms

    def kernelInfo(self):
        info = np.zeros(27, dtype=np.int32)
        self._check(self._dll.speechPlayer_batch_kernelInfo(self._h, info.ctypes.data, len(info)))
        # (the last launch's wavefronts -- one per workgroup and stage of the tracked group -- that ran without a dead term, option "dead_terms")
        dead = dict(waves_without_parallel1=int(info[20]), waves_without_turbulence=int(info[21]), waves_without_aspiration=int(info[22]))
        # (... and by the utterances' second word of present terms: the source stage without turbulence and the nasal pair, the final stage without
        # parallel 5 / without parallel 5 and 6, the parallel stage without parallel 1..4)
        dead.update(stages_without_nasal=int(info[23]), stages_without_parallel5=int(info[24]), stages_without_parallel56=int(info[25]),
                    stages_without_parallel1to4=int(info[26]))
        return dict(vgprs=int(info[0]), lds_bytes=int(info[1]), wavefronts=int(info[2]), cus=int(info[3]),
                    workgroups_per_cu_by_lds=int(info[4]), scratch_bytes=int(info[5]),
                    stage_parallel_chunk=int(info[6]), noisy_group=bool(info[7]),
                    lane_pipelined=bool(info[8]), lane_pipelined_utterances=int(info[9]),
                    nasal_free=bool(info[10]), nasal_free_utterances=int(info[11]),
                    tracked_utterances=int(info[12]), tracks=int(info[13]), track_mbytes=int(info[14]), tracked=bool(info[15]),
                    direct_utterances=int(info[16]), direct=bool(info[17]), direct_mbytes=int(info[18]), **dead)

    def devicePcm(self):
        return self._dll.speechPlayer_batch_devicePcm(self._h)

    def deviceOffset(self, u):
        return self._dll.speechPlayer_batch_deviceOffset(self._h, u)

    def _stage(self, kind, nRows, handle, bands=None, columns=None):
        if not handle:
            raise RuntimeError("%s failed: %s" % (STAGE_MAKERS.get(kind, "%sStage" % kind), _native.last_error()))
        return SignalStage(self, kind, nRows, handle, bands, columns)

    def lpcStage(self, nRows, order=16, nWin=512, hop=256, phase=0, window=None, lagWindow=None, fields=("lpc", "error")):
        """A SignalStage of nRows rows that takes the linear-prediction analysis chunk by chunk (speechPlayer_batch_stageLpc): lpcTensor's
        arguments, with the last nWin - 1 samples of every row kept between pushes; a push emits the steps whose whole frame has come in
        (lpcEmitted), an ended row's the rest of the definition's.  Its output is not a signal: it ends a SignalChain."""
        _, nRows, (order, nWin, hop, phase, window, lagWindow, bits, cols, _) = check_stage_request("lpc", nRows, order, nWin, hop, phase, window, lagWindow, fields)
        return self._stage("lpc", nRows, self._dll.speechPlayer_batch_stageLpc(self._h, nRows, order, nWin, hop, phase, _ptr(window), _ptr(lagWindow), bits), columns=cols)

    def pitchStage(self, nRows, sampleRate, fmin=60.0, fmax=500.0, nWin=1024, hop=256, phase=0, threshold=0.1, fields=("f0", "aperiodicity"), lagMin=None, lagMax=None):
        """A SignalStage of nRows rows that estimates the pitch (YIN) chunk by chunk (speechPlayer_batch_stagePitch): pitchTensor's
        arguments for a signal at sampleRate, with the last nWin + lagMax - 1 samples of every row kept between pushes; a push emits the
        steps whose whole frame has come in (pitchEmitted), an ended row's the rest of the definition's.  It ends a SignalChain."""
        _, nRows, (sampleRate, nWin, lagMin, lagMax, threshold, hop, phase, bits, cols, _) = check_stage_request(
            "pitch", nRows, sampleRate, fmin, fmax, nWin, hop, phase, threshold, fields, lagMin, lagMax)
        return self._stage("pitch", nRows, self._dll.speechPlayer_batch_stagePitch(self._h, nRows, sampleRate, nWin, lagMin, lagMax, threshold, hop, phase, bits), columns=cols)

    def resampleStage(self, nRows, srcRate, rate, zeros=6, rolloff=0.99, window="hann", beta=None):
        """A SignalStage of nRows rows that resamples from srcRate to rate Hz chunk by chunk (speechPlayer_batch_stageResample):
        resampledTensor's resampler with the last 2 Z - 1 samples of every row kept between pushes.  The player need never be set."""
        _, nRows, plan = check_stage_request("resample", nRows, srcRate, rate, zeros, rolloff, window, beta)
        srcRate, rate, zeros, rolloff, win, beta = plan[:6]
        return self._stage("resample", nRows, self._dll.speechPlayer_batch_stageResample(self._h, nRows, srcRate, rate, zeros, rolloff, win, beta))

    def filterStage(self, nRows, filters, filterOf=None, tail=0):
        """A SignalStage of nRows rows through cascades of biquad sections chunk by chunk (speechPlayer_batch_stageFilter):
        filteredTensor's filters -- filterOf the filter of each row of the stage -- with every section's state kept between pushes; the
        push that ends a row emits `tail` more outputs of zero input."""
        _, nRows, (sec, start, of, tail, _) = check_stage_request("filter", nRows, filters, filterOf, tail)
        return self._stage("filter", nRows, self._dll.speechPlayer_batch_stageFilter(self._h, nRows, sec.ctypes.data, start.ctypes.data, len(start) - 1, _ptr(of), tail))

    def convolveStage(self, nRows, irs, irOf=None, tail=True):
        """A SignalStage of nRows rows through impulse responses chunk by chunk (speechPlayer_batch_stageConvolve): convolvedTensor's
        irs -- irOf the response of each row of the stage -- with the last taps - 1 samples of every row kept between pushes; a push
        emits as many samples as it takes, an ended row's its tail of taps - 1 more (tail=True)."""
        _, nRows, (h, start, of, tail, _) = check_stage_request("convolution", nRows, irs, irOf, tail)
        return self._stage("convolution", nRows, self._dll.speechPlayer_batch_stageConvolve(self._h, nRows, h.ctypes.data, start.ctypes.data, len(start) - 1, _ptr(of), tail))

    def spectrogramStage(self, nRows, nFft=1024, hop=256, phase=0, window=None, bank=None, power=2, log=None, floor=1e-10):
        """A SignalStage of nRows rows that takes the STFT or band (mel) spectrogram chunk by chunk
        (speechPlayer_batch_stageSpectrogram): spectrogramTensor's arguments, with the last nFft - 1 samples of every row kept between
        pushes; a push emits the steps whose whole frame has come in (spectrogramEmitted), an ended row's the rest of the definition's.
        Its output is not a signal: it ends a SignalChain."""
        _, nRows, (nFft, hop, phase, window, bank, bands, power, scale, floor, _) = check_stage_request("spectrogram", nRows, nFft, hop, phase, window, bank, power, log, floor)
        return self._stage("spectrogram", nRows, self._dll.speechPlayer_batch_stageSpectrogram(self._h, nRows, nFft, hop, phase, _ptr(window), _ptr(bank),
                                                                                             bands if bank is not None else 0, power, scale, floor), bands)

    def codeStage(self, nRows, codec):
        """A SignalStage of nRows rows through a codec chunk by chunk (speechPlayer_batch_stageCode): codedTensor's codecs, the ADPCM
        predictor and step index of every row kept between pushes."""
        _, nRows, (codec, _, _, _) = check_stage_request("code", nRows, codec)
        return self._stage("code", nRows, self._dll.speechPlayer_batch_stageCode(self._h, nRows, codec))

    def close(self):
        if getattr(self, "_h", None):
            self._dll.speechPlayer_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NodePlayer(object):
    """One batch over several GPUs of a node (speechPlayer_node_*): contiguous shards of near-equal sample count, one
    per device, synthesised side by side; no exchange between devices.  `devices`: HIP device per shard."""

    def __init__(self, sampleRate, devices, mode=0, layout=None):
        self.sampleRate = sampleRate
        self._dll = _native.load()
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        self._h = self._dll.speechPlayer_node_create(sampleRate, len(dev), dev.ctypes.data)
        if not self._h:
            raise RuntimeError("speechPlayer_node_create failed: %s" % _native.last_error())
        self._check(self._dll.speechPlayer_node_setOption(self._h, b"mode", mode))
        if layout is not None:
            self._check(self._dll.speechPlayer_node_setOption(self._h, b"layout", layout))
        self.nUtterances = 0
        self._lens = None

    def _check(self, rc):
        if rc is None or rc < 0:
            raise RuntimeError("speechPlayer node call failed: %s" % _native.last_error())
        return rc

    def setUtterances(self, frameStart, frames, minSamples, fadeSamples, userIndex=None, isNull=None, noiseSeed=None):
        fs = np.ascontiguousarray(frameStart, dtype=np.int64)
        fr = np.ascontiguousarray(frames, dtype=np.float64).reshape(-1, 47)
        m = np.ascontiguousarray(minSamples, dtype=np.uint32)
        f = np.ascontiguousarray(fadeSamples, dtype=np.uint32)
        assert fs[-1] == len(fr) == len(m) == len(f)
        ix = None if userIndex is None else np.ascontiguousarray(userIndex, dtype=np.int32)
        nu = None if isNull is None else np.ascontiguousarray(isNull, dtype=np.uint8)
        sd = None if noiseSeed is None else np.ascontiguousarray(noiseSeed, dtype=np.uint32)
        p = lambda a: None if a is None else a.ctypes.data
        self._check(self._dll.speechPlayer_node_setUtterances(self._h, len(fs) - 1, p(fs), p(fr), p(m), p(f), p(ix), p(nu), p(sd)))
        self.nUtterances = len(fs) - 1
        per = np.maximum(m.astype(np.int64), np.maximum(f.astype(np.int64), 1) + 1) + 1
        c = np.concatenate([[0], np.cumsum(per)])
        self._lens = c[fs[1:]] - c[fs[:-1]]

    def setIpa(self, texts, speed=1, basePitch=100, inflection=0.5, clauseType=None, noiseSeed=None, voice=None,
               trailing_silence_ms=150.0, textOf=None):
        """The node's batch from IPA text (speechPlayer_node_setIpa): arguments as BatchPlayer.setIpa; the producer's compact form goes to
        every shard, the deal decides which utterances each shard speaks."""
        from .ipa import _text_pointers, _clauses
        ptrs, n, keep = _text_pointers(texts, textOf)
        pitch = np.ascontiguousarray(np.broadcast_to(np.asarray(basePitch, dtype=np.float64), (n,)))
        sd = None if noiseSeed is None else np.ascontiguousarray(noiseSeed, dtype=np.uint32)
        by_name = voice is None or isinstance(voice, str)
        vo = None if by_name else np.ascontiguousarray(np.broadcast_to(np.asarray(voice, dtype=np.int32), (n,)))
        self._check(self._dll.speechPlayer_node_setIpa(self._h, int(self.sampleRate), n, ptrs.ctypes.data, float(speed), pitch.ctypes.data, float(inflection),
                                                       _clauses(clauseType, n), None if vo is None else vo.ctypes.data,
                                                       (voice.encode("utf8") if (by_name and voice) else None),
                                                       -1.0 if trailing_silence_ms is None else float(trailing_silence_ms), None if sd is None else sd.ctypes.data))
        del keep
        self.nUtterances = n
        self._lens = None

    def utteranceSamples(self, u):
        """Samples utterance u produces (from the shard that holds it)."""
        for d in range(self._dll.speechPlayer_node_devices(self._h)):
            mem = self.shardUtterances(d)
            at = np.flatnonzero(mem == u)
            if len(at):
                return self._dll.speechPlayer_batch_utteranceSamples(self._dll.speechPlayer_node_part(self._h, d), int(at[0]))
        raise RuntimeError("NodePlayer.utteranceSamples: utterance %d out of range" % u)

    @property
    def totalSamples(self):
        return self._dll.speechPlayer_node_totalSamples(self._h)

    def shards(self):
        """[(first utterance, utterances, samples, device)] per shard."""
        import ctypes
        out = []
        for d in range(self._dll.speechPlayer_node_devices(self._h)):
            a, n, s, dev = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
            self._check(self._dll.speechPlayer_node_shardInfo(self._h, d, ctypes.byref(a), ctypes.byref(n), ctypes.byref(s), ctypes.byref(dev)))
            out.append((a.value, n.value, s.value, dev.value))
        return out

    def synthesize(self, wait=True):
        self._check(self._dll.speechPlayer_node_synthesize(self._h))
        if wait:
            self._check(self._dll.speechPlayer_node_wait(self._h))

    def read(self, u):
        if not 0 <= u < self.nUtterances:
            raise RuntimeError("NodePlayer.read: utterance %d out of range" % u)
        n = int(self._lens[u]) if self._lens is not None else int(self.utteranceSamples(u))
        buf = np.zeros(max(n, 1), dtype=np.int16)
        got = self._check(self._dll.speechPlayer_node_read(self._h, u, buf.ctypes.data, n))
        return buf[:got]

    def getLastIndex(self, u):
        return self._dll.speechPlayer_node_getLastIndex(self._h, u)

    def setOption(self, name, value):
        """Batch options go to every shard; "deal": 0 contiguous shards (default), 1 the sorted deal (blocks of 64 length-sorted
        utterances dealt round-robin) -- set it before setUtterances."""
        self._check(self._dll.speechPlayer_node_setOption(self._h, name.encode(), int(value)))

    def shardUtterances(self, d):
        """The utterances of shard d (numbers in the node batch), in the shard's own order."""
        n = self._check(self._dll.speechPlayer_node_shardUtterances(self._h, d, None, 0))
        out = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._dll.speechPlayer_node_shardUtterances(self._h, d, out.ctypes.data, n))
        return out[:n]

    def digests(self):
        """Per-utterance digests of the PCM in the node batch's utterance order, computed where each shard's PCM lives
        (speechPlayer_batch_digest on the shards: nothing is copied but 8 bytes per utterance)."""
        out = np.zeros(max(self.nUtterances, 1), dtype=np.uint64)
        for d in range(self._dll.speechPlayer_node_devices(self._h)):
            mem = self.shardUtterances(d)
            part = self._dll.speechPlayer_node_part(self._h, d)
            if not part:
                raise RuntimeError("speechPlayer_node_part(%d) failed: %s" % (d, _native.last_error()))
            per = np.zeros(max(len(mem), 1), dtype=np.uint64)
            self._check(self._dll.speechPlayer_batch_digest(part, per.ctypes.data, None))
            out[mem] = per[:len(mem)]
        return out[:self.nUtterances]

    def time(self, launches):
        ms = np.zeros(launches, dtype=np.float32)
        self._check(self._dll.speechPlayer_node_time(self._h, launches, ms.ctypes.data))
        return ms

    def close(self):
        if getattr(self, "_h", None):
            self._dll.speechPlayer_node_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
