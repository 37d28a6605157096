"""ctypes binding of oracle/_ref/libspeechPlayer_ref.so -- the reference itself, compiled in place from its checkout.

Test infrastructure, shaped like tests/oracle.py.  `make -C oracle ref` builds the library (oracle/Makefile; the checkout's
place comes from NVSP_REFERENCE); it is kept out of git, so a clone without a checkout beside it has none: available() says
so and the tests that need it skip.  What the library answered is recorded as digests in tests/golden/reference.json.

Noise: the reference calls the process-global rand(); the build sends it to ref_rand() (oracle/ref_noise.cpp), which passes
through to libc or gives klatt_noise31(seed, k).  That state is global, so every call into the library is made under one lock
with the calling player's (seed, k) put in first and k read back after.
"""
import ctypes
import os
import subprocess
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
LIB_PATH = os.path.join(ORACLE_DIR, "_ref", "libspeechPlayer_ref.so")
CHECKOUT = os.environ.get("NVSP_REFERENCE", "/root/reference")

NOISE_LIBC = 0
NOISE_COUNTER = 1
NP = 47

_lib = None
_lock = threading.Lock()


def have_checkout():
    return os.path.exists(os.path.join(CHECKOUT, "src", "speechWaveGenerator.cpp"))


def available():
    """The library is there, or can be built from the checkout."""
    return os.path.exists(LIB_PATH) or have_checkout()


def build(force=False):
    if have_checkout():         # make rebuilds when the recipe or the checkout changed
        subprocess.check_call(["make", "-s"] + (["-B"] if force else []) + ["-C", ORACLE_DIR, "ref", "NVSP_REFERENCE=" + CHECKOUT])
    elif not os.path.exists(LIB_PATH):
        raise RuntimeError("no %s and no reference checkout at %s" % (LIB_PATH, CHECKOUT))
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(LIB_PATH)
        vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        L.speechPlayer_initialize.restype = vp          # (a 64-bit handle: the default int would cut it)
        L.speechPlayer_initialize.argtypes = [i32]
        L.speechPlayer_queueFrame.restype = None
        L.speechPlayer_queueFrame.argtypes = [vp, vp, u32, u32, i32, ctypes.c_bool]
        L.speechPlayer_synthesize.restype = i32
        L.speechPlayer_synthesize.argtypes = [vp, u32, vp]
        L.speechPlayer_getLastIndex.restype = i32
        L.speechPlayer_getLastIndex.argtypes = [vp]
        L.speechPlayer_terminate.restype = None
        L.speechPlayer_terminate.argtypes = [vp]
        L.ref_noise_set.restype = None
        L.ref_noise_set.argtypes = [i32, u32, u32]
        L.ref_noise_position.restype = u32
        L.ref_noise_position.argtypes = []
        L.ref_noise31.restype = u32
        L.ref_noise31.argtypes = [u32, u32]
        _lib = L
    return _lib


class RefPlayer:
    """tests/oracle.py's OraclePlayer on the compiled reference: durations in samples."""

    def __init__(self, sample_rate, noise=NOISE_COUNTER, seed=0):
        self.L = lib()
        self.noise, self.seed, self.k = int(noise), int(seed) & 0xFFFFFFFF, 0
        with _lock:
            self.h = self.L.speechPlayer_initialize(int(sample_rate))
        assert self.h

    def queue(self, frame, min_samples, fade_samples, user_index=-1, purge=False):
        if frame is None:
            ptr = None
        else:
            buf = np.ascontiguousarray(frame, dtype=np.float64)
            assert buf.shape == (NP,)
            ptr = buf.ctypes.data
        with _lock:
            self.L.speechPlayer_queueFrame(self.h, ptr, int(min_samples), int(fade_samples), int(user_index), bool(purge))

    def synthesize(self, n):
        out = np.zeros(n, dtype=np.int16)
        with _lock:
            self.L.ref_noise_set(self.noise, self.seed, self.k)
            got = self.L.speechPlayer_synthesize(self.h, n, out.ctypes.data)
            self.k = self.L.ref_noise_position()
        return out[:got]

    def drain(self, chunk=8192):
        parts = []
        while True:
            p = self.synthesize(chunk)
            parts.append(p)
            if len(p) < chunk:
                break
        return np.concatenate(parts) if parts else np.zeros(0, np.int16)

    def last_index(self):
        with _lock:
            return self.L.speechPlayer_getLastIndex(self.h)

    def close(self):
        if self.h:
            with _lock:
                self.L.speechPlayer_terminate(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def play_reference(scn):
    """scenarios.play_oracle on the compiled reference."""
    from tests import scenarios
    return scenarios.play(scn, RefPlayer(scn.sr, noise=NOISE_COUNTER, seed=scn.seed))
