"""The glottal source of a batch on the host (include/speechPlayer_batch.h: speechPlayer_batch_exportSource, _epochCounts, _exportEpochs):
declarations and bindings, the argument checks of BatchPlayer.sourceTensor -- and `source`, the comparand of tests/test_gpu_source.py:
the definitions of the header restated one sample at a time over `walk` (tests/test_timeline_host.py, itself held to the oracle), with
math.sin and x - math.trunc(x).  The inputs the GPU tests compare exactly are checked here for ties, so that no GPU test has to set an
utterance aside.  No GPU."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import scenarios
from tests.test_timeline_host import utterance, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
NEW_ENTRIES = ("speechPlayer_batch_exportSource", "speechPlayer_batch_epochCounts", "speechPlayer_batch_exportEpochs")
F0, PHASE, VIBRATO_PHASE, CYCLE, OPEN, WAVE = range(6)
NAMED = ("hannah_vibrato", "nan_hold", "duration_edges", "cfg0_a_1s_batch")      # the scenarios tests/test_gpu_source.py compares
NAN = float("nan")


def frac(x):
    return x - math.trunc(x) if math.isfinite(x) else NAN


def source(cur, sr):
    """The definitions of include/speechPlayer_batch.h over cur [L, 47], the frame of every sample (walk): -> (columns [L, 6] float64,
    epochs [E, 4] float64, x [L]: the sum whose fraction is the glottal phase).  Plain Python floats: every operation is one IEEE
    binary64 operation, in the order the header gives."""
    sr = float(sr)
    L = len(cur)
    cols = np.zeros((L, 6))
    xs = np.zeros(L)
    epochs = []
    V = P = 0.0
    C = 0
    for t, f in enumerate(np.asarray(cur, dtype=np.float64).tolist()):
        V = frac(f[2] / sr + V)
        vib = math.sin(V * 6.283185307179586) * 0.06 * f[1] + 1
        hz = f[0] * vib
        x = hz / sr + P
        P = frac(x)
        epoch = math.isfinite(x) and abs(x) >= 1
        C += epoch
        cols[t] = (hz, P, V, C, 1.0 if P >= f[4] else 0.0, (P * 2 - 1) * f[5])
        xs[t] = x
        if epoch:
            epochs.append((float(t), t - P / (hz / sr), hz, f[5] * f[44]))
    return cols, np.array(epochs, dtype=np.float64).reshape(len(epochs), 4), xs


def vibrato_free(cur):
    """vibratoPitchOffset is exactly zero on every sample: vib is 1 exactly (or NaN on both sides), whatever the sine's last bit."""
    return not cur[:, 1].any()


def ties(cur, cols, xs):
    """Samples on which a sine one ulp off could change CYCLE, OPEN or the epochs: -> (wrap ties, open-quotient ties).  vib is exact
    up to the first sample with a vibrato depth, so the phases carry no difference before it; from there on a phase differs by at most
    L * 2^-52, and a tie is |x| within that of an integer >= 1, or P within that of glottalOpenQuotient.  None in a vibrato-free utterance."""
    L = len(cur)
    deep = np.flatnonzero(cur[:, 1] != 0)
    if not len(deep):
        return 0, 0
    tol = L * 2.0 ** -52
    sl = slice(int(deep[0]), None)
    with np.errstate(invalid="ignore"):
        ax = np.abs(xs[sl])
        wrap = np.isfinite(ax) & (ax > 0.5) & (np.abs(ax - np.round(ax)) < tol)
        opened = np.abs(cols[sl, PHASE] - cur[sl, 4]) < tol
    return int(wrap.sum()), int(opened.sum())


class Sourced:
    """A batch and, per utterance, the walk's frames and the restatement over them, computed when first asked for."""

    def __init__(self, batch, sr=22050):
        self.b, self.sr = batch, sr
        self.n = len(batch["frame_start"]) - 1
        self._t = {}

    def get(self, u):
        """-> (cur, columns, epochs, x)"""
        if u not in self._t:
            cur = walk(*utterance(self.b, u))[0]
            self._t[u] = (cur,) + source(cur, self.sr)
        return self._t[u]

    def length(self, u):
        return len(self.get(u)[0])


@functools.lru_cache(maxsize=None)
def compared(name):
    """The batches tests/test_gpu_source.py holds to the restatement, computed once per process."""
    if name == "plain":
        return Sourced(scenarios.random_batch(np.random.default_rng(21), 24))
    if name == "wild":
        return Sourced(scenarios.random_batch(np.random.default_rng(22), 24, wild=True))
    if name == "plain16k":
        return Sourced(scenarios.random_batch(np.random.default_rng(21), 24), sr=16000)
    if name == "named":
        from tests.test_gpu_parity import make_batch
        by_name = {s.name: s for s in scenarios.build_scenarios(scenarios.Ref()) if s.batchable and s.sr == 22050}
        return Sourced(make_batch([by_name[n] for n in NAMED]))
    raise KeyError(name)


def test_entry_points_are_declared_exported_and_bound():
    from nvspeechplayer_amd import _native
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name in NEW_ENTRIES:
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_longlong and fn.argtypes, name
    assert len(L.speechPlayer_batch_exportSource.argtypes) == 11 and len(L.speechPlayer_batch_epochCounts.argtypes) == 4
    assert len(L.speechPlayer_batch_exportEpochs.argtypes) == 8 and L.speechPlayer_batch_exportEpochs.argtypes[5] is ctypes.c_double
    for k, name in enumerate(("F0", "PHASE", "VIBRATO_PHASE", "CYCLE", "OPEN", "WAVE", "COLUMNS")):
        assert any(line.split()[:3] == ["#define", "SPEECHPLAYER_SOURCE_" + name, str(k)] for line in header.splitlines()), name
    assert "#define SPEECHPLAYER_EPOCH_COLUMNS 4" in header
    from nvspeechplayer_amd import speechPlayer
    assert speechPlayer.SOURCE_COLUMNS == ["f0", "phase", "vibratoPhase", "cycle", "open", "wave"]
    assert speechPlayer.EPOCH_COLUMNS == ["sample", "instant", "f0", "gain"]
    for method in ("sourceTensor", "epochCounts", "epochTensor"):
        assert callable(getattr(speechPlayer.BatchPlayer, method)), method


def test_a_null_batch_is_an_argument_error():
    from nvspeechplayer_amd import _native
    L = _native.load()
    cols = np.array([1], np.int32)
    assert L.speechPlayer_batch_exportSource(None, None, 0, cols.ctypes.data, 1, 1, 0, None, 1, 0, None) == -1
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"exportSource" in L.speechPlayer_lastError()
    assert L.speechPlayer_batch_epochCounts(None, None, 0, None) == -1
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"epochCounts" in L.speechPlayer_lastError()
    assert L.speechPlayer_batch_exportEpochs(None, None, 0, None, 0, -1.0, 0, None) == -1
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"exportEpochs" in L.speechPlayer_lastError()


def test_source_request_checks():
    import torch
    from nvspeechplayer_amd.speechPlayer import SOURCE_COLUMNS, check_source_request
    cols, hop, phase, fmt = check_source_request(["f0", "wave", 3, "phase", "f0"], 256, 3, None)
    assert list(cols) == [0, 5, 3, 1, 0] and cols.dtype == np.int32 and (hop, phase, fmt) == (256, 3, 1)
    assert check_source_request("vibratoPhase", 1, 0, torch.float64)[0].tolist() == [SOURCE_COLUMNS.index("vibratoPhase")]
    assert check_source_request(range(6), 1, 0, torch.float64)[3] == 0
    with pytest.raises(KeyError):
        check_source_request(["voicePitch"], 1, 0, None)
    with pytest.raises(ValueError):
        check_source_request([6], 1, 0, None)
    with pytest.raises(ValueError):
        check_source_request([-1], 1, 0, None)
    with pytest.raises(ValueError):
        check_source_request([], 1, 0, None)
    with pytest.raises(ValueError):
        check_source_request([0], 0, 0, None)
    with pytest.raises(ValueError):
        check_source_request([0], 1, -1, None)
    with pytest.raises(TypeError):
        check_source_request([0], 1, 0, torch.int16)


def test_a_steady_quarter_rate_pitch_by_hand():
    """voicePitch = sr / 4 without vibrato, after a fade of 1: the phase steps by a quarter, wraps on every fourth sample, and the
    wave takes its four values."""
    sr = 22050
    f = np.zeros(47); f[0] = f[46] = sr / 4; f[4] = 0.5; f[5] = 0.75; f[44] = 2.0
    cur = walk(f[None], [20], [1], [-1], [0])[0]
    assert len(cur) == 21 and not cur[0].any() and list(cur[1:, 0]) == [sr / 4] * 20
    cols, epochs, xs = source(cur, sr)
    assert list(cols[:, PHASE]) == [0.0] + [0.25, 0.5, 0.75, 0.0] * 5
    assert list(cols[:, F0]) == [0.0] + [sr / 4] * 20 and not cols[:, VIBRATO_PHASE].any()
    assert list(epochs[:, 0]) == [4.0, 8.0, 12.0, 16.0, 20.0] and list(epochs[:, 1]) == [4.0, 8.0, 12.0, 16.0, 20.0]
    assert list(epochs[:, 2]) == [sr / 4] * 5 and list(epochs[:, 3]) == [1.5] * 5
    assert list(cols[:, CYCLE]) == [float(t // 4) for t in range(21)]
    assert list(cols[1:, WAVE]) == [-0.5 * 0.75, 0.0, 0.5 * 0.75, -0.75] * 5 and cols[0, WAVE] == 0.0      # (sample 0: amplitude 0)
    assert list(cols[:, OPEN]) == [1.0] + [0.0, 1.0, 1.0, 0.0] * 5       # P >= 0.5; sample 0 compares 0 >= 0
    assert ties(cur, cols, xs) == (0, 0)                                   # exact wraps, but no vibrato: nothing can move them


def test_the_vibrato_phase_by_hand():
    """vibratoSpeed = sr / 8 gives V its eight values, with or without a depth; a depth moves the pitch by 6 % of it at most."""
    sr = 16000
    cur = np.zeros((17, 47)); cur[:, 2] = sr / 8; cur[:, 0] = 100.0
    cols, epochs, _ = source(cur, sr)
    assert list(cols[:, VIBRATO_PHASE]) == [((t + 1) % 8) / 8 for t in range(17)]
    assert list(cols[:, F0]) == [100.0] * 17 and len(epochs) == 0
    cur[:, 1] = 0.5
    deep = source(cur, sr)[0]
    assert list(deep[:, VIBRATO_PHASE]) == list(cols[:, VIBRATO_PHASE])
    assert deep[1, F0] == 100.0 * (math.sin(0.25 * 6.283185307179586) * 0.06 * 0.5 + 1) and abs(deep[1, F0] - 103.0) < 1e-12
    assert np.all(np.abs(deep[:, F0] - 100.0) <= 3.0 + 1e-12)


def test_a_nan_pitch_freezes_the_cycle_count_by_hand():
    sr = 22050
    cur = np.zeros((12, 47)); cur[:, 0] = sr / 2; cur[:, 5] = 1.0; cur[:, 44] = 1.0; cur[:, 4] = 0.25
    cur[7, 0] = NAN
    cols, epochs, xs = source(cur, sr)
    assert list(cols[:7, PHASE]) == [0.5, 0.0, 0.5, 0.0, 0.5, 0.0, 0.5] and np.isnan(cols[7:, PHASE]).all()
    assert list(cols[:, CYCLE]) == [0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0] + [3.0] * 5
    assert list(epochs[:, 0]) == [1.0, 3.0, 5.0] and np.isnan(cols[7:, WAVE]).all()
    assert not cols[7:, OPEN].any() and list(cols[8:, F0]) == [sr / 2] * 4 and np.isnan(cols[7, F0])
    # an infinite pitch does the same through frac
    cur[7, 0] = float("inf")
    cols = source(cur, sr)[0]
    assert np.isnan(cols[7:, PHASE]).all() and cols[7, F0] == float("inf") and cols[-1, CYCLE] == 3.0


def test_an_option_value_that_does_not_fit_a_c_int_is_refused():
    """speechPlayer_batch_setOption takes an int: 2 ** 40 would arrive as 0 ("source_lane_lists" would then send every walk through
    the lane kernel instead of none)."""
    from nvspeechplayer_amd.speechPlayer import check_option_value
    assert check_option_value("source_lane_lists", 2 ** 31 - 1) == 2 ** 31 - 1 and check_option_value("layout", -1) == -1
    assert check_option_value("source_table_mb", np.int64(7)) == 7 and check_option_value("mode", -2 ** 31) == -2 ** 31
    for value in (2 ** 31, 1 << 40, -2 ** 31 - 1):
        with pytest.raises(ValueError):
            check_option_value("source_lane_lists", value)


@pytest.mark.parametrize("name", ["plain", "wild", "named", "plain16k"])
def test_what_the_gpu_tests_compare_has_no_tie(name):
    """The share of utterances tests/test_gpu_source.py may set aside is zero: no sample of its batches is a tie, so CYCLE, OPEN, the
    epochs' samples and the counts must be equal exactly.  Also what the issue recorded about the two random batches."""
    s = compared(name)
    samples = epochs = vibrato = free = nan = 0
    for u in range(s.n):
        cur, cols, ep, xs = s.get(u)
        assert ties(cur, cols, xs) == (0, 0), (name, u)
        samples += len(cur); epochs += len(ep)
        vibrato += int((cur[:, 1] != 0).any()); free += int(vibrato_free(cur)); nan += int(np.isnan(cols[:, PHASE]).any())
    print(name, "utterances", s.n, "samples", samples, "epochs", epochs, "with vibrato", vibrato, "vibrato-free", free, "NaN phase", nan)
    if name == "plain":
        assert (s.n, samples, epochs, vibrato, free) == (24, 90428, 1215, 18, 6)
    if name == "wild":
        assert (s.n, samples, epochs, vibrato, free, nan) == (24, 121150, 1240, 20, 4, 3)      # (three of the four vibrato-free ones reach a NaN phase)
    if name == "named":
        assert s.n == len(NAMED) and vibrato >= 1 and free >= 1 and epochs > 100
