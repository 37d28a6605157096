"""The PCM-derived exports (BatchPlayer.spectrogramTensor, resampledTensor, convolvedTensor, mixedTensor, powerTensor) read the batch's
pool or a signal through one body each: on a batch whose rows end beside, on and past the ends of the 1024-sample tiles, the pool, the
pool's int16 PCM handed back padded and the same handed back packed give the same bits and the same second tensors, in both output forms
and under a selection with repeats; and every input refuses in its own words.  Needs a GPU.

The rows have 3, 63, 1024, 1025 and 2049 samples: the shortest utterance a request can make (a frame lasts max(min, fade + 1) + 1 samples,
and a fade at least one: there is no utterance of one sample), just under a wavefront, one tile, one past it, two tiles and one."""
import numpy as np
import pytest

from tests.test_gpu_mix import single_frames
from tests.test_gpu_spectrogram import player

pytestmark = pytest.mark.gpu
LENS = [3, 63, 1024, 1025, 2049]
SEL = [4, 0, 0, 2]
TAPS = np.array([0.5, -0.25, 0.125, 0.0625, -0.03125], np.float32)


@pytest.fixture(scope="module")
def inputs():
    """The player, its PCM, and the three inputs: None (the pool) and pcmTensor(int16), padded and packed, as signal=."""
    import torch
    bp, pcm = player(single_frames(LENS))
    assert [len(p) for p in pcm] == LENS and sum(p.any() for p in pcm) >= 4
    yield bp, pcm, [None, bp.pcmTensor(dtype=torch.int16, padded=True), bp.pcmTensor(dtype=torch.int16, padded=False)]
    bp.close()


def terms(rows):
    import nvspeechplayer_amd as eng
    return [[eng.MixTerm(utterance=(u + 1) % len(LENS), gain=0.5)] for u in rows]


EXPORTS = {
    "spectrogramTensor": lambda bp, rows, **kw: bp.spectrogramTensor(nFft=64, hop=16, **kw),
    "resampledTensor": lambda bp, rows, **kw: bp.resampledTensor(16000, **kw),
    "convolvedTensor": lambda bp, rows, **kw: bp.convolvedTensor(TAPS, **kw),
    "mixedTensor": lambda bp, rows, **kw: bp.mixedTensor(terms(rows), **kw),
}


def same_bytes(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_the_three_inputs_give_the_same_bits(inputs, name):
    import torch
    bp, pcm, signals = inputs
    for utterances in (None, SEL):
        rows = range(len(LENS)) if utterances is None else utterances
        for padded in (True, False):
            outs = [EXPORTS[name](bp, rows, utterances=utterances, padded=padded, signal=s) for s in signals]
            assert outs[0][0].numel() > 0 and outs[0][0].any()
            for out, second in outs[1:]:
                assert same_bytes(out, outs[0][0]) and second.dtype == torch.int64 and torch.equal(second, outs[0][1]), (name, utterances, padded)


def test_power_sums_over_the_pool_and_mean_squares_over_a_signal(inputs):
    import torch
    import nvspeechplayer_amd as eng
    bp, pcm, signals = inputs
    for utterances in (None, SEL):
        rows = range(len(LENS)) if utterances is None else utterances
        sums, lens = bp.powerTensor(utterances=utterances)
        assert sums.dtype == lens.dtype == torch.int64 and sums.is_cuda and lens.is_cuda
        assert list(sums.cpu().numpy()) == [int((pcm[u].astype(np.int64) ** 2).sum()) for u in rows] and list(lens.cpu().numpy()) == [LENS[u] for u in rows]
        for signal in signals[1:]:
            powers, plens = bp.powerTensor(utterances=utterances, signal=signal)
            assert powers.dtype == torch.float64 and torch.equal(plens, lens)
            want = np.array([eng.signalPower(pcm[u]) for u in rows], np.float64)
            assert np.array_equal(powers.cpu().numpy().view(np.uint64), want.view(np.uint64)) and want.any()


def test_every_input_refuses_in_its_own_words(inputs):
    import nvspeechplayer_amd as eng
    bp, pcm, signals = inputs
    on_cpu = (signals[1][0].cpu(), signals[1][1])
    cases = []
    for name, export in list(EXPORTS.items()) + [("powerTensor", lambda bp, rows, **kw: bp.powerTensor(**kw))]:
        cases.append((lambda e=export: e(bp, [0, 5], utterances=[0, 5]), ValueError, "%s: utterance numbers must lie in [0, 5)" % name))
        for signal in signals[1:]:
            cases.append((lambda e=export, s=signal: e(bp, [0, 5], utterances=[0, 5], signal=s), ValueError, "%s: row numbers must lie in [0, 5)" % name))
        cases.append((lambda e=export: e(bp, SEL, utterances=SEL, signal=on_cpu), ValueError,
                      "%s: the samples must be on the batch's device, cuda:%d, not cpu" % (name, bp.device)))
    cases.append((lambda: bp.resampledTensor(16000, signalRate=22050), ValueError, "resampledTensor: signalRate comes with a signal"))
    for signal in signals:
        cases.append((lambda s=signal: bp.convolvedTensor([TAPS, TAPS], irOf=[0, 1, 0], utterances=SEL, signal=s), ValueError,
                      "convolvedTensor: irOf has 3 entries for 4 rows"))
    for signal in signals[1:]:
        cases.append((lambda s=signal: bp.mixedTensor([[]] * 3 + [[eng.MixTerm(noise=0, gain=1.0), eng.MixTerm(utterance=9, gain=0.5)]], utterances=SEL, signal=s),
                      ValueError, "mixedTensor: row 3, term 1: source 9 is not a row of the signal (5)"))
    assert len(cases) == 5 * 4 + 1 + 3 + 2
    for call, kind, message in cases:
        with pytest.raises(kind) as e:
            call()
        assert type(e.value) is kind and str(e.value) == message
    out, second = bp.resampledTensor(16000, utterances=SEL, signal=signals[2])      # the player is as usable as before
    assert list(second.numpy()) == [-(-LENS[u] * 320 // 441) for u in SEL]
