"""The row source of the PCM-derived exports and the helpers the binding shares (nvspeechplayer_amd/speechPlayer.py: RowSource,
_step_counts, _sample_format through the check_*_request functions): which rows a call chooses from the batch's pool or from a signal,
in which words it refuses, what record a signal becomes, how many steps a length has, which dtypes name a sample format.  No GPU."""
import numpy as np
import pytest

from nvspeechplayer_amd import speechPlayer as sp

LENGTHS = np.array([7, 0, 300, 12, 5], np.int64)


def pool(utterances, lengths=LENGTHS, what="pcmTensor"):
    return sp.RowSource(what, "utterance", len(lengths), lengths, utterances)


def test_none_is_every_row_in_order():
    src = pool(None)
    assert src.sel is None and src.n == 5 and src.count == 5 and (src.lead, src.suffix) == ((), "")
    assert src.lengths.dtype == np.int64 and list(src.lengths) == list(LENGTHS)
    lazy = sp.RowSource("pcmTensor", "utterance", 5, lambda: LENGTHS, [1])      # (the pool's lengths: a call, made when they are asked for)
    assert list(lazy.lengths) == [0]


def test_a_selection_with_repeats_in_reverse_order():
    import torch
    for given in ([4, 2, 2, 0], np.array([4, 2, 2, 0], np.int32), torch.tensor([4, 2, 2, 0])):
        src = pool(given)
        assert src.sel.dtype == np.int64 and src.sel.flags["C_CONTIGUOUS"] and list(src.sel) == [4, 2, 2, 0] and src.n == 4
        assert src.lengths.dtype == np.int64 and list(src.lengths) == [5, 300, 300, 7]


def test_nothing_chosen_and_nothing_to_choose_from():
    src = pool([])
    assert src.n == 0 and src.sel.dtype == np.int64 and len(src.sel) == 0 and len(src.lengths) == 0
    src = pool(None, np.zeros(0, np.int64))
    assert src.n == 0 and src.sel is None and len(src.lengths) == 0
    assert pool([], np.zeros(0, np.int64)).n == 0


@pytest.mark.parametrize("bad", [[-1], [5], [0, 4, 5], [2, -1, 2]])
def test_an_index_outside_is_refused_in_the_inputs_words(bad):
    import torch
    with pytest.raises(ValueError) as e:
        pool(bad, what="mixedTensor")
    assert str(e.value) == "mixedTensor: utterance numbers must lie in [0, 5)"
    signal = (torch.zeros((5, 8), dtype=torch.int16), [8, 0, 3, 1, 2])
    with pytest.raises(ValueError) as e:
        sp.RowSource.of_signal("powerTensor", signal, None, bad)
    assert str(e.value) == "powerTensor: row numbers must lie in [0, 5)"
    with pytest.raises(ValueError) as e:
        pool([0], np.zeros(0, np.int64), what="stemTensor")
    assert str(e.value) == "stemTensor: utterance numbers must lie in [0, 0)"


def fields(src):
    return {k: int(src.record[k][0]) for k in ("data", "format", "nRows", "rowStride")}


def extent_of(src, n):
    import ctypes
    return list((ctypes.c_longlong * n).from_address(int(src.record["extent"][0])))


def test_a_signal_source_from_cpu_tensors():
    import torch
    padded = torch.zeros((3, 10), dtype=torch.int16)
    src = sp.RowSource.of_signal("convolvedTensor", (padded, torch.tensor([10, 0, 4])), None, [2, 0])
    assert src.suffix == "Of" and src.lead == (src.record.ctypes.data,) and src.record.dtype == sp._signalDtype
    assert fields(src) == dict(data=padded.data_ptr(), format=0, nRows=3, rowStride=10) and extent_of(src, 3) == [10, 0, 4]
    assert (src.n, src.count, list(src.sel), list(src.lengths)) == (2, 3, [2, 0], [4, 10]) and src.lengths.dtype == np.int64
    packed = torch.zeros(20, dtype=torch.float32)
    src = sp.RowSource.of_signal("convolvedTensor", (packed, [0, 6, 6, 19]), None, None)
    assert src.suffix == "Of" and fields(src) == dict(data=packed.data_ptr(), format=1, nRows=3, rowStride=0) and extent_of(src, 4) == [0, 6, 6, 19]
    assert (src.n, src.sel, list(src.lengths)) == (3, None, [6, 0, 13])
    empty = torch.zeros((4, 0), dtype=torch.float32)      # rows of nothing: rowStride 0 means packed, so the extents are n + 1 zero offsets
    src = sp.RowSource.of_signal("convolvedTensor", (empty, [0, 0, 0, 0]), None, None)
    assert fields(src)["rowStride"] == 0 and fields(src)["nRows"] == 4 and extent_of(src, 5) == [0] * 5 and list(src.lengths) == [0] * 4
    _, _, n, stride, extent, _ = sp.check_signal_request((empty, [0, 0, 0, 0]))      # (what check_signal_request answers: unchanged)
    assert (n, stride, list(extent)) == (4, 0, [0] * 5)


@pytest.mark.parametrize("hop,phase", [(1, 0), (3, 0), (3, 2), (256, 5)])
def test_step_counts_against_a_loop(hop, phase):
    lens = [0, 1, phase, phase + 1, phase + hop, phase + hop + 1]
    want = [sum(1 for _ in range(phase, L, hop)) for L in lens]
    got = sp._step_counts(np.array(lens), hop, phase)
    assert got.dtype == np.int64 and list(got) == want
    assert [int(sp._step_counts(L, hop, phase)) for L in lens] == want


def requests(dtype):
    """The three request checks that end in the dtype parser: -> their export formats."""
    return (sp.check_resample_request(22050, 16000, 6, 0.99, "hann", None, dtype)[6],
            sp.check_convolve_request(np.ones(3, np.float32), None, 1, True, dtype)[4],
            sp.check_mix_request([[]], 1, None, dtype)[3])


def test_the_dtype_parser_through_the_three_requests():
    import torch
    for dtype, fmt in ((None, 1), (np.float32, 1), (torch.float32, 1), ("float32", 1), (np.int16, 0), (torch.int16, 0), ("int16", 0)):
        assert requests(dtype) == (fmt, fmt, fmt), dtype
    for dtype in (np.float64, torch.int32, "pcm"):
        for what, call in (("resampledTensor", lambda: sp.check_resample_request(22050, 16000, 6, 0.99, "hann", None, dtype)),
                           ("pcmResample", lambda: sp.check_resample_request(22050, 16000, 6, 0.99, "hann", None, dtype, "pcmResample")),
                           ("convolvedTensor", lambda: sp.check_convolve_request(np.ones(3, np.float32), None, 1, True, dtype)),
                           ("signalConvolve", lambda: sp.check_convolve_request(np.ones(3, np.float32), None, 1, True, dtype, "signalConvolve")),
                           ("mixedTensor", lambda: sp.check_mix_request([[]], 1, None, dtype)),
                           ("signalMix", lambda: sp.signalMix(np.zeros(4, np.float32), [], [], dtype=dtype))):
            with pytest.raises(TypeError) as e:
                call()
            assert str(e.value) == "%s: dtype must be float32 or int16, not %s" % (what, dtype), (what, dtype)
