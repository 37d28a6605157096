"""The response, stems and source exports (csrc/klatt_response.h, klatt_stems.h, klatt_source.h) at every sample rate, on the two-part
batch of tests/export_rates.py: the edge part reaches every class of the coefficient code from mixed wavefronts, the pure part fills
wavefronts with one class -- the two wave-uniform short cuts of coefficient_parts (csrc/klatt_device.h) -- and breaks them by one lane.
Each export against the host statement that tests/test_export_rates_host.py holds to something independent at the rate.  Formats, hops,
padding, refusals and stream ordering do not depend on the rate: tests/test_gpu_response.py, test_gpu_stems.py, test_gpu_source.py.
Needs a GPU."""
import numpy as np
import pytest

from tests import export_rates as X
from tests import oracle
from tests.export_rates import RATES
from tests.test_gpu_parity import compare
from tests.test_gpu_response import ALL as KINDS, PARAMS, host_equal
from tests.test_gpu_source import check_batch
from tests.test_gpu_stems import ALL as COLUMNS, check_rows, rows_of
from tests.test_gpu_timeline import same as same_bits
from tests.test_response_host import LEFT_OUT_MOST, bounded_response, within
from tests.test_source_host import Sourced
from tests.test_stems_host import OUTPUT, Stemmed, in_documented_range, native_coefficients, same, stems, to_pcm

pytestmark = pytest.mark.gpu
THREADS = 16


@pytest.fixture(scope="module", params=RATES)
def held(request):
    """One BatchPlayer at the rate, both parts set as shared lists (rows 2, 66 and 130 speak their left neighbour's list), synthesised
    once in MODE_EXACT: -> dict(sr, bp, parts, lens, pcm, starts)."""
    import nvspeechplayer_amd as eng
    sr = request.param
    p = X.parts(sr)
    lists = p["lists"]
    bp = eng.BatchPlayer(sr)
    bp.setUtterancesShared(lists["frame_start"], lists["frames"], lists["min"], lists["fade"], p["list_of"], lists["index"], lists["isnull"], p["seeds"])
    lens = X.lengths(p["batch"])
    assert bp.nUtterances == len(lens) and bp.totalSamples == int(lens.sum())
    bp.synthesize()
    pcm, starts = bp.readAll()
    assert np.array_equal(np.diff(starts), lens)
    yield dict(sr=sr, bp=bp, parts=p, lens=lens, pcm=pcm, starts=starts)
    bp.close()


def test_response(held):
    """responseTensor at bins(sr), all eight kinds, float64, packed, without and with the gains -- the pure part on every sample, the
    edge part on every third -- against speechPlayer_frameResponse of trackTensor's frames at the rate: on the steps whose frames are
    inside the documented range RE, IM and MAG bit for bit and the dB kinds within 4 ulp (host_equal); on the distinct frames of all
    steps, the out-of-range utterances' among them, within bounded_response's bounds with no miss and at most LEFT_OUT_MOST left out.
    Rows of one list are equal bit for bit; an odd one out equals the row it copies on every step whose frame is untouched, although
    the wavefronts of the steps next to the changed ones voted differently."""
    import torch
    sr, bp, p = held["sr"], held["bp"], held["parts"]
    freqs = X.bins(sr)
    for name, rows, hop, phase in (("pure", p["pure"], 1, 0), ("edge", p["edge"], 3, 1)):
        rows = [int(u) for u in rows]
        tracks, off = bp.trackTensor(PARAMS, hop=hop, phase=phase, utterances=rows, dtype=torch.float64, padded=False)
        frames, off = tracks.cpu().numpy(), off.numpy()
        del tracks
        inside = X.in_range(frames, sr)
        assert np.isfinite(frames[:, 1:46]).all() and (inside.all() if name == "pure" else 0 < (~inside).sum() < len(frames))
        keyed = frames.copy()
        keyed[:, [0, 46]] = 0.0
        first = np.unique(keyed, axis=0, return_index=True)[1]
        del keyed
        for gain in (False, True):
            t, goff = bp.responseTensor(freqs, KINDS, hop=hop, phase=phase, utterances=rows, dtype=torch.float64, padded=False, gain=gain)
            got = t.cpu().numpy()
            del t
            assert np.array_equal(goff.numpy(), off) and got.shape == (len(frames), 8, 5)
            assert host_equal(got[inside], frames[inside], freqs, KINDS, gain, sr), (sr, name, gain)
            miss = left_out = total = 0
            for i in range(0, len(first), 4096):
                pick = first[i:i + 4096]
                value, bound, rel = bounded_response(frames[pick], sr, freqs, gain)
                m, l, n = within(got[pick], value, bound, rel)
                miss, left_out, total = miss + m, left_out + l, total + n
            print("%d Hz %s part, gain %d: %d steps, %d distinct frames, %d of %d elements left out (share %.4f), %d miss their bound" % (
                sr, name, gain, len(frames), len(first), left_out, total, left_out / total, miss))
            assert miss == 0 and left_out <= LEFT_OUT_MOST * total, (sr, name, gain, miss, left_out, total)
            if name == "edge":
                continue
            row = lambda r, a=got: a[off[r]:off[r + 1]]
            for r in X.SHARED:
                assert same_bits(row(r), row(r - 1)) and not same_bits(row(r)[:400], row(r + 1)[:400]), (sr, r)
            for odd, orig in X.pure_part(sr)["original"].items():
                fo, fg = frames[off[odd]:off[odd + 1]], frames[off[orig]:off[orig + 1]]
                untouched = (fo == fg).all(axis=1)
                changed = np.flatnonzero(~untouched)
                assert len(changed) > 100 and untouched[:changed[0]].all() and untouched[changed[-1] + 1:].sum() > 16, (sr, odd)
                assert same_bits(row(odd)[untouched], row(orig)[untouched]) and not same_bits(row(odd)[changed], row(orig)[changed]), (sr, odd)


def test_stems(held):
    """All seven columns, float64, packed.  The pure part exported on its own: its rows' lengths do not increase, so the kernel's
    wavefronts are 64 low rows, 64 upper rows, 63 low rows with the odd one at lane 37, and a ragged one; the edge part on its own.
    The utterances of restated_subset(sr), all inside the documented range: bit for bit against `stems` over the device's own glottal
    phase and speechPlayer_resonatorCoefficients.  Every utterance of the batch: OUTPUT clipped and truncated is the engine's
    MODE_EXACT PCM on every sample, and the oracle's at the usual bar.  An odd one out equals the row it copies, with its seed, in all
    seven columns on every sample before their frames part."""
    import torch
    sr, bp, p, lens, pcm, starts = (held[k] for k in ("sr", "bp", "parts", "lens", "pcm", "starts"))
    b = p["batch"]
    got = {}
    for rows in (p["pure"], p["edge"]):
        rows = [int(u) for u in rows]
        flat, offsets = bp.stemTensor(COLUMNS, utterances=rows, dtype=torch.float64, padded=False)
        assert int(offsets[-1]) == 7 * int(lens[rows].sum())
        got.update(zip(rows, rows_of(flat, offsets.numpy(), lens[rows], 7)))
    assert sorted(got) == list(range(len(lens)))
    # the restated subset, bit for bit
    s = Stemmed(b, sr)
    sub = X.restated_subset(sr)
    ph, off = bp.sourceTensor(["phase"], utterances=sub, dtype=torch.float64, padded=False)
    ph, off = ph.cpu().numpy()[:, 0], off.numpy()
    want = []
    for i, u in enumerate(sub):
        cur = s.cur(u)
        assert in_documented_range(cur, sr) and off[i + 1] - off[i] == len(cur), (sr, u)
        want.append(stems(cur, ph[off[i]:off[i + 1]], s.seed(u), sr, native_coefficients))
    check_rows([got[u] for u in sub], want, "%d Hz, utterances %s" % (sr, sub))
    # every utterance: the engine's PCM exactly, the oracle's at compare's bar
    exp, exp_start, total = oracle.batch_synthesize(sr, b, threads=THREADS)
    assert total == len(pcm) and np.array_equal(exp_start, starts)
    flips = 0
    for u in range(len(lens)):
        mine = to_pcm(got[u][OUTPUT])
        differ = np.flatnonzero(mine != pcm[starts[u]:starts[u + 1]])
        assert len(differ) == 0, ("engine", sr, u, len(differ), int(differ[0]))
        flips += compare(mine, exp[starts[u]:starts[u + 1]], "%d Hz stems utt %d" % (sr, u))
    print("%d Hz stems: %d utterances, %d samples, %d one-LSB differences from the oracle" % (sr, len(lens), total, flips))
    # the odd ones out and the rows they copy
    for odd, orig in X.pure_part(sr)["original"].items():
        part = int(np.flatnonzero((s.cur(odd) != s.cur(orig)).any(axis=1))[0])
        assert part > 120 and p["seeds"][odd] == p["seeds"][orig]
        for c in COLUMNS:
            assert same(got[odd][c, :part], got[orig][c, :part]), (sr, odd, c)
        assert not same(got[odd][OUTPUT], got[orig][OUTPUT]), (sr, odd)
        assert np.array_equal(to_pcm(got[odd][OUTPUT, :part]), pcm[starts[orig]:starts[orig] + part]), (sr, odd)
    for r in X.SHARED:      # one list, two seeds: the noisy rows differ
        assert not same(got[r][OUTPUT], got[r - 1][OUTPUT]), (sr, r)


def test_source(held):
    """Every column of every sample and every epoch of restated_subset(sr) -- tie-free at every rate (tests/test_export_rates_host.py)
    -- with tests/test_gpu_source.py's own tolerances for the sine's last bit."""
    sr, bp, p = held["sr"], held["bp"], held["parts"]
    sub = X.restated_subset(sr)
    samples, epochs = check_batch(bp, Sourced(p["batch"], sr), utterances=sub)
    assert samples == int(held["lens"][sub].sum()) and epochs > 100
