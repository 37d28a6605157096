"""Phoneme alignment of batches set from IPA text, exported on the device (include/speechPlayer_batch.h: speechPlayer_batch_exportAlignment,
_exportUnits, _unitCounts, _setRecordsLabelled; BatchPlayer.alignmentTensor / unitTensor / hasLabels; csrc/klatt_align.h) against
`align_walk` and `unit_table` of tests/test_alignment_host.py.  The comparand takes nothing from the device: its labels are
speechPlayer_ipa_labels's (held to the reference's front-end there) plus the trailing silence, its timeline speechPlayer_planTimeline's
over the producer's durations (held to the oracle in tests/test_timeline_host.py).  Needs a GPU."""
import ctypes

import numpy as np
import pytest

from tests import scenarios
from tests.test_alignment_host import CLAUSES, COLUMNS, GAP, PUFF, UNIT_COLUMNS, align_walk, unit_first, unit_table
from tests.test_timeline_host import plan_timeline

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
ALL = list(range(8))


class Case:
    """One utterance of a text batch as the host knows it: its timeline (first[n + 1]) and its labels (n, the trailing silence last)."""

    def __init__(self, first, labels):
        self.first, self.labels, self.length = first, labels, int(first[-1])

    def dense(self, cols, hop=1, phase=0):
        w = align_walk(self.first, self.labels, hop, phase)
        return np.stack([w[COLUMNS[c]] for c in cols], axis=1).astype(np.int64).reshape(-1, len(cols))

    def steps(self, hop, phase):
        return max(0, -(-(self.length - phase) // hop))


def host_cases(texts, speed=1.0, basePitch=100.0, clauseType=None, textOf=None, tail=150.0, **_):
    """What setIpa(texts, ...) must leave on the device, from the host alone."""
    from nvspeechplayer_amd import ipa
    count = len(ipa.phonemeSymbols()) - 2
    pk = ipa.frames_for_batch(texts, speed=speed, basePitch=basePitch, clauseType=clauseType, trailing_silence_ms=tail, textOf=textOf)
    first, length = plan_timeline(pk["frame_start"], pk["min"], pk["fade"])
    fs = pk["frame_start"]
    own = {}
    out = []
    for u in range(len(fs) - 1):
        text = texts[u if textOf is None else int(textOf[u])]
        if text not in own:
            lab = ipa.labels(text)
            sil = np.array([(count + 1, 0, (int(lab["unit"].max()) + 1) if len(lab) else 0, -1)], ipa.LABEL_DTYPE)
            own[text] = np.concatenate([lab, sil]) if tail is not None else lab
        assert fs[u + 1] - fs[u] == len(own[text])
        out.append(Case(np.concatenate([first[fs[u]:fs[u + 1]], [length[u]]]), own[text]))
    return out


@pytest.fixture(scope="module")
def groups():
    """The 126 cases of ref_frames.npz, grouped by speed (a setIpa call has one): [(setIpa arguments, [Case])]."""
    z = np.load(scenarios.GOLDEN + "/ref_frames.npz")
    lines = [b.decode("utf8") for b in z["ipa_lines"]]
    by_speed = {}
    for meta in z["ipa_case_meta"]:
        by_speed.setdefault((float(meta[1]), float(meta[4])), []).append((lines[int(meta[0])], CLAUSES[int(meta[2])], float(meta[3])))
    out = []
    for (speed, infl), items in sorted(by_speed.items()):
        spec = dict(texts=[t for t, _, _ in items], speed=speed, inflection=infl, clauseType=[c for _, c, _ in items], basePitch=[p for _, _, p in items])
        out.append((spec, host_cases(**spec)))
    assert sum(len(c) for _, c in out) == 126
    return out


def check_packed(bp, cases, cols, hop=1, phase=0, dtype=None, utterances=None):
    order = list(range(len(cases))) if utterances is None else list(utterances)
    got, offsets = bp.alignmentTensor(cols, hop=hop, phase=phase, utterances=utterances, dtype=dtype, padded=False)
    got, offsets = got.cpu().numpy(), offsets.numpy()
    assert len(offsets) == len(order) + 1 and offsets[-1] == len(got) and got.shape[1] == len(cols)
    for r, u in enumerate(order):
        want = cases[u].dense(cols, hop, phase)
        assert offsets[r + 1] - offsets[r] == len(want) == cases[u].steps(hop, phase), (u, hop, phase)
        assert np.array_equal(got[offsets[r]:offsets[r + 1]].astype(np.int64), want), "utterance %d hop %d phase %d" % (u, hop, phase)
    return len(got)


def test_every_sample_of_all_126_cases(groups):
    """Every sample (hop 1) of all 126 cases, all columns, against align_walk; the `frame` column equals trackTensor's.  Then the 126 as ONE
    ragged batch: the groups' records objects merged and set with their labels (setRecordsLabelled) -- the same rows."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import ipa
    bp = eng.BatchPlayer(22050)
    assert not bp.hasLabels
    samples, rows = 0, []
    for spec, cases in groups:
        bp.setIpa(**spec)
        assert bp.hasLabels and bp.nUtterances == len(cases)
        assert [bp.utteranceSamples(u) for u in range(len(cases))] == [c.length for c in cases]
        samples += check_packed(bp, cases, ALL)
        frame, _ = bp.alignmentTensor("frame", padded=False)
        track, _ = bp.trackTensor("frame", dtype=torch.float64, padded=False)
        assert torch.equal(frame, track.to(torch.int64))
        rows.append(bp.alignmentTensor(ALL, padded=False)[0])
    assert samples == sum(c.length for _, cases in groups for c in cases) > 2000000
    shapes, recs, labs, starts, at = [], [], [], [0], 0
    for spec, _ in groups:
        pk = ipa.records_for_batch(spec["texts"], speed=spec["speed"], basePitch=spec["basePitch"], inflection=spec["inflection"], clauseType=spec["clauseType"])
        assert len(set(pk["list_of"])) == len(pk["list_of"])
        r = pk["records"].copy()
        r["shape"] = np.where(r["shape"] == ipa.RECORD_SILENCE, ipa.RECORD_SILENCE, r["shape"] + at).astype(np.uint32)
        for l in pk["list_of"]:
            a, e = pk["list_start"][l], pk["list_start"][l + 1]
            recs.append(r[a:e]); labs.append(pk["labels"][a:e]); starts.append(starts[-1] + e - a)
        shapes.append(pk["shapes"]); at += len(pk["shapes"])
    bp.setRecords(np.concatenate(shapes), starts, np.concatenate(recs), labels=np.concatenate(labs))
    assert bp.hasLabels and bp.nUtterances == 126
    one, offsets = bp.alignmentTensor(ALL, padded=False)
    assert torch.equal(one, torch.cat(rows)) and offsets[-1] == samples
    bp.close()


@pytest.mark.parametrize("hop", [1, 7, 256])
def test_hops_phases_dtypes_and_layouts(groups, hop):
    """Hops 1, 7, 256 with phases 0 and hop - 1; int32 and int64; padded with two pad values, and packed; repeated and reversed utterances
    and columns."""
    import torch
    import nvspeechplayer_amd as eng
    spec, cases = groups[-1]
    bp = eng.BatchPlayer(22050)
    bp.setIpa(**spec)
    n = len(cases)
    picks = [None, list(range(n))[::-1], [n - 1, 0, 0, 3, n - 1, 2, 3]]
    columns = [ALL[::-1] + [0, 0, 7], ["phoneme"], ["remaining", "phoneme", "unit"]] + ([ALL, [6, 5]] if hop > 1 else [])
    for phase in sorted({0, hop - 1}):
        for sel in picks:
            order = list(range(n)) if sel is None else sel
            for cols in columns:
                idx = [COLUMNS.index(c) if isinstance(c, str) else c for c in cols]
                want = [cases[u].dense(idx, hop, phase) for u in order]
                for dtype in (torch.int32, torch.int64):
                    assert check_packed(bp, cases, idx, hop, phase, dtype, sel) == sum(len(w) for w in want)
                    for pad in (-1, 12345):
                        got, steps = bp.alignmentTensor(cols, hop=hop, phase=phase, utterances=sel, dtype=dtype, pad=pad)
                        assert got.dtype == dtype and list(steps) == [len(w) for w in want] and got.shape == (len(order), max(len(w) for w in want), len(idx))
                        got = got.cpu().numpy()
                        for r, w in enumerate(want):
                            assert np.array_equal(got[r, :len(w)], w) and np.all(got[r, len(w):] == pad), (r, hop, phase, cols)
    # a phase beyond every utterance: no steps
    got, steps = bp.alignmentTensor(ALL, hop=hop, phase=10 ** 9)
    assert got.shape == (n, 0, 8) and not steps.any()
    bp.close()


def test_unit_tensor(groups):
    """samples sum to the utterance's length, steps to the row's step count for every hop and phase, firstSample is the timeline at the
    units' first frames, the whole table equals unit_table; by="frame" agrees with the dense export."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(22050)
    for spec, cases in groups[:2]:
        bp.setIpa(**spec)
        n = len(cases)
        for by in ("unit", "frame"):
            counts = bp.unitCounts(by=by)
            assert list(counts) == [len(unit_first(c.labels)) - 1 if by == "unit" else len(c.labels) for c in cases]
            for hop, phase in ((1, 0), (7, 0), (7, 6), (256, 0), (256, 255)):
                for sel in (None, [n - 1, 1, 1, 0]):
                    order = list(range(n)) if sel is None else sel
                    units, cnt = bp.unitTensor(hop=hop, phase=phase, utterances=sel, by=by, pad=-5)
                    packed, offsets = bp.unitTensor(hop=hop, phase=phase, utterances=sel, by=by, padded=False)
                    assert units.dtype == torch.int64 and units.shape == (len(order), int(counts[order].max()), 7) and list(cnt) == list(counts[order])
                    units, packed, offsets = units.cpu().numpy(), packed.cpu().numpy(), offsets.numpy()
                    for r, u in enumerate(order):
                        c = cases[u]
                        want = unit_table(c.first, c.labels, hop, phase, by)
                        got = units[r, :counts[u]]
                        assert np.array_equal(got, want), (u, hop, phase, by)
                        assert np.all(units[r, counts[u]:] == -5) and np.array_equal(packed[offsets[r]:offsets[r + 1]], want)
                        assert got[:, UNIT_COLUMNS.index("samples")].sum() == c.length == bp.utteranceSamples(u)
                        assert got[:, UNIT_COLUMNS.index("steps")].sum() == c.steps(hop, phase)
                        first, _ = bp.timeline(u)
                        edges = unit_first(c.labels) if by == "unit" else np.arange(len(c.labels) + 1)
                        assert np.array_equal(got[:, 3], first[edges[:-1]])
        # per frame: the dense export's `frame` column visits entry i on exactly its `steps` steps, with its phoneme
        for hop, phase in ((1, 0), (7, 3)):
            table, cnt = bp.unitTensor(hop=hop, phase=phase, by="frame", pad=0)
            dense, steps = bp.alignmentTensor(["frame", "phoneme"], hop=hop, phase=phase)
            table, dense = table.cpu().numpy(), dense.cpu().numpy()
            for u in range(n):
                d = dense[u, :steps[u]]
                assert np.array_equal(np.bincount(d[:, 0], minlength=int(cnt[u])), table[u, :cnt[u], 6])
                assert np.array_equal(table[u, d[:, 0], 0], d[:, 1])
        # units: gaps and aspirations are counted to their stops
        table, cnt = bp.unitTensor()
        flags = table[..., 1].cpu().numpy()
        assert ((flags >= 0) & (flags & GAP != 0)).any() and ((flags >= 0) & (flags & PUFF != 0)).any()
    bp.close()


def test_voices_per_text_and_labelled_records_give_the_same_tensors(groups):
    """setIpaVoices with a voice per text, and setRecordsLabelled from a records object, against setIpa: labels do not depend on the voice."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import ipa
    spec, cases = groups[0]
    n = len(cases)
    bp = eng.BatchPlayer(22050)
    bp.setIpa(**spec)
    dense = bp.alignmentTensor(ALL, hop=3, phase=1, padded=False)[0]
    units = bp.unitTensor(hop=256, padded=False)[0]
    voice = (np.arange(n) % 5 - 1).astype(np.int32)
    bp.setIpa(voice=voice, **spec)
    assert bp.hasLabels
    assert torch.equal(bp.alignmentTensor(ALL, hop=3, phase=1, padded=False)[0], dense) and torch.equal(bp.unitTensor(hop=256, padded=False)[0], units)
    pk = ipa.records_for_batch(spec["texts"], speed=spec["speed"], basePitch=spec["basePitch"], inflection=spec["inflection"], clauseType=spec["clauseType"], voice=voice)
    other = eng.BatchPlayer(22050)
    other.setRecords(pk["shapes"], pk["list_start"], pk["records"], listOf=pk["list_of"], labels=pk["labels"])
    assert other.hasLabels
    assert torch.equal(other.alignmentTensor(ALL, hop=3, phase=1, padded=False)[0], dense) and torch.equal(other.unitTensor(hop=256, padded=False)[0], units)
    # the same records without labels: none
    other.setRecords(pk["shapes"], pk["list_start"], pk["records"], listOf=pk["list_of"])
    assert not other.hasLabels
    # labels whose units do not count from 0 by steps of at most one are refused, and the batch before stays
    other.setRecords(pk["shapes"], pk["list_start"], pk["records"], listOf=pk["list_of"], labels=pk["labels"])
    bad = pk["labels"].copy()
    bad["unit"][3] += 2
    with pytest.raises(RuntimeError, match="units"):
        other.setRecords(pk["shapes"], pk["list_start"], pk["records"], listOf=pk["list_of"], labels=bad)
    # ... a list that opens with unit -1 (a whole list of them too), and a negative phoneme id on a frame that opens a unit
    ls = pk["list_start"]
    for spoil in (lambda b: b["unit"].__setitem__(ls[1], -1), lambda b: b["unit"].__setitem__(slice(ls[1], ls[2]), -1),
                  lambda b: b["unit"].__setitem__(0, 1), lambda b: b["phoneme"].__setitem__(ls[2], -1),
                  lambda b: b["phoneme"].__setitem__(int(np.flatnonzero(np.diff(pk["labels"]["unit"]) == 1)[0]) + 1, -3)):
        bad = pk["labels"].copy()
        spoil(bad)
        assert not np.array_equal(bad, pk["labels"])
        with pytest.raises(RuntimeError, match="units"):
            other.setRecords(pk["shapes"], pk["list_start"], pk["records"], listOf=pk["list_of"], labels=bad)
        assert other.hasLabels
    assert torch.equal(other.alignmentTensor(ALL, hop=3, phase=1, padded=False)[0], dense)
    assert other.hasLabels and torch.equal(other.unitTensor(hop=256, padded=False)[0], units)
    other.close()
    bp.close()


def test_configs2_at_full_size_labels_are_per_list():
    """BASELINE configs[2], 65 536 utterances over 512 lists: a seeded sample of rows against the walk (every sample, all columns), and on
    the device for ALL rows: the units' samples sum to the lengths and their steps to the step counts."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import ipa, workloads
    n = 65536
    spec = workloads.cfg2_spec(n)
    bp = eng.BatchPlayer(22050)
    bp.setIpa(**spec)
    assert bp.hasLabels
    sample = np.sort(np.random.default_rng(9).choice(n, 48, replace=False))
    sub = dict(spec, textOf=spec["textOf"][sample], basePitch=spec["basePitch"][sample])
    cases = host_cases(**sub)
    got, offsets = bp.alignmentTensor(ALL, utterances=sample, padded=False)
    got, offsets = got.cpu().numpy(), offsets.numpy()
    for r, c in enumerate(cases):
        assert np.array_equal(got[offsets[r]:offsets[r + 1]], c.dense(ALL)), int(sample[r])
    lens = torch.from_numpy(bp._lengths().astype(np.int64)).to("cuda:%d" % bp.device)
    for hop, phase in ((256, 0), (1, 0), (7, 6)):
        units, counts = bp.unitTensor(hop=hop, phase=phase, pad=0)
        assert units.shape[0] == n and int(counts.min()) > 5
        assert torch.equal(units[..., 4].sum(dim=1), lens)
        assert torch.equal(units[..., 6].sum(dim=1), torch.clamp((lens - phase + hop - 1) // hop, min=0))
        del units
    # framewise phoneme ids at a hop for all rows: as many steps per row as the units say, ids within the table
    dense, steps = bp.alignmentTensor("phoneme", hop=256, dtype=torch.int32)
    assert dense.shape == (n, int(steps.max()), 1) and int(dense.max()) == len(ipa.phonemeSymbols()) - 1 and int(dense.min()) == -1
    assert torch.equal((dense[..., 0] >= 0).sum(dim=1).cpu(), steps)
    bp.close()


def test_ordering_with_streams_set_calls_and_synthesis(groups):
    """An export queued behind a non-default torch stream; a set call issued right after an export (the export's result is unchanged);
    an export before any synthesis launch; PCM digests of the batch identical with and without exports."""
    import torch
    import nvspeechplayer_amd as eng
    (spec_a, cases_a), (spec_b, cases_b) = groups[0], groups[1]
    plain = eng.BatchPlayer(22050)
    plain.setIpa(**spec_a)
    plain.synthesize()
    digest = plain.digest(per_utterance=True)
    plain.close()
    bp = eng.BatchPlayer(22050)
    dev = "cuda:%d" % bp.device
    bp.setIpa(**spec_a)
    want_a = np.concatenate([c.dense(ALL) for c in cases_a])
    want_b = np.concatenate([c.dense(ALL) for c in cases_b])
    # before any synthesis launch, on a stream of the caller's that is busy with work of its own
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        busy = torch.ones(1 << 24, device=dev)
        for _ in range(20):
            busy = busy * 1.0001
        got, _ = bp.alignmentTensor(ALL, padded=False)
        units, _ = bp.unitTensor(hop=256, padded=False)
        after = got.sum()                      # (queued behind the export on the same stream)
    # a set call right away, with no host wait in between: it waits for the exports on the device
    bp.setIpa(**spec_b)
    got_b, _ = bp.alignmentTensor(ALL, padded=False)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want_a) and int(after) == int(want_a.sum())
    assert np.array_equal(units.cpu().numpy(), np.concatenate([unit_table(c.first, c.labels, 256) for c in cases_a]))
    assert np.array_equal(got_b.cpu().numpy(), want_b)
    # exports around the synthesis do not touch the PCM
    bp.setIpa(**spec_a)
    bp.alignmentTensor(ALL, hop=5)
    bp.synthesize(wait=False)
    mid, _ = bp.alignmentTensor(ALL, padded=False)
    bp.wait()
    bp.unitTensor(by="frame")
    whole, per = bp.digest(per_utterance=True)
    assert whole == digest[0] and np.array_equal(per, digest[1])
    assert np.array_equal(mid.cpu().numpy(), want_a)
    bp.close()


def test_refusals(groups):
    """No labels on this batch, a bad column, hop < 1, a pointer that is not device memory of this device, a capacity too small: a negative
    code, SPEECHPLAYER_ERR_ARGUMENT and a message; nothing written.  After setUtterances on the same player hasLabels is False."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native, ipa
    L = _native.load()
    spec, cases = groups[0]
    bp = eng.BatchPlayer(22050)
    bp.setIpa(**spec)
    dev = "cuda:%d" % bp.device
    steps = sum(c.length for c in cases)
    out = torch.full((steps + 16,), -77, dtype=torch.int64, device=dev)
    cols = np.array([0], np.int32)
    stream = torch.cuda.current_stream(bp.device).cuda_stream

    def dense(columns=cols, n_cols=1, hop=1, phase=0, ptr=None, fmt=0, stride=0, capacity=None, utt=None, n_utt=0):
        return L.speechPlayer_batch_exportAlignment(bp._h, utt, n_utt, columns.ctypes.data, n_cols, hop, phase, out.data_ptr() if ptr is None else ptr,
                                                    fmt, stride, -1, steps if capacity is None else capacity, stream)

    def units(hop=256, phase=0, ptr=None, stride=0, capacity=None):
        return L.speechPlayer_batch_exportUnits(bp._h, None, 0, hop, phase, 0, out.data_ptr() if ptr is None else ptr, stride, -1,
                                                out.numel() if capacity is None else capacity, stream)

    def refused(rc, word):
        assert rc == -1 and L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and word in L.speechPlayer_lastError().decode(), (rc, L.speechPlayer_lastError())

    assert dense() == steps
    host = np.zeros(steps, np.int64)
    pinned = eng.speechPlayer.host_array((steps,), np.int64)
    refused(dense(columns=np.array([8], np.int32)), "columns[0] = 8")
    refused(dense(columns=np.array([0, -1], np.int32), n_cols=2, capacity=2 * steps), "columns[1] = -1")
    refused(dense(n_cols=0), "columns")
    refused(dense(hop=0), "hop")
    refused(dense(phase=-1), "phase")
    refused(dense(fmt=2), "format")
    refused(dense(capacity=steps - 1), "capacity")
    refused(dense(stride=1), "rowStride")
    refused(dense(ptr=host.ctypes.data), "exportAlignment")
    refused(dense(ptr=pinned.ctypes.data), "not device memory")
    refused(dense(ptr=out.data_ptr() + 4), "aligned")
    bad = np.array([len(cases)], np.int64)
    refused(dense(utt=bad.ctypes.data, n_utt=1), "not an utterance")
    n_units = int(bp.unitCounts().sum())
    assert units() == 7 * n_units
    refused(units(hop=0), "hop")
    refused(units(capacity=7 * n_units - 1), "capacity")
    refused(units(stride=1), "rowStride")
    refused(units(ptr=host.ctypes.data), "exportUnits")
    if torch.cuda.device_count() > 1:
        far = torch.zeros(steps, dtype=torch.int64, device="cuda:%d" % ((bp.device + 1) % torch.cuda.device_count()))
        refused(dense(ptr=far.data_ptr()), "memory of device")
    torch.cuda.synchronize()
    assert int(out[steps:].min()) == -77 == int(out[steps:].max())            # nothing past what the two good calls wrote
    with pytest.raises(ValueError):
        bp.alignmentTensor(ALL, utterances=[len(cases)])
    with pytest.raises(ValueError):
        bp.unitTensor(by="syllable")
    # a batch set any other way has no labels, and says so
    pk = ipa.frames_for_batch(spec["texts"][:3])
    bp.setUtterances(pk["frame_start"], pk["frames"], pk["min"], pk["fade"], None, pk["isnull"])
    assert not bp.hasLabels
    refused(dense(capacity=out.numel()), "no labels")
    refused(units(), "no labels")
    assert L.speechPlayer_batch_unitCounts(bp._h, None, 0, 0, None) == -1 and b"no labels" in L.speechPlayer_lastError()
    for call in (lambda: bp.alignmentTensor("phoneme"), lambda: bp.unitTensor(), lambda: bp.unitCounts()):
        with pytest.raises(RuntimeError, match="no labels"):
            call()
    bp.trackTensor("frame")                                                   # (the track export does not need them)
    bp.setIpa(**spec)
    assert bp.hasLabels and dense() == steps
    bp.close()
