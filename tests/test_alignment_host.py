"""Phoneme labels on the host (include/speechPlayer_batch.h: speechPlayer_ipa_labels, speechPlayer_records_labels and the alignment
exports' declarations): the producer's labels against what the REFERENCE's front-end says about every frame of the 126 captured cases
(tests/golden/ref_segments.npz, recorded from ipa.IPAToPhonemes + correctHPhonemes by tests/golden/make_alignment_golden.py), their
units and text offsets, the labels of a records object, the producer's sanitizer run over the label pass -- and `align_walk` /
`unit_table`, the comparands of tests/test_gpu_alignment.py.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import scenarios
from tests.test_timeline_host import plan_timeline, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT = 1
CLAUSES = {0: ".", 1: ",", 2: "?", 3: "!", 4: None}
NEW_ENTRIES = ("speechPlayer_ipa_labels", "speechPlayer_records_labels", "speechPlayer_batch_setRecordsLabelled", "speechPlayer_batch_hasLabels",
               "speechPlayer_batch_exportAlignment", "speechPlayer_batch_exportUnits", "speechPlayer_batch_unitCounts")
COLUMNS = ["phoneme", "stress", "flags", "unit", "textOffset", "frame", "position", "remaining"]
UNIT_COLUMNS = ["phoneme", "flags", "textOffset", "firstSample", "samples", "firstStep", "steps"]
STRESS, TIED_TO, TIED_FROM, LONG, WORD_START, SYLLABLE_START, GAP, PUFF = 3, 4, 8, 16, 32, 64, 128, 256


def unit_first(labels):
    """First frame of every unit of one utterance, and one past the end: units count from 0 and rise by at most one."""
    unit = np.asarray(labels["unit"], dtype=np.int64)
    assert len(unit) == 0 or (unit[0] == 0 and np.all((np.diff(unit) == 0) | (np.diff(unit) == 1)))
    return np.concatenate([np.flatnonzero(np.diff(unit, prepend=-1)), [len(unit)]]).astype(np.int64)


def align_walk(firstSample, labels, hop=1, phase=0):
    """The framewise labels of one utterance at the samples phase + j * hop, restated: firstSample[n + 1] is the utterance's timeline
    (speechPlayer_planTimeline / BatchPlayer.timeline: request k is dequeued on sample firstSample[k], firstSample[n] is the length --
    held to test_timeline_host.walk and to the oracle pulled sample by sample in tests/test_timeline_host.py, and to walk again below),
    labels its n labels.  The request in effect on sample t is the last one dequeued on or before t.  -> {column: int64 [steps]}."""
    first = np.asarray(firstSample, dtype=np.int64)
    n = len(first) - 1
    t = np.arange(phase, first[-1], hop, dtype=np.int64)
    k = np.searchsorted(first[:n], t, side="right") - 1
    uf = unit_first(labels)
    unit = np.asarray(labels["unit"], dtype=np.int64)[k]
    flags = np.asarray(labels["flags"], dtype=np.int64)[k]
    return {"phoneme": np.asarray(labels["phoneme"], dtype=np.int64)[k], "stress": flags & STRESS, "flags": flags, "unit": unit,
            "textOffset": np.asarray(labels["textOffset"], dtype=np.int64)[k], "frame": k,
            "position": t - first[uf[unit]], "remaining": first[uf[unit + 1]] - t}


def unit_table(firstSample, labels, hop=1, phase=0, by="unit"):
    """The segment table of one utterance, restated: -> int64 [entries, 7] (UNIT_COLUMNS)."""
    first = np.asarray(firstSample, dtype=np.int64)
    n = len(first) - 1
    edges = unit_first(labels) if by == "unit" else np.arange(n + 1)
    below = lambda x: (x - phase + hop - 1) // hop if x > phase else 0      # steps phase + j * hop below sample x
    rows = []
    for a, e in zip(edges[:-1], edges[1:]):
        fl = np.asarray(labels["flags"][a:e], dtype=np.int64)
        own = a + int(np.argmax((fl & (GAP | PUFF)) == 0))      # the entry's frame that is neither gap nor aspiration (else its first)
        rows.append([int(labels["phoneme"][own]), int(np.bitwise_or.reduce(fl)), int(labels["textOffset"][own]), int(first[a]), int(first[e] - first[a]),
                     below(int(first[a])), below(int(first[e])) - below(int(first[a]))])
    return np.array(rows, dtype=np.int64).reshape(len(rows), 7)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(scenarios.GOLDEN, "ref_frames.npz"))
    s = np.load(os.path.join(scenarios.GOLDEN, "ref_segments.npz"))
    return z, s


def cases(z):
    lines = [b.decode("utf8") for b in z["ipa_lines"]]
    for i, meta in enumerate(z["ipa_case_meta"]):
        yield i, lines[int(meta[0])], float(meta[1]), CLAUSES[int(meta[2])], float(meta[3]), float(meta[4])


def test_entry_points_are_declared_exported_and_bound():
    from nvspeechplayer_amd import _native
    header = open(os.path.join(ROOT, "include", "speechPlayer_batch.h")).read()
    L = _native.load()
    for name in NEW_ENTRIES:
        assert name + "(" in header, name
        assert name in _native.EXPORTS, name
        assert getattr(L, name).argtypes, name
    for q, name in enumerate(COLUMNS):
        macro = "SPEECHPLAYER_ALIGN_" + {"textOffset": "TEXT_OFFSET"}.get(name, name.upper())
        assert any(line.split()[:3] == ["#define", macro, str(q)] for line in header.splitlines()), macro
    from nvspeechplayer_amd import ipa, speechPlayer
    assert speechPlayer.ALIGN_COLUMNS == COLUMNS and speechPlayer.UNIT_COLUMNS == UNIT_COLUMNS
    assert ipa.LABEL_DTYPE.itemsize == 16
    assert (ipa.LABEL_STRESS_MASK, ipa.LABEL_TIED_TO, ipa.LABEL_TIED_FROM, ipa.LABEL_LONG, ipa.LABEL_WORD_START, ipa.LABEL_SYLLABLE_START,
            ipa.LABEL_GAP, ipa.LABEL_PUFF) == (STRESS, TIED_TO, TIED_FROM, LONG, WORD_START, SYLLABLE_START, GAP, PUFF)
    for name, value in (("TIED_TO", 4), ("TIED_FROM", 8), ("LONG", 16), ("WORD_START", 32), ("SYLLABLE_START", 64), ("GAP", 128), ("PUFF", 256)):
        assert any(line.replace(",", " ").split()[:3] == ["SPEECHPLAYER_LABEL_" + name, "=", str(value)] for line in header.splitlines()), name


def test_labels_equal_the_reference_front_end_on_all_126_cases(golden):
    """Frame count, phoneme id, gap / aspiration, stress and every prosodic bit of speechPlayer_ipa_labels against the reference's own
    phoneme list: zero mismatches.  The frame count is speechPlayer_ipa_frames's for the same call."""
    from nvspeechplayer_amd import ipa
    z, s = golden
    names = [b.decode("utf8") for b in z["phoneme_names"]]
    symbols = ipa.phonemeSymbols()
    assert symbols == names + ["<gap>", "<sil>"]
    count = len(names)
    start = s["seg_start"]
    assert len(start) == 127 and np.array_equal(start, z["ipa_start"])
    mismatches, frames = [], 0
    for i, text, speed, clause, pitch, infl in cases(z):
        lab = ipa.labels(text)
        a, e = int(start[i]), int(start[i + 1])
        n_frames = len(ipa.frame_arrays(text, speed=speed, basePitch=pitch, inflection=infl, clauseType=clause)[1])
        if not len(lab) == e - a == n_frames:
            mismatches.append((i, "frames", len(lab), e - a, n_frames))
            continue
        gap = s["seg_gap"][a:e].astype(bool)
        want = {
            "phoneme": np.where(gap, count, s["seg_key"][a:e]),
            "gap": gap, "puff": s["seg_puff"][a:e].astype(bool), "stress": s["seg_stress"][a:e],
            "tied_to": s["seg_tied_to"][a:e].astype(bool), "tied_from": s["seg_tied_from"][a:e].astype(bool), "long": s["seg_lengthened"][a:e].astype(bool),
            "word": s["seg_word_start"][a:e].astype(bool), "syllable": s["seg_syllable_start"][a:e].astype(bool),
        }
        fl = lab["flags"]
        got = {"phoneme": lab["phoneme"], "gap": (fl & GAP) != 0, "puff": (fl & PUFF) != 0, "stress": fl & STRESS, "tied_to": (fl & TIED_TO) != 0,
               "tied_from": (fl & TIED_FROM) != 0, "long": (fl & LONG) != 0, "word": (fl & WORD_START) != 0, "syllable": (fl & SYLLABLE_START) != 0}
        for key in want:
            if not np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)):
                mismatches.append((i, key))
        # the reference's gap is its only silence; `_char` is the first character of the table key, None for an aspiration (a copy of /h/)
        assert np.array_equal(s["seg_silence"][a:e].astype(bool), gap)
        for k in range(e - a):
            ch = int(s["seg_char"][a + k])
            if want["gap"][k]:
                assert ch == -1 and s["seg_key"][a + k] == -1
            elif want["puff"][k]:
                assert ch == -1 and names[int(lab["phoneme"][k])] == "h"
            elif symbols[int(lab["phoneme"][k])][0] != names[ch]:
                mismatches.append((i, k, "char"))
        assert np.array_equal(z["ipa_isnull"][a:e].astype(bool), lab["phoneme"] >= count), i
        frames += e - a
    assert not mismatches, mismatches[:10]
    assert frames == int(start[-1]) == 2604
    # the captured cases exercise every bit but tied-from (the table joins every tied pair of theirs into one row: the reference sets
    # `_tiedFrom` nowhere in them); test_units_and_text_offsets has pairs the table does not join
    every = np.bitwise_or.reduce(np.concatenate([ipa.labels(t)["flags"] for _, t, *_ in cases(z)]))
    assert every == 511 - TIED_FROM and not s["seg_tied_from"].any()


def test_units_and_text_offsets(golden):
    """unit is non-decreasing; a gap shares the unit of the stop after it, an aspiration that of the stop before it; for every frame that
    is not inserted the text at textOffset starts with the UTF-8 symbol of its row; inserted frames have -1."""
    from nvspeechplayer_amd import ipa
    z, _ = golden
    symbols = ipa.phonemeSymbols()
    texts = sorted({t for _, t, *_ in cases(z)}) + ["t͡ʃɑ #pɑː", "ˈt͡ʃɑ", "a͡ɪ t͡s", " ɑː  ˌpliːz", "", "#7 "]
    seen_gap = seen_puff = seen_tie_row = seen_tied_pair = seen_long_row = 0
    for text in texts:
        lab = ipa.labels(text)
        raw = text.encode("utf8")
        unit = lab["unit"].astype(np.int64)
        if len(lab) == 0:
            continue
        assert unit[0] == 0 and np.all((np.diff(unit) == 0) | (np.diff(unit) == 1)), text
        inserted = (lab["flags"] & (GAP | PUFF)) != 0
        assert np.all(lab["textOffset"][inserted] == -1), text
        assert np.array_equal(unit[~inserted], np.arange(np.count_nonzero(~inserted))), text      # one unit per text symbol
        last = -1
        for k in range(len(lab)):
            if lab["flags"][k] & GAP:
                assert not inserted[k + 1] and unit[k] == unit[k + 1] and (k == 0 or unit[k - 1] == unit[k] - 1), (text, k)
                seen_gap += 1
            elif lab["flags"][k] & PUFF:
                assert not inserted[k - 1] and unit[k] == unit[k - 1] and (k + 1 == len(lab) or unit[k + 1] == unit[k] + 1), (text, k)
                seen_puff += 1
            else:
                sym = symbols[int(lab["phoneme"][k])].encode("utf8")
                off = int(lab["textOffset"][k])
                assert off > last and raw[off:off + len(sym)] == sym, (text, k, off, sym)
                last = off
                seen_tie_row += "͡" in sym.decode("utf8")
                seen_long_row += bool(lab["flags"][k] & LONG)          # (a symbol before a length mark; the table has no lengthened row of its own)
                seen_tied_pair += bool(lab["flags"][k] & TIED_FROM) and "͡" not in sym.decode("utf8")
    assert seen_gap > 20 and seen_puff > 5 and seen_tie_row > 0 and seen_tied_pair > 0 and seen_long_row > 0
    # by hand: gap t͡ʃ ɑ | gap p (aspiration) ɑː -- "#" is unknown and skipped
    lab = ipa.labels("t͡ʃɑ #pɑː")
    assert [symbols[p] for p in lab["phoneme"]] == ["<gap>", "t͡ʃ", "ɑ", "<gap>", "p", "h", "ɑ"]
    assert list(lab["unit"]) == [0, 0, 1, 2, 2, 2, 3]
    assert list(lab["textOffset"]) == [-1, 0, 5, -1, 9, -1, 10]
    assert list(lab["flags"]) == [GAP, TIED_TO | WORD_START | SYLLABLE_START, 0, GAP, WORD_START | SYLLABLE_START, PUFF, LONG]
    lab = ipa.labels("ˈhɛləʊ ˌwɜːld")
    assert (lab["flags"][0] & STRESS) == 1 and 2 in list(lab["flags"] & STRESS)
    # invalid UTF-8 is an unknown symbol: the offsets of what follows still count bytes
    from nvspeechplayer_amd import _native
    L = _native.load()
    off = np.zeros(8, np.int32)
    assert L.speechPlayer_ipa_labels(b"h\xff\xfe\xc3\xa6l", None, None, None, off.ctypes.data, 8) == 3 and list(off[:3]) == [0, 3, 5]


def test_records_labels_are_parallel_to_the_records_and_ignore_pitch_and_voice(golden):
    """A multi-voice, multi-pitch speechPlayer_ipa_records call: labels per LIST, parallel to the records (silence where the record is
    silence, the trailing silence last); lists of one (text, clause) with another pitch or voice carry equal labels, equal to
    speechPlayer_ipa_labels plus the silence."""
    from nvspeechplayer_amd import ipa
    z, _ = golden
    lines = [b.decode("utf8") for b in z["ipa_lines"]]
    texts, pitch, clause, voice = [], [], [], []
    for li in (0, 3, 9, 12):
        for p, c, v in ((100.0, ".", -1), (140.0, ".", -1), (100.0, ".", 2), (100.0, "?", 0), (100.0, ".", -1)):
            texts.append(lines[li]); pitch.append(p); clause.append(c); voice.append(v)
    pk = ipa.records_for_batch(texts, basePitch=pitch, clauseType=clause, voice=voice)
    ls, lo, lab, rec = pk["list_start"], pk["list_of"], pk["labels"], pk["records"]
    assert lab.dtype == ipa.LABEL_DTYPE and len(lab) == len(rec) == ls[-1]
    assert len(ls) - 1 == 16 and lo[4] == lo[0] and len(set(lo)) == 16            # the repeat shares its list
    count = len(ipa.phonemeSymbols()) - 2
    assert np.array_equal(rec["shape"] == ipa.RECORD_SILENCE, lab["phoneme"] >= count)
    for u, text in enumerate(texts):
        own = lab[ls[lo[u]]:ls[lo[u] + 1]]
        one = ipa.labels(text)
        assert np.array_equal(own[:-1], one), u
        assert tuple(own[-1]) == (count + 1, 0, (one["unit"].max() + 1) if len(one) else 0, -1), u
        first = lab[ls[lo[u - u % 5]]:ls[lo[u - u % 5] + 1]]
        assert np.array_equal(own, first), u
    # no trailing silence: the labels alone; an empty text: an empty list
    pk = ipa.records_for_batch(["hælou", ""], trailing_silence_ms=None)
    assert np.array_equal(pk["labels"], ipa.labels("hælou")) and list(pk["list_start"]) == [0, len(ipa.labels("hælou")), len(ipa.labels("hælou"))]


def test_label_pass_under_sanitizers(tmp_path):
    """The producer's sanitizer run (CPU build of the same source, AddressSanitizer + UBSan) over the label pass: 40 000 random symbol
    sequences through speechPlayer_ipa_labels, a packed batch through speechPlayer_records_labels and the batch entry points, setText among them."""
    exe = str(tmp_path / "fuzz_labels")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-DSPEECHPLAYER_LABELLED_SET", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "fuzz_labels.cpp"),
                           os.path.join(ROOT, "nvspeechplayer_amd", "csrc", "frame_producer.cpp"), "-o", exe])
    # speechPlayer_batch_setText's labels too (units counting on through the clauses, no text offsets, one silence per text), over a
    # stand-in for eSpeak NG that answers a clause with the clause itself
    fake = str(tmp_path / "libfake_espeak.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", os.path.join(ROOT, "tests", "native", "fake_espeak.c"), "-o", fake])
    out = subprocess.check_output([exe, fake], stderr=subprocess.STDOUT).decode()
    assert out.startswith("ok ") and "runtime error" not in out and "AddressSanitizer" not in out, out


def test_align_walk_is_held_to_the_frame_manager_walk(golden):
    """The comparand of the GPU tests: its `frame` column is the request test_timeline_host.walk -- the reference's frame manager, sample by
    sample -- has most recently dequeued, on every sample; position and remaining count within the unit; the table's steps add up."""
    from nvspeechplayer_amd import ipa
    z, _ = golden
    lines = [b.decode("utf8") for b in z["ipa_lines"]]
    count = len(ipa.phonemeSymbols()) - 2
    for text in (lines[0], lines[9], "p t k"):
        pk = ipa.frames_for_batch([text])
        n = len(pk["min"])
        _, _, number = walk(pk["frames"], pk["min"], pk["fade"], np.full(n, -1), pk["isnull"])
        first, length = plan_timeline(pk["frame_start"], pk["min"], pk["fade"])
        first = np.concatenate([first, length])
        lab = np.concatenate([ipa.labels(text), np.array([(count + 1, 0, ipa.labels(text)["unit"].max() + 1, -1)], ipa.LABEL_DTYPE)])
        got = align_walk(first, lab)
        assert len(number) == length[0] and np.array_equal(got["frame"], number)
        assert np.array_equal(got["phoneme"], lab["phoneme"][number]) and got["phoneme"][-1] == count + 1
        uf = unit_first(lab)
        for u in range(len(uf) - 1):
            on = got["unit"] == u
            span = int(first[uf[u + 1]] - first[uf[u]])
            assert np.count_nonzero(on) == span
            assert np.array_equal(got["position"][on], np.arange(span)) and np.array_equal(got["remaining"][on], span - np.arange(span))
        for hop, phase in ((1, 0), (7, 6), (256, 0), (256, 255), (5, 100000)):
            w = align_walk(first, lab, hop, phase)
            for c in COLUMNS:
                assert np.array_equal(w[c], got[c][phase::hop]), (c, hop, phase)
            for by in ("unit", "frame"):
                t = unit_table(first, lab, hop, phase, by)
                assert t[:, 4].sum() == length[0] and t[:, 6].sum() == len(w["frame"]) and np.array_equal(t[:, 3], np.cumsum(t[:, 4]) - t[:, 4])
                assert np.array_equal(t[:, 5], np.cumsum(t[:, 6]) - t[:, 6])
                steps_of = w["unit"] if by == "unit" else w["frame"]
                assert np.array_equal(np.bincount(steps_of, minlength=len(t)), t[:, 6])
    # by hand: a vowel of 5 samples with a fade of 2, then silence (test_timeline_host.test_walk_quirks_by_hand): samples 0..5 and 6..8
    lab = np.array([(7, WORD_START | SYLLABLE_START | 1, 0, 0), (count + 1, 0, 1, -1)], ipa.LABEL_DTYPE)
    w = align_walk([0, 6, 9], lab)
    assert list(w["frame"]) == [0] * 6 + [1] * 3 and list(w["position"]) == [0, 1, 2, 3, 4, 5, 0, 1, 2] and list(w["remaining"]) == [6, 5, 4, 3, 2, 1, 3, 2, 1]
    assert unit_table([0, 6, 9], lab, 4, 1).tolist() == [[7, 97, 0, 0, 6, 0, 2], [count + 1, 0, -1, 6, 3, 2, 0]]


def test_alignment_request_checks_and_refusals_without_a_batch():
    import torch
    from nvspeechplayer_amd import _native
    from nvspeechplayer_amd.speechPlayer import check_alignment_request
    cols, hop, phase, fmt = check_alignment_request(["phoneme", "remaining", 3, "phoneme"], 256, 3, None)
    assert list(cols) == [0, 7, 3, 0] and cols.dtype == np.int32 and (hop, phase, fmt) == (256, 3, 0)
    assert check_alignment_request("unit", 1, 0, torch.int32)[3] == 1
    for bad, exc in ((["phonem"], KeyError), ([8], ValueError), ([-1], ValueError), ([], ValueError)):
        with pytest.raises(exc):
            check_alignment_request(bad, 1, 0, None)
    with pytest.raises(ValueError):
        check_alignment_request([0], 0, 0, None)
    with pytest.raises(ValueError):
        check_alignment_request([0], 1, -1, None)
    with pytest.raises(TypeError):
        check_alignment_request([0], 1, 0, torch.float32)
    L = _native.load()
    cols = np.array([0], np.int32)
    assert L.speechPlayer_batch_exportAlignment(None, None, 0, cols.ctypes.data, 1, 1, 0, None, 1, 0, -1, 0, None) == -1
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"exportAlignment" in L.speechPlayer_lastError()
    assert L.speechPlayer_batch_exportUnits(None, None, 0, 1, 0, 0, None, 0, -1, 0, None) == -1
    assert L.speechPlayer_lastErrorCode() == ERR_ARGUMENT and b"exportUnits" in L.speechPlayer_lastError()
    assert L.speechPlayer_batch_unitCounts(None, None, 0, 0, None) == -1 and L.speechPlayer_batch_hasLabels(None) == -1
    assert L.speechPlayer_records_labels(None, None, None) == -1
