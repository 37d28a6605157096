#!/usr/bin/env python3
"""Generate tests/golden/ref_segments.npz: what the REFERENCE's front-end says about every frame of the 126 cases of ref_frames.npz.

Runs only where the reference's checkout can be imported (as make_golden.py: its ipa.py, speechPlayer.py and data.py as a throw-away
package of links outside the repository).  Nothing of the reference travels as source: the output is integers.

For every case, in the order of ref_frames.npz's `ipa_case_meta` (the case list is rebuilt here the way make_golden.py builds it, and
checked against the committed file), the phoneme list of ipa.IPAToPhonemes + ipa.correctHPhonemes -- the list generateFramesAndTiming
yields one frame per entry of (reference ipa.py:336-353) -- is recorded entry by entry:

  seg_start[cases + 1]   case c owns entries seg_start[c] .. seg_start[c + 1] - 1
  seg_char               `_char` as an index into ref_frames.npz's phoneme_names; -1 where the reference has none (a pre-stop gap;
                         a post-stop aspiration, whose `_char` is None)
  seg_key                the key of the phoneme table the entry was copied from (index into phoneme_names): for an aspiration the row
                         data['h'], for a symbol matched together with its tie or length mark that two- or three-character key;
                         -1 for a gap.  The reference does not keep the key: the table's entries are tagged with their own key (a
                         '_key' item, which every .copy() the reference makes carries along) before the reference's functions run.
  seg_silence, seg_gap, seg_puff                     `_silence`, `_preStopGap`, `_postStopAspiration`
  seg_stress, seg_syllable_start, seg_word_start     `_stress` (0 when absent), `_syllableStart`, `_wordStart`
  seg_tied_to, seg_tied_from, seg_lengthened         `_tiedTo`, `_tiedFrom`, `_lengthened`

Usage:  python tests/golden/make_alignment_golden.py      (from the repository root)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NVSP_REFERENCE", "/root/reference")
EXTRA = 10           # the lines make_golden.py appends to sampleIpa.txt's eight


def import_reference():
    """ipa.py does `from . import speechPlayer`: a throw-away package of links outside the repository (make_golden.py::import_reference)."""
    tmp = tempfile.mkdtemp(prefix="nvsp_ref_")
    pkg = os.path.join(tmp, "nvsp_ref")
    os.mkdir(pkg)
    open(os.path.join(pkg, "__init__.py"), "w").close()
    for name in ("ipa.py", "speechPlayer.py", "data.py"):
        os.symlink(os.path.join(REF, name), os.path.join(pkg, name))
    sys.path.insert(0, tmp)
    from nvsp_ref import ipa
    return ipa


def case_list(n_sample_lines):
    """(line, speed, clause, pitch, inflection) of every case, as make_golden.py::main builds them."""
    cases = []
    for speed in (1.0, 0.6):
        for clause in (".", ",", "?", "!", None):
            for li in range(n_sample_lines):
                cases.append((li, speed, clause, 100.0, 0.5))
    for li in range(n_sample_lines):
        cases.append((li, 1.0, ".", 140.0, 0.5))
        cases.append((li, 1.0, ".", 70.0, 1.0))
    for xi in range(EXTRA):
        for speed, clause, pitch, infl in ((1.0, ".", 100.0, 0.5), (0.8, "?", 120.0, 0.7), (1.3, None, 90.0, 0.3)):
            cases.append((n_sample_lines + xi, speed, clause, pitch, infl))
    return cases


def main():
    ipa = import_reference()
    ref = np.load(os.path.join(HERE, "ref_frames.npz"))
    names = [n.decode("utf8") for n in ref["phoneme_names"]]
    assert names == sorted(ipa.data.keys())
    lines = [l.decode("utf8") for l in ref["ipa_lines"]]
    cases = case_list(len(lines) - EXTRA)
    code = {".": 0, ",": 1, "?": 2, "!": 3, None: 4}
    meta = np.array([(li, speed, code[clause], pitch, infl) for li, speed, clause, pitch, infl in cases], dtype=np.float64)
    assert len(cases) == 126 and np.array_equal(meta, ref["ipa_case_meta"]), "the case list no longer matches ref_frames.npz"
    # every table entry says which key it is: the copies the reference makes of an entry carry the item along
    for key, entry in ipa.data.items():
        entry["_key"] = key
    index = {n: i for i, n in enumerate(names)}
    fields = ["char", "key", "silence", "gap", "puff", "stress", "syllable_start", "word_start", "tied_to", "tied_from", "lengthened"]
    cols = {f: [] for f in fields}
    start = [0]
    for c, (li, speed, clause, pitch, infl) in enumerate(cases):
        phonemes = ipa.IPAToPhonemes(lines[li])
        ipa.correctHPhonemes(phonemes)
        assert len(phonemes) == int(ref["ipa_start"][c + 1] - ref["ipa_start"][c]), c
        for p in phonemes:
            char = p.get("_char")
            cols["char"].append(index[char] if char is not None else -1)
            cols["key"].append(index[p["_key"]] if "_key" in p else -1)
            cols["silence"].append(bool(p.get("_silence")))
            cols["gap"].append(bool(p.get("_preStopGap")))
            cols["puff"].append(bool(p.get("_postStopAspiration")))
            cols["stress"].append(int(p.get("_stress", 0)))
            cols["syllable_start"].append(bool(p.get("_syllableStart")))
            cols["word_start"].append(bool(p.get("_wordStart")))
            cols["tied_to"].append(bool(p.get("_tiedTo")))
            cols["tied_from"].append(bool(p.get("_tiedFrom")))
            cols["lengthened"].append(bool(p.get("_lengthened")))
        start.append(start[-1] + len(phonemes))
    out = {"seg_" + f: np.array(cols[f], dtype=np.int16) for f in fields}
    out["seg_start"] = np.array(start, dtype=np.int64)
    path = os.path.join(HERE, "ref_segments.npz")
    np.savez_compressed(path, **out)
    print("ref_segments.npz: %d cases, %d entries, %d bytes" % (len(cases), start[-1], os.path.getsize(path)))


if __name__ == "__main__":
    main()
