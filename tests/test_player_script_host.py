"""The script of tests/player_script.py on the host, no GPU needed: the conditions under which tests/test_gpu_player_script.py can fail.
A reused player that handed out the batch before would pass unnoticed if two neighbouring steps looked alike; a stale tail or a freed
buffer would never be met if nothing shrank or grew.  So: every step differs from the one before it in every row both have -- PCM,
lengths, index marks and speechPlayer_planTimeline's tables; every quantity the engine sizes a buffer by both shrinks (staying above
zero) and grows (past every earlier maximum) somewhere along the script; and the mixed batch holds every class the routing knows."""
import numpy as np

from tests import player_script as ps


def neighbours():
    """(earlier step, later step) for every step after the first: the step right before it, and -- where that one has fewer rows --
    also the latest step before it that has at least as many (what the rows beyond the neighbour's last would be stale from)."""
    out = []
    for k in range(1, len(ps.SCRIPT)):
        n = len(ps.built(ps.NAMES[k])["frame_start"]) - 1
        out.append((k - 1, k))
        if len(ps.built(ps.NAMES[k - 1])["frame_start"]) - 1 < n:
            j = next((j for j in range(k - 2, -1, -1) if len(ps.built(ps.NAMES[j])["frame_start"]) - 1 >= n), None)
            if j is not None:
                out.append((j, k))
    return out


def test_neighbouring_steps_differ():
    """Row u of a step against row u of the step before it (and of the last step before that with as many rows), for every u both have:
    the oracle's PCM differs by more than 1 LSB in at least 25 samples (tests/test_one_at_a_time_host.py's floor; a sample only one of the
    two rows has counts as one), and over the whole batch the lengths, the index marks and the planTimeline tables differ.  G carries
    C's frames under other seeds: the frames and tables are equal there, the PCM is not."""
    for j, k in neighbours():
        a, b = ps.NAMES[j], ps.NAMES[k]
        pa, sa, ma = ps.expected(a)
        pb, sb, mb = ps.expected(b)
        ba, bb = ps.built(a), ps.built(b)
        d = ps.rows_differing(pa, sa, pb, sb)
        if len(d):
            print("%-2s -> %-2s: %3d common rows, weakest row %d differs in %d samples" % (a, b, len(d), int(np.argmin(d)), int(d.min())))
        else:
            print("%-2s -> %-2s: no common row" % (a, b))
            assert min(len(sa), len(sb)) == 1
            continue
        n = len(d)
        (fa, la), (fb, lb) = ps.timeline(ba), ps.timeline(bb)
        if {a, b} == {"C", "G"}:
            # (a row whose utterance makes no noise does not hear its seed)
            noisy = ps.utterance_classes(bb)[:n] >= 2
            assert noisy.sum() > n // 2 and d[noisy].min() >= ps.MIN_SAMPLES, (a, b, d)
            assert np.array_equal(ba["frames"], bb["frames"], equal_nan=True) and np.array_equal(fa, fb) and np.array_equal(la, lb)
            assert not np.array_equal(ba["seeds"], bb["seeds"]) and not np.array_equal(pa, pb)
            continue
        assert d.min() >= ps.MIN_SAMPLES, (a, b, int(np.argmin(d)), int(d.min()))
        assert not np.array_equal(la[:n], lb[:n]), (a, b)
        assert not np.array_equal(ma[:n], mb[:n]), (a, b)
        assert not np.array_equal(ba["frame_start"][:n + 1], bb["frame_start"][:n + 1]) or not np.array_equal(fa[:bb["frame_start"][n]], fb[:bb["frame_start"][n]]), (a, b)
    # C and G are in the script, three steps apart
    assert ps.NAMES.index("G") - ps.NAMES.index("C") == 4
    assert ps.rows_differing(*ps.expected("C")[:2], *ps.expected("G")[:2]).max() > 1000
    # A' is A
    assert np.array_equal(ps.expected("A")[0], ps.expected("A'")[0]) and ps.SCRIPT[0].build is ps.SCRIPT[-1].build


def test_every_counted_quantity_shrinks_and_grows():
    """Frames, utterances, lists, pool samples (every utterance padded to kTile) and track entries (speechPlayer_planTracks under the
    step's options): each shrinks at least once to a smaller value above zero -- a buffer reused in place under the tail of a larger
    batch -- and grows at least once past every earlier maximum after the first step -- a buffer freed and allocated again."""
    table = [ps.counted(s) for s in ps.SCRIPT]
    for q in table[0]:
        v = [t[q] for t in table]
        shrinks = [k for k in range(1, len(v)) if 0 < v[k] < v[k - 1]]
        grows = [k for k in range(1, len(v)) if v[k] > max(v[:k]) and max(v[:k]) > 0]
        print("%-13s %s: shrinks at %s, grows past every earlier maximum at %s" % (
            q, v, [ps.NAMES[k] for k in shrinks], [ps.NAMES[k] for k in grows]))
        assert shrinks and grows, (q, v)
    # the sizes the issue names
    assert [t["utterances"] for t in table] == [70, 42, 37, 101, 130, 65, 37, 0, 3, 70]
    assert table[5]["lists"] == 6 and table[1]["frames"] > table[2]["frames"]
    assert max(t["utterances"] for t in table) <= 130
    assert sum(len(ps.expected(n)[0]) for n in ps.NAMES) < 4500000


def test_the_batches_are_what_the_script_says():
    """The mixed batch E holds at least one utterance of every class the routing knows -- quiet without the nasal pair, quiet, noisy
    with finite parameters, non-finite -- by speechPlayer_frameFacts' flags and speechPlayer_planDirect's fade ends; its quiet utterances sit
    in runs of 32 or more of one timing (fewer would be re-routed to the noisy kernels); under its 1 MB budget the tracks run out
    part-way.  A is 70 quiet nasal-free utterances of one length; C holds NaN holds, NULL frames and M = 0 real frames; F's lists 2 and 5
    are spoken by nobody and list 4 is empty; H3's rows 0 and 2 have no frames."""
    e = ps.built("E")
    cls = ps.utterance_classes(e)
    counts = ps.class_counts(e)
    print("E:", counts)
    assert all(counts[c] > 0 for c in ps.CLASSES) and sum(counts.values()) == 130
    _, length = ps.timeline(e)
    for c in (0, 1):
        assert counts[ps.CLASSES[c]] >= 32 and len(set(length[cls == c])) == 1
    with_budget = ps.track_entries(ps.SCRIPT[ps.NAMES.index("E")])
    without = ps.track_entries(ps.SCRIPT[ps.NAMES.index("E")]._replace(options=dict(tracks=1)))
    print("E: %d track entries under 1 MB, %d without the budget" % (with_budget, without))
    assert 0 < with_budget < without and with_budget * 16 <= 1 << 20 < without * 16
    a = ps.built("A")
    assert ps.class_counts(a) == dict(no_nasal=70, quiet=0, noisy_finite=0, non_finite=0) and len(set(ps.timeline(a)[1])) == 1 and 70 % 64 == 6
    c = ps.built("C")
    real = c["isnull"] == 0
    assert np.isnan(c["frames"][real]).any() and (~real).any() and (c["min"][real] == 0).any()
    f = ps.built("F")
    assert set(f["list_of"]) == {0, 1, 3, 4} and len(f["list_of"]) == 65 and len(set(f["seeds"])) == 65
    assert f["lists"]["frame_start"][5] == f["lists"]["frame_start"][4]
    h = ps.built("H3")
    assert list(np.diff(h["frame_start"])) == [0, 2, 0] and len(ps.built("H0")["frame_start"]) == 1
    for s in ps.SCRIPT:
        assert set(s.options) <= set(ps.DEFAULTS), s.name
        for w in s.walk or ():
            assert set(w) <= set(ps.DEFAULTS), s.name
