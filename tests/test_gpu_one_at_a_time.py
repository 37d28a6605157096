"""The one-parameter-at-a-time corpus (tests/one_at_a_time.py) through every synthesis path at 22 050 Hz.  Needs a GPU.

Every kernel decides per fade WHICH parameters move and acts on those alone; here exactly one moves (or jumps out of a silence), so
a wrong mask bit, offset or stride shows, and the failure names the parameter, manner, composition, lane and path.
All MODE_EXACT results of the same utterances must be the same bytes (docs/KERNELS.md section 4) -- batch paths, "sort", layouts,
live handles against the batch -- and every result is held to tests/test_gpu_parity.py's bar against the oracle.
"""
import numpy as np
import pytest

from tests import one_at_a_time as oat
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu

# the batch paths of the noisy variant: name -> options (None: the defaults)
NOISY_PATHS = {"untracked stages": dict(tracks=0, direct=0), "flat stages": dict(tracks=1, direct=0), "direct stages": dict(tracks=0, direct=2),
               "defaults": None}
_corpora, _anchors = {}, {}


def corpus_of(name):
    """(corpus, the oracle's pcm, start): built and synthesized once per module run."""
    if name not in _corpora:
        c = oat.live_corpus() if name == "live" else oat.batch_corpus(name)
        exp, exp_start, _ = c.oracle(threads=8)
        exp.setflags(write=False)
        _corpora[name] = (c, exp, exp_start)
    return _corpora[name]


def run_batch(c, mode, layout=None, sort=1, options=None):
    import nvspeechplayer_amd as eng
    b = c.batch
    bp = eng.BatchPlayer(oat.SR, mode=mode, layout=layout)
    for k, v in (options or {}).items():
        bp.setOption(k, v)
    bp.setOption("sort", sort)
    bp.setUtterances(b["frame_start"], b["frames"], b["min"], b["fade"], b["index"], b["isnull"], b["seeds"])
    bp.synthesize()
    pcm, start = bp.readAll()
    info = bp.kernelInfo()
    bp.close()
    return pcm, start, info


def anchor_of(name):
    """The MODE_EXACT bytes every other MODE_EXACT result of a corpus is compared with: the stages with the frame state machine, no
    tracks, no direct stages (the quiet variants: the lane kernel), lanes sorted."""
    if name not in _anchors:
        c = corpus_of(name)[0]
        pcm, _, _ = run_batch(c, 0, layout=None if name in ("noisy", "live") else 0, options=dict(tracks=0, direct=0))
        pcm.setflags(write=False)
        _anchors[name] = pcm
    return _anchors[name]


def check(name, path, mode, got, start):
    """Lengths as the oracle's; MODE_EXACT: the anchor's bytes; the oracle within the bar (<= 1 LSB anywhere, <= 5 one-LSB differences
    per million samples, RMS < 1e-5).  A failure names the first differing utterance and sample."""
    c, exp, exp_start = corpus_of(name)
    where = "%s, MODE_%s" % (path, "FAST" if mode else "EXACT")
    assert np.array_equal(start, exp_start), where
    if mode == 0:
        diff = c.first_difference(got, anchor_of(name), start)
        assert diff is None, "%s against the untracked stages: %s" % (where, diff)
    try:
        flips = compare(got, exp, where)
    except AssertionError as e:
        beyond = int(np.abs(got.astype(np.int32) - exp.astype(np.int32)).max()) > 1
        raise AssertionError("%s -- %s" % (e, c.first_difference(got, exp, start, 1 if beyond else 0)))
    print("%s %s: %d utterances, %d samples, %d one-LSB differences from the oracle" % (name, where, len(c), len(exp), flips))
    return flips


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path", list(NOISY_PATHS))
def test_noisy_batch_paths(path, mode):
    """The noisy corpus (every parameter: move pure and as an intruder, jump as an intruder and pure per kind, edges ragged) on the
    untracked stages, the flat stages, the direct stages and the defaults, lanes sorted and in the given order (sort = 0: a
    wavefront holds what the corpus wrote); kernelInfo() says that the path meant was the path taken.
    (Found with it: the direct source stage left the vibrato's phase standing for the rest of the chunk in which a fade's first row
    brought a vibrato that does not move, no lane having had one before -- every utterance of this corpus, up to 1483 LSB.)"""
    c = corpus_of("noisy")[0]
    n = len(c)
    for sort in (0, 1):
        got, start, info = run_batch(c, mode, sort=sort, options=NOISY_PATHS[path])
        counts = (info["tracked_utterances"], info["direct_utterances"])
        if path == "defaults":
            assert sum(counts) == n, info
        else:
            assert counts == {"untracked stages": (0, 0), "flat stages": (n, 0), "direct stages": (0, n)}[path], info
        assert info["lane_pipelined_utterances"] == 0 and info["nasal_free_utterances"] == 0 and info["noisy_group"], info
        check("noisy", "%s, sort %d" % (path, sort), mode, got, start)


def test_noisy_flat_stages_two_workgroups_per_cu():
    """The noisy corpus repeated in order until it no longer fits one workgroup per CU (kernelInfo(): wavefronts // 4 + 1 against cus): the
    flat launch with two workgroups per CU, the instantiation bench.py times (another kernel, whatever its hand-overs and registers), which
    the corpus as it is -- 168 wavefronts -- never takes.  Lanes in the given order, so every wavefront keeps its composition.
    MODE_EXACT: the anchor's bytes, tile by tile; MODE_FAST: the bar.  Every term is present in the noisy base: no wavefront drops one
    (option "dead_terms")."""
    c0, exp, exp_start = corpus_of("noisy")
    anchor = anchor_of("noisy")
    flat = NOISY_PATHS["flat stages"]
    _, _, info0 = run_batch(c0, 0, sort=0, options=flat)
    cus = info0["cus"]
    assert info0["wavefronts"] // 4 + 1 <= cus and info0["tracked_utterances"] == len(c0), info0
    k = 1
    while len(c0) * k // oat.LANES + 1 <= cus:
        k += 1
    c = c0.tiled(k)
    n = len(exp)
    want_start = np.concatenate([[0], np.cumsum(np.tile(np.diff(exp_start), k))]).astype(np.int64)
    for mode in (0, 1):
        got, start, info = run_batch(c, mode, sort=0, options=flat)
        print("noisy x %d, MODE_%s: %d wavefronts on %d CUs, hand-overs of %d samples, %d VGPRs (untiled: %d wavefronts, %d samples, %d VGPRs in MODE_EXACT)" % (
            k, "FAST" if mode else "EXACT", info["wavefronts"], cus, info["stage_parallel_chunk"], info["vgprs"], info0["wavefronts"],
            info0["stage_parallel_chunk"], info0["vgprs"]))
        assert info["wavefronts"] // 4 + 1 > cus, info
        assert info["tracked_utterances"] == len(c) and info["direct_utterances"] == 0 and info["scratch_bytes"] == 0, info
        assert not any(v for key, v in info.items() if key.startswith("waves_without_")), info
        assert np.array_equal(start, want_start)
        if mode == 0:
            for t in range(k):
                diff = c0.first_difference(got[t * n:(t + 1) * n], anchor, exp_start)
                assert diff is None, "two workgroups per CU, tile %d of %d against the untracked stages: %s" % (t, k, diff)
        want = np.tile(exp, k)
        try:
            flips = compare(got, want, "flat stages, two workgroups per CU, MODE_%s" % ("FAST" if mode else "EXACT"))
        except AssertionError as e:
            beyond = int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max()) > 1
            raise AssertionError("%s -- %s" % (e, c.first_difference(got, want, start, 1 if beyond else 0)))
        print("%d utterances, %d samples, %d one-LSB differences from the oracle" % (len(c), len(want), flips))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("layout", [-1, 2, 1, 0])
@pytest.mark.parametrize("variant", ["quiet", "quiet_nasal_free"])
def test_quiet_batch_layouts(variant, layout, mode):
    """The quiet corpora on the lane-pipelined (2), stage-parallel and nasal-free (1) and lane (0) kernels; at the engine's own choice
    (-1) the ragged wavefront -- 64 timings, none shared by 32 utterances -- goes to the flat stages, the rest to the quiet kernels."""
    c = corpus_of(variant)[0]
    n, nasal_free = len(c), variant == "quiet_nasal_free"
    ragged = sum(1 for w in c.what if w[2] == "ragged")
    assert ragged == oat.LANES
    for sort in (0, 1):
        got, start, info = run_batch(c, mode, layout=layout, sort=sort)
        quiet_kernels = n - ragged if layout == -1 else n
        assert info["tracked_utterances"] == (ragged if layout == -1 else 0) and info["direct_utterances"] == 0, info
        if layout == 2:
            assert info["lane_pipelined_utterances"] == (n if nasal_free else 0) and info["lane_pipelined"] == nasal_free, info
            assert info["nasal_free_utterances"] == 0, info
        elif layout == 1:
            assert info["nasal_free_utterances"] == (n if nasal_free else 0) and info["nasal_free"] == nasal_free, info
            assert info["lane_pipelined_utterances"] == 0, info
        elif layout == 0:
            assert info["lane_pipelined_utterances"] == 0 and info["nasal_free_utterances"] == 0, info
        else:
            assert info["lane_pipelined_utterances"] + info["nasal_free_utterances"] == (quiet_kernels if nasal_free else 0), info
        assert not info["noisy_group"], info
        check(variant, "layout %d, sort %d" % (layout, sort), mode, got, start)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel", ["stage", "lane", "switched"])
@pytest.mark.parametrize("policy", ["alone", "shared"])
def test_live_handles(policy, kernel, mode):
    """One move, one jump and one edges case per entry kind and of the two pitches on live handles, pulled together 137 samples at a
    time: the pulls begin inside fades at every offset of the hand-over, where stage_state_load re-derives the masks from the fade's
    end points.  Every handle in a wavefront of its own and 64 to a wavefront; the stage-parallel STREAM kernel, the lane kernel,
    and the kernel changed once between two pulls.  MODE_EXACT: the bytes of the same utterances as a batch."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import _native
    L = _native.load()
    c, exp, exp_start = corpus_of("live")
    if mode == 0:
        batch, start, _ = run_batch(c, 0)
        check("live", "as a batch, defaults", 0, batch, start)
    pull, players = 137, []
    try:
        assert L.speechPlayer_setGlobalOption(b"live_mode", mode) == 0
        assert L.speechPlayer_setGlobalOption(b"live_alone", 1536 if policy == "alone" else 1) == 0
        assert L.speechPlayer_setGlobalOption(b"live_layout", 0 if kernel == "lane" else 1) == 0
        players = [eng.SpeechPlayer(oat.SR, noiseSeed=int(s)) for s in c.seeds]
        for p, frames in zip(players, c.cases):
            for fr, m, f in frames:
                p.queueFrameSamples(None if fr is None else eng.Frame.from_array(fr), m, f)
        out = np.zeros((len(players), pull), np.int16)
        parts, pulls = [[] for _ in players], 0
        longest = int(np.diff(exp_start).max())
        while pulls * pull <= longest:
            if kernel == "switched" and pulls == 5:      # (samples 685 ..: inside the move cases' fade into B')
                assert L.speechPlayer_setGlobalOption(b"live_layout", 0) == 0
            produced = eng.SpeechPlayer.synthesizeMany(players, pull, out=out)
            for k, got in enumerate(produced):
                parts[k].append(out[k, :max(int(got), 0)].copy())
            pulls += 1
        got = np.concatenate([x for p in parts for x in p])
        start = np.concatenate([[0], np.cumsum([sum(len(x) for x in p) for p in parts])]).astype(np.int64)
    finally:
        for p in players:
            p.close()
        L.speechPlayer_setGlobalOption(b"live_mode", 0)
        L.speechPlayer_setGlobalOption(b"live_layout", 1)
        L.speechPlayer_setGlobalOption(b"live_alone", 1536)
    check("live", "live handles %s, %s kernel, pulls of %d" % (policy, kernel, pull), mode, got, start)
