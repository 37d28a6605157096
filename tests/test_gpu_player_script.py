"""One long-lived BatchPlayer through the script of tests/player_script.py (needs a GPU): the life a serving process gives a player --
whatever batch arrives next, of another class, through another entry point, larger or smaller than the one before -- against fresh
players that see one batch each.  What a fresh player's reads and exports ARE is held to the oracle and to their statements by the
other modules; this one adds that HISTORY changes no bit: every read and every export of the reused player equals the fresh player's,
before a launch nothing of the batch before comes back, a refused set call leaves every output of the resident batch as it was, and
options changed between a set call and a launch change which kernels run and never the PCM of MODE_EXACT.
tests/test_player_script_host.py holds the script to the conditions under which this can fail."""
import collections
import functools

import numpy as np
import pytest

from tests import player_script as ps
from tests.test_gpu_parity import compare

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = 1
# the two resamplers the steps alternate between: a step asks for the OTHER one first (the table the step before left on the batch is
# reused across the set call), then for its own (the table is replaced) and for its own again (reused)
RESAMPLERS = (dict(rate=16000, window="hann"), dict(rate=24000, window="kaiser"))
OWN_RESAMPLER = dict(zip(ps.NAMES, (0, 1, 0, 1, 0, 1, 0, 1, 1, 0)))        # (H0 has nothing to resample: G, H3, A' alternate)


def same_bits(a, b):
    """Two outputs hold the same bytes: device tensors, arrays, or tuples / lists / dicts of them."""
    import torch
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        if not isinstance(b, torch.Tensor) or a.shape != b.shape or a.dtype != b.dtype:
            return False
        if a.is_floating_point():
            it = {8: torch.int64, 4: torch.int32, 2: torch.int16}[a.element_size()]
            a, b = a.contiguous().view(it), b.contiguous().view(it)
        return bool(torch.equal(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def refused(call):
    """The call raises and leaves SPEECHPLAYER_ERR_ARGUMENT."""
    from nvspeechplayer_amd import _native
    with pytest.raises(RuntimeError):
        call()
    assert _native.last_error_code() == ERR_ARGUMENT, _native.last_error()


def before_the_launch(bp, name, pinned):
    """After a set call and before a launch: the exports of the PCM and readAllAsync refuse, read and readAll give no sample."""
    n = bp.nUtterances
    if bp.totalSamples > 0:
        refused(lambda: bp.pcmTensor())
        refused(lambda: bp.spectrogramTensor(nFft=256, hop=64))
        refused(lambda: bp.resampledTensor(**RESAMPLERS[OWN_RESAMPLER[name]]))
        refused(lambda: bp.readAllAsync(pinned))
    else:
        assert bp.pcmTensor()[0].numel() == 0 and bp.resampledTensor(16000)[0].numel() == 0 and len(bp.readAllAsync(pinned)[0]) == 0
        bp.readWait()
    for u in range(n):
        assert len(bp.read(u)) == 0, (name, u)
    pcm, starts = bp.readAll()
    assert len(pcm) == 0 and not starts.any() and len(starts) == n + 1, name


def device_exports(bp, name):
    """Every export the batch offers into device tensors on torch's current stream, without a host wait of its own:
    an ordered dict of (tensor, counts or offsets)."""
    import torch
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import speechPlayer as sp
    out = collections.OrderedDict()
    out["pcm int16 padded"] = bp.pcmTensor(dtype=torch.int16)
    out["pcm float32 padded"] = bp.pcmTensor()
    out["pcm int16 packed"] = bp.pcmTensor(dtype=torch.int16, padded=False)
    out["pcm float32 packed"] = bp.pcmTensor(padded=False)
    out["tracks, 49 columns, hop 1"] = bp.trackTensor(list(range(49)), padded=False)
    out["tracks, 49 columns, hop 7 phase 3"] = bp.trackTensor(list(range(49)), hop=7, phase=3, dtype=torch.float64)
    out["source, 6 columns"] = bp.sourceTensor(list(range(6)), dtype=torch.float64, padded=False)
    out["response, 8 kinds, 5 bins, hop 64"] = bp.responseTensor(5, kinds=sp.RESPONSE_KINDS, hop=64, dtype=torch.float64)
    out["stems, 7 columns"] = bp.stemTensor(list(range(7)), dtype=torch.float64, padded=False)
    out["spectrogram, nFft 256, hop 64, 20 mel bands"] = bp.spectrogramTensor(nFft=256, hop=64, bank=eng.melFilterbank(ps.SR, 256, 20), log="db")
    own = OWN_RESAMPLER[name]
    out["resampled, the step before's table"] = bp.resampledTensor(padded=False, **RESAMPLERS[1 - own])
    out["resampled, another table"] = bp.resampledTensor(**RESAMPLERS[own])
    out["resampled, the same table again"] = bp.resampledTensor(dtype=torch.int16, padded=False, **RESAMPLERS[own])
    if bp.hasLabels:
        out["alignment, 8 columns"] = bp.alignmentTensor(list(range(8)), padded=False)
        out["units, hop 64"] = bp.unitTensor(hop=64)
    else:
        refused(lambda: bp.alignmentTensor(list(range(8))))
        refused(lambda: bp.unitTensor(hop=64))
        out["alignment and units refused"] = True
    return out


def host_reads(bp, pinned):
    """Every read that comes back to the host, and the exports whose counts wait for the device."""
    n = bp.nUtterances
    out = collections.OrderedDict()
    out["read"] = [bp.read(u) for u in range(n)]
    out["readFloat"] = [bp.readFloat(u) for u in range(n)]
    pcm, starts = bp.readAll()
    out["readAll"] = (pcm.copy(), starts)
    view, starts = bp.readAllAsync(pinned)
    bp.readWait()
    out["readAllAsync + readWait"] = (np.array(view), starts)
    whole, per = bp.digest(per_utterance=True)
    out["digest"] = (whole, per.copy())
    out["getLastIndex"] = [bp.getLastIndex(u) for u in range(n)]
    out["timeline"] = [bp.timeline(u) for u in range(n)]
    out["marks"] = [bp.marks(u) for u in range(n)]
    out["frames"] = [bp.frames(u) for u in range(n)]
    out["epochCounts"] = bp.epochCounts()
    out["epochTensor"] = bp.epochTensor()
    out["lengths"] = np.array([bp.utteranceSamples(u) for u in range(n)], np.int64)
    out["totals"] = (int(bp.totalSamples), int(bp.totalFrames), bool(bp.hasLabels))
    return out


def all_outputs(bp, name, pinned):
    out = host_reads(bp, pinned)
    out.update(device_exports(bp, name))
    return out


def differing(got, want):
    return [k for k in want if k not in got or not same_bits(got[k], want[k])]


def pinned_buffer():
    import nvspeechplayer_amd as eng
    return eng.host_array((max(len(ps.expected(n)[0]) for n in ps.NAMES) + 64,), np.int16)


def against_the_oracle(out, name):
    """readAll's PCM against the oracle utterance by utterance at the usual bar; lengths and index marks exactly.
    -> (samples compared, one-LSB differences)."""
    exp, exp_start, marks = ps.expected(name)
    pcm, starts = out["readAll"]
    assert np.array_equal(starts, exp_start), name
    assert out["getLastIndex"] == marks.tolist(), name
    flips = 0
    for u in range(len(starts) - 1):
        flips += compare(pcm[starts[u]:starts[u + 1]], exp[exp_start[u]:exp_start[u + 1]], "step %s utterance %d" % (name, u))
    return len(exp), flips


@functools.lru_cache(maxsize=None)
def fresh(name):
    """A step on a player of its own, once per process: -> (kernelInfo() after the set call, every output after the launch)."""
    import torch
    import nvspeechplayer_amd as eng
    step = ps.SCRIPT[ps.NAMES.index(name)]
    bp = eng.BatchPlayer(ps.SR)
    pinned = pinned_buffer()
    ps.apply(bp, step, stream=torch.cuda.Stream(bp.device))
    info = bp.kernelInfo()
    before_the_launch(bp, name, pinned)
    bp.synthesize()
    out = all_outputs(bp, name, pinned)
    torch.cuda.synchronize()
    bp.close()
    return info, out


def refused_set_calls(bp):
    """Three set calls the validation refuses: each leaves -1 and SPEECHPLAYER_ERR_ARGUMENT, and the batch before in place."""
    c, f, b = ps.built("C"), ps.built("F"), ps.built("B")["records"]
    start = c["frame_start"].copy(); start[0] = 1
    yield "frameStart[0] != 0", lambda: bp.setUtterances(start, c["frames"], c["min"], c["fade"], c["index"], c["isnull"], c["seeds"])
    l = f["lists"]
    beyond = f["list_of"].copy(); beyond[11] = 6
    yield "listOf past the lists", lambda: bp.setUtterancesShared(l["frame_start"], l["frames"], l["min"], l["fade"], beyond, l["index"], l["isnull"], f["seeds"])
    labels = b["labels"].copy()
    labels["unit"][3] += 2
    yield "a unit that jumps by two", lambda: bp.setRecords(b["shapes"], b["list_start"], b["records"], listOf=b["list_of"], labels=labels)


def test_one_player_through_the_script():
    """ONE BatchPlayer through A .. A', each step also on a fresh player.  After every set call and before the launch nothing of the step
    before comes back; after the launch the PCM is the oracle's at the usual bar, lengths and index marks exactly, and every read and
    every export holds the fresh player's bytes; between B and C and between E and F three refused set calls leave every output as it
    was (against copies taken before them); A' gives what A gave."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(ps.SR)
    pinned = pinned_buffer()
    side = torch.cuda.Stream(bp.device)
    first = None
    total = 0
    for step in ps.SCRIPT:
        name = step.name
        info_fresh, want = fresh(name)
        ps.apply(bp, step, stream=side)
        info = bp.kernelInfo()
        classes = ps.class_counts(ps.built(name))
        assert step.routed(info, bp.hasLabels, classes), (name, info, classes)
        assert info == info_fresh, (name, info, info_fresh)
        assert name != "G" or info == fresh("C")[0], (info, fresh("C")[0])      # (the same frames: the same plan)
        before_the_launch(bp, name, pinned)
        bp.synthesize()
        got = all_outputs(bp, name, pinned)
        torch.cuda.synchronize()
        samples, flips = against_the_oracle(got, name)
        assert list(got) == list(want), name
        assert differing(got, want) == [], name
        compared = len(want)
        if name in ("B", "E"):
            for what, call in refused_set_calls(bp):
                refused(call)
                again = all_outputs(bp, name, pinned)
                torch.cuda.synchronize()
                assert differing(again, got) == [], (name, what)
                assert bp.kernelInfo() == info, (name, what)
                compared += len(got)
        if first is None:
            first = got
        total += compared
        print("step %-2s %7d samples against the oracle, %d one-LSB differences; %d outputs equal the fresh player's bytes" % (name, samples, flips, compared))
    assert differing(got, first) == [] and list(got) == list(first), "A' against A"
    print("%d outputs compared in all" % total)
    bp.close()


def launch_and_check(bp, name, first_exact):
    """One more launch of the resident batch: lengths and index marks exactly; MODE_EXACT gives first_exact's bytes (None: it is taken)."""
    exp, exp_start, marks = ps.expected(name)
    bp.synthesize()
    pcm, starts = bp.readAll()
    assert np.array_equal(starts, exp_start)
    assert [bp.getLastIndex(u) for u in range(len(marks))] == marks.tolist()
    flips = 0
    for u in range(len(starts) - 1):
        flips += compare(pcm[starts[u]:starts[u + 1]], exp[exp_start[u]:exp_start[u + 1]], "step %s utterance %d" % (name, u))
    return pcm.copy(), flips


def exports_as_set(bp):
    import torch
    from nvspeechplayer_amd import speechPlayer as sp
    out = collections.OrderedDict()
    out["tracks"] = bp.trackTensor(list(range(49)), dtype=torch.float64, padded=False)
    out["source"] = bp.sourceTensor(list(range(6)), dtype=torch.float64, padded=False)
    out["response"] = bp.responseTensor(5, kinds=sp.RESPONSE_KINDS, hop=64, dtype=torch.float64)
    out["stems"] = bp.stemTensor(list(range(7)), dtype=torch.float64, padded=False)
    torch.cuda.synchronize()
    return out


def walk(bp, step):
    """The step's batch set once under its own options, then launched again and again with the options of its walk changed in
    between and no further set call."""
    ps.apply(bp, step)
    before = exports_as_set(bp)
    state = dict(ps.DEFAULTS, **step.options)
    exact = None
    for change in step.walk:
        for k, v in change.items():
            bp.setOption(k, v)
        state.update(change)
        info = bp.kernelInfo()
        if state["tracks"] == 0 or state["layout"] == 0:
            assert info["tracked_utterances"] == 0, (step.name, change, info)
        elif step.name == "E":
            assert info["tracked_utterances"] > 0, (step.name, change, info)
        if state["layout"] == 2:
            assert info["lane_pipelined_utterances"] > 0, (step.name, change, info)
        if state["layout"] in (0, 1):
            assert info["lane_pipelined_utterances"] == 0, (step.name, change, info)
        pcm, flips = launch_and_check(bp, step.name, exact)
        if state["mode"] == 0:
            if exact is None:
                exact = pcm
            assert pcm.tobytes() == exact.tobytes(), (step.name, change)
        print("%s launched under %-32s %d one-LSB differences from the oracle; tracked %d direct %d lane-pipelined %d nasal-free %d" % (
            step.name, change or "its own options", flips, info["tracked_utterances"], info["direct_utterances"], info["lane_pipelined_utterances"],
            info["nasal_free_utterances"]))
    assert exact is not None
    assert differing(exports_as_set(bp), before) == [], step.name


def test_options_between_set_and_launch():
    """Batch E, set once, launched thirteen times with one option changed before each launch (tracks, layout, mode, direct_lean,
    quiet_last): lengths and index marks are the oracle's after every launch, every MODE_EXACT launch gives the first one's bytes, every
    launch passes the usual bar, kernelInfo() shows what ran, and the exports of the batch as set hold the same bits before and after.
    The same for A, whose tail of six has replicas, through every layout and both modes.  Then directAligned: a time-aligned noisy
    batch, a set call that forms no direct group, and D on the direct stages -- residency and PCM are those of a fresh player given
    only the last set call."""
    import nvspeechplayer_amd as eng
    from nvspeechplayer_amd import workloads
    from tests.test_gpu_timeline import set_host
    bp = eng.BatchPlayer(ps.SR)
    walk(bp, ps.SCRIPT[ps.NAMES.index("E")])
    other = eng.BatchPlayer(ps.SR)
    walk(other, ps.SCRIPT[ps.NAMES.index("A")])
    other.close()
    d = ps.built("D")
    ps.set_options(bp, dict(tracks=0))
    # (128 utterances are runs of 16 equally timed ones, below the 32 the routing calls aligned: the direct stages take them; 256 are
    # runs of 32, which MODE_EXACT keeps on the stages with the frame state machine -- the verdict "aligned" is what must not outlive them)
    for n_utt, on_direct in ((128, True), (256, False)):
        set_host(bp, workloads.make("cfg2", n_utt))
        info = bp.kernelInfo()
        assert (info["direct_utterances"] > 0) == on_direct and info["tracked_utterances"] == 0, (n_utt, info)
        bp.synthesize()
    bp.setOption("direct", 0)
    set_host(bp, d)
    assert bp.kernelInfo()["direct_utterances"] == 0
    bp.setOption("direct", 2)
    set_host(bp, d)
    alone = eng.BatchPlayer(ps.SR)
    ps.set_options(alone, dict(tracks=0, direct=2))
    set_host(alone, d)
    for mode in (0, 1):
        result = []
        for p in (bp, alone):
            p.setOption("mode", mode)
            p.setOption("direct_lean", -1)
            info = p.kernelInfo()
            assert info["direct"] and info["direct_utterances"] > 0, info
            p.synthesize()
            result.append((info, p.readAll()[0].copy(), p.digest()))
        assert result[0][0] == result[1][0], (mode, result[0][0], result[1][0])
        assert result[0][1].tobytes() == result[1][1].tobytes() and result[0][2] == result[1][2], mode
        print("D after an aligned batch, mode %d: hand-over chunk %d, %d utterances on the direct stages, as on a fresh player" % (
            mode, result[0][0]["stage_parallel_chunk"], result[0][0]["direct_utterances"]))
    alone.close()
    bp.close()


def test_the_script_without_host_waits():
    """The script on one player with synthesize(wait=False): the exports go on a side stream right behind each launch, the next set
    call follows at once, and the device tensors are looked at only at the end -- they hold what the fresh players gave."""
    import torch
    import nvspeechplayer_amd as eng
    bp = eng.BatchPlayer(ps.SR)
    side = torch.cuda.Stream(bp.device)
    kept = []
    for step in ps.SCRIPT:
        ps.apply(bp, step, stream=side)
        bp.synthesize(wait=False)
        with torch.cuda.stream(side):
            kept.append(device_exports(bp, step.name))
    torch.cuda.synchronize()
    total = 0
    for step, got in zip(ps.SCRIPT, kept):
        want = fresh(step.name)[1]
        assert differing(got, {k: want[k] for k in got}) == [] and set(got) <= set(want), step.name
        total += len(got)
        print("step %-2s %d exports queued behind the launch equal the fresh player's bytes" % (step.name, len(got)))
    print("%d exports compared in all" % total)
    bp.close()
