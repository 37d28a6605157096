"""What tests/test_gpu_stage_far.py rests on, without a GPU (tests/far_offsets.py: DeepStream, DEEP, deep_*): the planning arithmetic of a
deep stream against brute force on small numbers and in closed form at 2^31 and 2^32; and, against the host statements signalResample,
signalConvolve and signalSpectrogram for each of the deep cases, the two facts that let a device push deep in a stream be held to a
statement the host can only run on a short one -- a periodic input gives a periodic output bit for bit, and the steady period W cut from
four periods is the period of a longer stream --, that a stream's last outputs do not depend on how many whole periods came before, and
that W changes in most of its elements when the period table is rotated by 2^31 mod P or 2^32 mod P: an index that lost its high bits
reads another sample of the period, so the device test can fail."""
import numpy as np
import pytest

from tests.far_offsets import (B31, B32, DEEP, FAR_WIDTH, SHORT, DeepStream, deep_bands, deep_emitted, deep_period, deep_plan, deep_short,
                               deep_statement, deep_table, deep_W, far_padded_signal, rotated)

FORMATS = (1, 0)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def resampler(Z, up, down):
    return lambda N: -(-max(N - Z, 0) * up // down)


def frames(nFft, hop, phase):
    return lambda N: 0 if N - (nFft // 2 - 1) - 1 - phase < 0 else (N - (nFft // 2 - 1) - 1 - phase) // hop + 1


@pytest.mark.parametrize("model", [("resample", 9, 320, 441, 3), ("resample", 7, 320, 147, 7), ("resample", 73, 1, 12, 5), ("convolution", 0, 1, 1, 37),
                                   ("spectrogram", 64, 16, 0, 7), ("spectrogram", 64, 80, 5, 3)])
def test_the_plan_against_brute_force_at_small_bounds(model):
    """Push after push by the closed forms of csrc/klatt_stage.h and klatt_stage_window.h, with the chunk near 2^11 and the bounds 2^15
    and 2^16: the counts before every push, the push that holds each bound, the pushes needed to pass it, the rotation."""
    kind, a, b, c_, odd = model
    if kind == "resample":
        emitted, P, Q = resampler(a, b, c_), c_ * odd, b * odd
    elif kind == "convolution":
        emitted, P, Q = (lambda N: N), odd, odd
    else:
        emitted, P, Q = frames(a, b, c_), b * odd, odd
    near = 1 << 11
    c = near // P * P
    plan = DeepStream(P, Q, c // P * Q - emitted(c), near)
    assert plan.c == c and plan.c % P == 0 and near - P < plan.c <= near and plan.G * P == plan.c * Q
    N, M, seen = 0, 0, []
    for k in range(500):
        assert (plan.consumed(k), plan.emitted(k)) == (N, M), (model, k)
        assert plan.rotation(k) == M % Q and (k < 2 or plan.rotation(k) == plan.rotation(1))
        seen.append((N, M))
        N += c
        M = emitted(N)
    for at, of in enumerate("NM"):
        for bound in ((1 << 15, 1 << 16) if of == "N" else ((1 << 15) * Q // P + 1, (1 << 16) * Q // P + 1)):      # (outputs scale with the ratio)
            holds = [k for k in range(len(seen) - 1) if seen[k][at] <= bound < seen[k + 1][at]]
            assert holds == [plan.crossing(bound, of)], (model, bound, of)
            assert plan.pushes_to_pass(bound, of) == min(k for k in range(len(seen)) if seen[k][at] > bound), (model, bound, of)
            assert plan.count(plan.crossing(bound, of), of) <= bound < plan.count(plan.crossing(bound, of) + 1, of)


@pytest.mark.parametrize("name", sorted(DEEP))
def test_the_periods_divide_no_power_of_two_and_the_bounds_fall_inside_a_push(name):
    case = DEEP[name]
    P, Q, mult = deep_period(case)
    odd = case.get("k", case.get("q", case.get("P")))
    assert odd % 2 == 1 and odd > 1 and P % odd == 0 and Q % odd == 0
    assert B31 % P and B32 % P and B31 % Q and B32 % Q
    plan = deep_plan(name)
    assert plan.c % P == 0 and (1 << 27) - P < plan.c <= 1 << 27 and plan.G == plan.c // P * Q
    pushes = plan.pushes_to_pass(case["bound"], "N")
    assert plan.consumed(pushes) > case["bound"] >= plan.consumed(pushes - 1) and pushes == case["bound"] // plan.c + 1
    for bound in (B31, B32):      # no bound at a push boundary, in N, in M or in the kernel's product M * mult
        for of, b in (("N", bound), ("M", bound), ("M", -(-bound // mult))):
            k = plan.crossing(b, of)
            if k < pushes:
                assert plan.count(k, of) < b < plan.count(k + 1, of), (name, bound, of)
    # what the table of the cases promises
    final_N, final_M = plan.consumed(pushes), plan.emitted(pushes)
    if name == "resample 22050 -> 48000":
        assert final_N > B31 and final_M > B32 and final_M * mult > B32
    elif case["kind"] == "spectrogram":
        assert final_M * mult > B32 and final_N > B32
    else:
        assert final_N > B32
    if case["rows"] == 2:
        assert plan.pushes_to_pass(1 << 30, "N") + 2 < pushes      # row 1 is reset well before the end


@pytest.mark.parametrize("name", sorted(DEEP))
def test_periodic_in_periodic_out_and_w_is_the_statements_period(name):
    """On seven periods: outputs 2 Q .. 6 Q - 1 are W again and again, in both formats, bit for bit (the last period is the resampler's and
    the spectrogram's run-out onto +0); on the short stream of four, the outputs before 2 Q are the longer stream's (a fresh row's first
    push is held to them), and they differ from W somewhere, so the first push is a case of its own."""
    case = DEEP[name]
    P, Q, _ = deep_period(case)
    for row in range(case["rows"]):
        for fmt in FORMATS:
            W = deep_W(name, row, fmt)
            assert W.shape == ((Q,) if deep_bands(case) == 1 else (Q, deep_bands(case)))
            long = deep_statement(name, row, np.tile(deep_table(name, row), 7), fmt)
            assert len(long) >= 7 * Q
            for j in range(2, 6):
                assert same(long[j * Q:(j + 1) * Q], W), (name, row, fmt, j)
            short = deep_short(name, row, fmt)
            assert same(short[:3 * Q], long[:3 * Q]), (name, row, fmt)
            assert same(rotated(W, 2 * Q + 3, 2 * Q + 1), long[2 * Q + 3:][:2 * Q + 1]), (name, row, fmt, "rotated")
            assert not same(short[:Q], W)


@pytest.mark.parametrize("name", sorted(DEEP))
def test_rotating_the_table_by_a_lost_high_bit_changes_most_of_w(name):
    """An index short of 2^31 or 2^32 reads the period 2^31 mod P or 2^32 mod P samples from its place: W of the table so rotated differs
    from W in most elements."""
    case = DEEP[name]
    P, Q, _ = deep_period(case)
    for row in range(case["rows"]):
        W = deep_W(name, row, 1)
        assert len(np.unique(W.reshape(-1))) > W.size // 2      # random: (nearly) all values of the period differ
        for r in (B31 % P, B32 % P, (-B31) % P, (-B32) % P):
            assert 0 < r < P
            other = deep_W(name, row, 1, rotate=r)
            assert other.shape == W.shape and np.mean(other.reshape(-1) != W.reshape(-1)) > 0.5, (name, row, r)
        for r in (B31 % Q, B32 % Q):      # ... and the same for an OUTPUT index that lost its high bits
            assert 0 < r < Q and np.mean(rotated(W, r).reshape(-1) != W.reshape(-1)) > 0.5, (name, row, r)


@pytest.mark.parametrize("name", sorted(DEEP))
def test_a_streams_last_outputs_do_not_depend_on_the_periods_before(name):
    """The last push of a deep stream -- P + 37 samples, 37 for the convolution, then the end -- against the statement on four periods and
    that chunk: the same count and the same values as behind seven periods."""
    case = DEEP[name]
    P, Q, _ = deep_period(case)
    for row in range(case["rows"]):
        last = deep_table(name, row, length=37 if case["kind"] == "convolution" else P + 37, seed=1)
        counts = {k: deep_emitted(name, row, k * P + len(last), ended=True) - deep_emitted(name, row, k * P) for k in (SHORT, 7, 1 << 20)}
        assert len(set(counts.values())) == 1 and counts[SHORT] > 0, (name, row, counts)
        for fmt in FORMATS:
            short = deep_short(name, row, fmt, last=last)
            long = deep_statement(name, row, np.concatenate([np.tile(deep_table(name, row), 7), last]), fmt)
            assert len(short) == deep_emitted(name, row, SHORT * P + len(last), ended=True)
            assert same(short[len(short) - counts[SHORT]:], long[len(long) - counts[SHORT]:]), (name, row, fmt)


def test_the_far_width_puts_both_bounds_just_inside_a_row():
    assert FAR_WIDTH % 2 == 1 and B31 == 21846 * FAR_WIDTH + 2 and B32 == 43692 * FAR_WIDTH + 4
    n, lens, real, straddlers = far_padded_signal([[65, 63, 131, 1], [131, 65, 63, 7]], (B31, B32), FAR_WIDTH)
    assert straddlers == {B31: 21846, B32: 43692} and real == [21846, 21845, 21847, 21848, 43692, 43691, 43693, 43694] and n == 43695
    for b, r in straddlers.items():
        assert r * FAR_WIDTH < b < r * FAR_WIDTH + 7 - 1      # the shortest chunk of a straddling row still holds the bound inside it
    assert n * FAR_WIDTH > B32
