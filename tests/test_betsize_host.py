"""CPU-only checks of bet sizing: the definition in tests/_bet_ref.py in its two forms against each other and
against the book's float mean, the discretisation against Python's round, the host closed forms, the host program of
csrc/fmk_bet_rule.h (tools/bet_check.cpp) bit for bit against the definition, and the refusals of the Python layer that need no
device."""
import functools
import math
import os
import struct
import subprocess
from statistics import NormalDist

import numpy as np
import pytest

from tests import _bet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def campaign(seed, cases, max_n, max_events):
    rng = np.random.default_rng(seed)
    for _ in range(cases):
        n = int(rng.integers(1, max_n + 1))
        ne = int(rng.integers(1, max_events + 1))
        yield (n,) + R.random_case(rng, n, ne, max_len=int(rng.integers(1, n + 1)))


# ---------------------------------------------------------------------------------------------- the two forms
# (the next three tests are self-checks of the reference in tests/_bet_ref.py: they run nothing of the library)
def test_direct_and_cumulative_forms_agree():
    steps = [0.0] + R.STEPS
    for k, (n, ev, tc, sig) in enumerate(campaign(10, 150, 60, 40)):
        step = steps[k % len(steps)]
        v1, c1 = R.path_direct(ev, tc, sig, n, step)
        v2, c2 = R.path_cumulative(ev, tc, sig, n, step)
        assert c1 == c2.tolist(), k
        assert np.array_equal(v1, v2), (k, step)                          # Python's round gives +0.0 where rint gives -0.0
        if step == 0.0:
            assert same_bits(v1, v2), k
            assert not np.any(np.signbit(v2) & (v2 == 0.0)), "-0.0 in an average"
        side = np.random.default_rng(k).integers(-1, 2, len(ev))
        m1, l1, s1 = R.budget_direct(ev, tc, side, n)
        m2, l2, s2 = R.budget_cumulative(ev, tc, side, n)
        assert (l1, s1) == (l2, s2) and same_bits(m1, m2), k


def test_units():
    assert [R.quantise(m) for m in (1.0, -1.0, 0.0, -0.0, 2.0 ** -31, 3 * 2.0 ** -31, 2.0 ** -30, 1 - 2.0 ** -30)] == \
        [1 << 30, -(1 << 30), 0, 0, 0, 2, 1, (1 << 30) - 1]
    v, c = R.path_cumulative([0, 0], [2, 2], [2.0 ** -31, 3 * 2.0 ** -31], 3)           # 0 and 2 units: the mean is one unit
    assert v.tolist() == [2.0 ** -30, 2.0 ** -30, 0.0] and c.tolist() == [2, 2, 0]


def test_definition_against_the_books_float_mean():
    """|value - snippet 10.2's mean| <= 2^-30 at the union points: each q_i 2^-30 is within 2^-31 of m_i and so is a mean of them;
    summing at most 32767 doubles of [-1, 1] adds less than 2^-37, the two roundings of the quotient less than 2^-52."""
    for k, (n, ev, tc, sig) in enumerate(campaign(11, 100, 200, 120)):
        v, _ = R.path_cumulative(ev, tc, sig, n)
        points, means = R.book_avg_active_signals(ev, tc, sig)
        worst = float(np.max(np.abs(v[points] - means)))
        assert worst <= 2.0 ** -30, (k, worst)


# ---------------------------------------------------------------------------------------------- discretisation
def discretise_cases(step):
    vs = [0.0, -0.0, 1.0, -1.0, 0.999999, -0.999999, 2.0 ** -30, -(2.0 ** -30), 0.5, -0.5, 0.25, -0.25]
    for k in range(-12, 12):
        t = (k + 0.5) * step                                              # candidates for v / step == k + 0.5 exactly
        for v in (t, np.nextafter(t, 2.0), np.nextafter(t, -2.0)):
            if -1.0 <= v <= 1.0:
                vs.append(float(v))
    vs += [1.0 - step / 4, -(1.0 - step / 4), 1.0 - step / 2, -(1.0 - step / 2)]       # the last step before the clip
    vs += np.random.default_rng(5).uniform(-1, 1, 300).tolist()
    return vs + [1.3, -1.3, 5.0, -5.0, 1.0 + step, -1.0 - step]       # beyond the clip


@pytest.mark.parametrize("step", R.STEPS)
def test_discretise_equals_pythons_round(step):
    from finmlkit_amd.label import discretise
    vs = discretise_cases(step)
    ties = [v for v in vs if (v / step) - math.floor(v / step) == 0.5]
    assert ties, "no exact tie among the cases"
    want = [R.discretise(v, step) for v in vs]
    assert np.array_equal(discretise(vs, step), want)                     # as numbers: Python's round loses the sign of a zero
    assert np.array_equal(R.book_discrete_signal(vs, step), want)
    assert same_bits(discretise(vs, step), R.discretise_np(vs, step))
    assert any(round(v / step) * step > 1.0 for v in vs) and any(round(v / step) * step < -1.0 for v in vs), "the clip is not reached"
    assert same_bits(discretise(vs, 0.0), vs)
    got = discretise([1.0, -1.0], step)
    assert got.tolist() == [R.discretise(1.0, step), R.discretise(-1.0, step)] and np.all(np.abs(got) <= 1.0)


def test_discretise_clips():
    from finmlkit_amd.label import discretise
    # 1 / (1/3) rounds to 3 and 3 * (1/3) to 1.0; a step whose multiple passes 1 is clipped
    assert discretise([0.96, -0.96], 0.7).tolist() == [0.7, -0.7]
    assert discretise([1.0, -1.0], 0.6).tolist() == [1.0, -1.0]           # rint(1.67) * 0.6 = 1.2 -> clipped
    assert R.discretise(1.0, 0.6) == 1.0 and round(1.0 / 0.6) * 0.6 > 1.0
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="step"):
            discretise([0.0], bad)


# ---------------------------------------------------------------------------------------------- signal_from_probability
def test_signal_from_probability():
    from finmlkit_amd.label import signal_from_probability as f
    for K in (2, 3, 5, 10):
        got = f([0.0, 1.0, 1.0 / K], n_classes=K)
        assert got.tolist() == [-1.0, 1.0, 0.0], K
        assert f([0.0, 1.0, 1.0 / K], [-1, -1, -1], n_classes=K).tolist() == [1.0, -1.0, -0.0]
    rng = np.random.default_rng(3)
    p = rng.uniform(0, 1, 500)
    pred = rng.choice([-1, 1], 500)
    side = rng.choice([-1, 0, 1], 500)
    base = f(p)
    assert same_bits(f(p, pred), base * pred) and same_bits(f(p, -pred), -(base * pred))
    assert same_bits(f(p, pred, side), base * pred * side) and same_bits(f(p, side=side), base * side)
    nd = NormalDist()
    for K in (2, 3):
        got = f(p, n_classes=K)
        z = (p - 1.0 / K) / np.sqrt(p * (1.0 - p))
        want = np.array([2.0 * nd.cdf(v) - 1.0 for v in z])
        assert float(np.max(np.abs(got - want))) <= 2.0 ** -50
        assert float(np.max(np.abs(f(p, pred, n_classes=K) - R.book_get_signal(p, pred, K)))) <= 2.0 ** -50
    assert np.all(np.abs(f(p, pred, side)) <= 1.0)
    for args, kw in ((([-0.1],), {}), (([1.1],), {}), (([float("nan")],), {}), (([0.5],), {"n_classes": 1}),
                     (([0.5],), {"n_classes": 2.5}), (([0.5, 0.6], [1]), {}), (([0.5, 0.6],), {"side": [1, 1, 1]}),
                     (([0.5], [2]), {}), (([0.5],), {"side": [float("nan")]})):
        with pytest.raises(ValueError):
            f(*args, **kw)


# ---------------------------------------------------------------------------------------------- the sigmoid family
def ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def test_sigmoid_family():
    from finmlkit_amd.label import bet_size_sigmoid, calibrate_w, inv_price, limit_price, target_position
    rng = np.random.default_rng(4)
    for _ in range(300):
        x = float(rng.uniform(0.01, 50.0)) * (1 if rng.random() < 0.5 else -1)
        m = math.copysign(float(rng.uniform(0.01, 0.99)), x)
        w = calibrate_w(x, m)
        # two evaluations of m^-2 may differ by an ulp each way; the subtraction of 1 magnifies that by m^-2 / (m^-2 - 1) = 1 / (1 - m^2)
        assert abs(w - R.book_get_w(x, m)) <= R.book_get_w(x, m) * 2.0 ** -52 * (2.0 + 2.0 / (1.0 - m * m))
        assert ulps(bet_size_sigmoid(w, x), m) <= 4, (x, m)
        f = float(rng.uniform(50, 150))
        w2 = float(rng.uniform(0.1, 100.0))
        price = inv_price(f, w2, m)                                       # the price at which the size is m ...
        assert abs(bet_size_sigmoid(w2, f - price) - m) <= 1e-12          # ... gives m back: a few ulp of f over the divergence
        assert abs(inv_price(f, w2, bet_size_sigmoid(w2, x)) - (f - x)) <= 1e-9 * max(1.0, abs(x))
        assert target_position(w2, f, price, 100) == R.book_get_t_pos(w2, f, price, 100)
    # the book's own numbers: pos 0, forecast 100, w from (10, .95), market price 90, maxPos 100
    w = calibrate_w(10.0, 0.95)
    t_pos = target_position(w, 100.0, 90.0, 100)
    assert t_pos == R.book_get_t_pos(w, 100.0, 90.0, 100) and t_pos in (94, 95)
    for tp, pos in ((t_pos, 0), (-40, 10), (10, -40), (3, 2), (-3, -2), (50, 49)):
        assert limit_price(tp, pos, 100.0, w, 100) == R.book_limit_price(tp, pos, 100.0, w, 100)
    assert math.isnan(limit_price(7, 7, 100.0, w, 100))
    assert target_position(w, np.array([100.0, 100.0]), np.array([90.0, 110.0]), 100).tolist() == [t_pos, -t_pos]
    for call in (lambda: bet_size_sigmoid(0.0, 1.0), lambda: bet_size_sigmoid(-1.0, 1.0), lambda: calibrate_w(1.0, 0.0),
                 lambda: calibrate_w(1.0, 1.0), lambda: calibrate_w(1.0, -1.5), lambda: inv_price(100.0, 0.0, 0.5),
                 lambda: inv_price(100.0, 1.0, 1.0), lambda: inv_price(100.0, 1.0, float("nan")),
                 lambda: target_position(1.0, 100.0, 90.0, 0), lambda: target_position(0.0, 100.0, 90.0, 10),
                 lambda: limit_price(5, 0, 100.0, -1.0, 10), lambda: limit_price(5, 0, 100.0, 1.0, 0),
                 lambda: limit_price(10, 0, 100.0, 1.0, 10), lambda: limit_price(1.5, 0, 100.0, 1.0, 10)):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------------------------- the host program
@functools.lru_cache(maxsize=None)
def check_program():
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(prefix="bet_check_"), "bet_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tools", "bet_check.cpp"),
                           "-o", exe])
    return exe


def path_text(ev, tc, sig, n, step):
    rows = "".join(f"{int(a)} {int(b)} {float(m).hex()}\n" for a, b, m in zip(ev, tc, sig))
    return f"path {len(ev)} {n} {float(step).hex()}\n" + rows


def budget_text(ev, tc, side, n):
    return f"budget {len(ev)} {n}\n" + "".join(f"{int(a)} {int(b)} {int(s)}\n" for a, b, s in zip(ev, tc, side))


def test_host_program_equals_the_definition_bit_for_bit():
    steps = [0.0] + R.STEPS
    cases = list(campaign(12, 120, 300, 200))
    big = np.zeros(40000, np.int64)                                       # refused: 40 000 events on one tick
    text, want = [], []
    for k, (n, ev, tc, sig) in enumerate(cases):
        step = steps[k % len(steps)]
        side = np.random.default_rng(k).integers(-1, 2, len(ev))
        text += [path_text(ev, tc, sig, n, step), budget_text(ev, tc, side, n)]
        v, c = R.path_cumulative(ev, tc, sig, n, step)
        m, ml, ms = R.budget_cumulative(ev, tc, side, n)
        want += ["ok"] + [f"{bits(a):016x} {int(b)}" for a, b in zip(v, c)]
        want += [f"ok {ml} {ms}"] + [f"{bits(a):016x}" for a in m]
    text += [path_text(big, big + 2, np.ones(40000), 4, 0.0), path_text([0, 3], [2, 1], [0.5, 0.5], 4, 0.0),
             path_text([0, 1], [2, 2], [float("nan"), 1.5], 4, 0.0), budget_text(big, big + 2, np.ones(40000), 4),
             budget_text(big, big + 2, -np.ones(40000), 4)]
    want += ["refused concurrency 40000", "refused spans 1", "refused signals 2", "refused concurrency 40000", "refused concurrency 40000"]
    vs = discretise_cases(0.1)
    text.append(f"disc {len(vs)} {0.1.hex()}\n" + "".join(f"{v.hex()}\n" for v in vs))
    want += [f"{bits(v):016x}" for v in R.discretise_np(vs, 0.1)]
    r = subprocess.run([check_program()], input="".join(text), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.strip().split("\n")
    assert len(got) == len(want)
    assert got == want, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w)


# ---------------------------------------------------------------------------------------------- the Python layer's refusals
def test_python_layer_refuses_before_any_device_call():
    from finmlkit_amd import label as L
    from finmlkit_amd.label import betsize as B
    ev, tc, sig = np.array([0, 2], np.int64), np.array([3, 5], np.int64), np.array([0.5, -0.5])
    side = np.array([1, -1], np.int8)
    calls = {
        "path": lambda e, t, x, **kw: L.bet_size_path(e, t, x, **kw),
        "at": lambda e, t, x, **kw: L.bet_size_at(e, t, x, **kw),
        "avg": lambda e, t, x, **kw: L.avg_active_signals(e, t, x, **kw),
    }
    for name, f in calls.items():
        with pytest.raises(ValueError, match="same length"):
            f(ev, tc[:1], sig)
        with pytest.raises(ValueError, match="length of event_idxs"):
            f(ev, tc, sig[:1])
        with pytest.raises(ValueError, match="integer arrays"):
            f(ev.astype(np.float64), tc, sig)
        with pytest.raises(ValueError, match="real numbers"):
            f(ev, tc, np.array(["a", "b"]))
        with pytest.raises(ValueError, match="real numbers"):
            f(ev, tc, sig.astype(np.complex128))
        with pytest.raises(ValueError, match="n_events"):
            f(ev[:0], tc[:0], sig[:0], n=4)
        with pytest.raises(ValueError, match="1 events outside"):
            f(ev, tc, sig, n=5)
        with pytest.raises(ValueError, match="1 events outside"):
            f(np.array([0, 4]), np.array([3, 2]), sig)
        with pytest.raises(ValueError, match="1 events outside"):
            f(np.array([-1, 2]), tc, sig)
        with pytest.raises(ValueError, match="1 signals are NaN"):
            f(ev, tc, np.array([0.5, float("nan")]))
        with pytest.raises(ValueError, match="2 signals are NaN"):
            f(ev, tc, np.array([1.0000000000000002, -1.5]))
        for step in (-0.5, 1.0000000000000002, float("nan"), float("inf"), "x"):
            with pytest.raises(ValueError, match="step"):
                f(ev, tc, sig, step=step)
        with pytest.raises(ValueError, match=r"2\^32"):
            f(ev, tc, sig, n=(1 << 32) + 1)
    with pytest.raises(ValueError, match="1 indices outside"):
        L.bet_size_at(ev, tc, sig, np.array([0, 6]))
    with pytest.raises(ValueError, match="1 indices outside"):
        L.bet_size_at(ev, tc, sig, np.array([-1, 5]))
    with pytest.raises(ValueError, match="integer array"):
        L.bet_size_at(ev, tc, sig, np.array([0.5]))
    with pytest.raises(ValueError, match="same length"):
        L.bet_size_budget(ev, tc[:1], side)
    with pytest.raises(ValueError, match="length of event_idxs"):
        L.bet_size_budget(ev, tc, side[:1])
    with pytest.raises(ValueError, match="integer array"):
        L.bet_size_budget(ev, tc, np.array([0.5, 1.0]))
    with pytest.raises(ValueError, match="1 events outside"):
        L.bet_size_budget(ev, tc, side, n=5)
    with pytest.raises(ValueError, match=r"2\^32"):
        L.bet_size_budget(ev, tc, side, n=(1 << 32) + 1)
    import pandas as pd
    frame = pd.DataFrame({"event_idx": ev, "touch_idx": tc})
    with pytest.raises(ValueError, match="one value per row"):
        L.BetSizing.from_probabilities(frame, [0.5])
    with pytest.raises(ValueError, match="must contain"):
        L.BetSizing.from_probabilities(frame[["event_idx"]], [0.5, 0.5])
    with pytest.raises(ValueError, match="outside"):
        L.BetSizing.from_probabilities(frame, [0.5, 1.5])
    g = B.geometry()                                                      # needs the library, not a device
    assert g["tile"] % g["row"] == 0 and g["row"] % 256 == 0 and g["agg_unit"] >= 64
