"""GPU checks of bet sizing (csrc/fmk_bet.hip): values, counts, budget positions and maxima equal to the Python
definition of tests/_bet_ref.py everywhere -- at every seam of the kernels' geometry, at the extremes of the sums, on the unit cases
of the signal, through the host-pointer and the resident entries -- and every refusal the device counts, after which the context
goes on working."""
import functools

import numpy as np
import pandas as pd
import pytest

from tests import _bet_ref as R

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def geo():
    from finmlkit_amd.label.betsize import geometry
    g = geometry()
    return g["tile"], g["row"], g["agg_unit"]


def check_path(ev, tc, sig, n, step=0.0):
    """host-pointer entry against the definition: values (as numbers and as bits) and counts -> (values, counts)"""
    from finmlkit_amd.label import bet_size_path
    ev, tc, sig = np.asarray(ev, np.int64), np.asarray(tc, np.int64), np.asarray(sig, np.float64)
    want_v, want_c = R.path_cumulative(ev, tc, sig, n, step)
    v, c = bet_size_path(ev, tc, sig, n=n, step=step, return_count=True)
    assert v.dtype == np.float64 and c.dtype == np.int16 and len(v) == len(c) == n
    assert np.array_equal(c, want_c), np.flatnonzero(c != want_c)[:5]
    assert np.array_equal(v, want_v), np.flatnonzero(v != want_v)[:5]
    assert same_bits(v, want_v)
    assert np.array_equal(bet_size_path(ev, tc, sig, n=n, step=step), want_v)           # the launch without the count
    return v, c


def check_budget(ev, tc, side, n):
    from finmlkit_amd.label import bet_size_budget
    want, wl, ws = R.budget_cumulative(ev, tc, side, n)
    m, ml, ms = bet_size_budget(np.asarray(ev, np.int64), np.asarray(tc, np.int64), np.asarray(side, np.int8), n=n)
    assert (ml, ms) == (wl, ws)
    assert np.array_equal(m, want) and same_bits(m, want)
    return m, ml, ms


# ---------------------------------------------------------------------------------------------- the tape axis
def seam_spans(n):
    """spans that straddle, start on and end on every seam (multiples of the row and of the tile) below n, the whole tape, a lone
    event that ends on the last tick and a few random ones"""
    T, Rw, _ = geo()
    seams = np.arange(Rw, n, Rw, dtype=np.int64)
    ev = [seams - 1, seams, np.maximum(seams - 3, 0), [0], [max(n - 2, 0)]]
    tc = [np.minimum(seams + 1, n - 1), np.minimum(seams + 3, n - 1), seams, [n - 1], [n - 1]]
    rng = np.random.default_rng(n)
    rev = rng.integers(0, n, 50)
    ev.append(rev)
    tc.append(np.minimum(rev + rng.integers(0, 2 * T, 50), n - 1))
    ev, tc = np.concatenate([np.asarray(a, np.int64) for a in ev]), np.concatenate([np.asarray(a, np.int64) for a in tc])
    sig = rng.uniform(-1, 1, len(ev))
    sig[::5] = rng.choice(R.UNIT_SIGNALS, len(sig[::5]))
    return ev, tc, sig


AXIS = ["1", "2", "R-1", "R", "R+1", "T-1", "T", "T+1", "2T+1", "AT+1"]


def axis_n(key):
    T, Rw, A = geo()
    return {"1": 1, "2": 2, "R-1": Rw - 1, "R": Rw, "R+1": Rw + 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1,
            "AT+1": A * T + 1}[key]


@pytest.mark.parametrize("key", AXIS)
def test_tape_axis_seams(key):
    n = axis_n(key)
    ev, tc, sig = seam_spans(n)
    v, c = check_path(ev, tc, sig, n)
    assert c[n - 1] == 0 and v[n - 1] == 0.0                               # nothing is open on the last tick: bets close at the touch
    check_path(ev, tc, sig, n, 0.1)
    side = np.sign(sig).astype(np.int8)
    check_budget(ev, tc, side, n)


# ---------------------------------------------------------------------------------------------- extremes
@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_largest_sum_is_carried_across_tiles(sign):
    T, _, _ = geo()
    n, m = 2 * T + 1, R.MAX_CONC
    v, c = check_path(np.zeros(m, np.int64), np.full(m, n - 1, np.int64), np.full(m, sign), n)
    assert np.all(c[:n - 1] == m) and np.all(v[:n - 1] == sign) and v[n - 1] == 0.0 and not np.signbit(v[n - 1])
    # the same with one unit less per event, and a mixed tape on top of a pile of 32766
    check_path(np.zeros(m, np.int64), np.full(m, n - 1, np.int64), np.full(m, sign * (1 - 2.0 ** -30)), n, 0.05)
    ev = np.concatenate([np.zeros(m - 1, np.int64), [T - 1]])
    tc = np.concatenate([np.full(m - 1, n - 1, np.int64), [T + 1]])
    check_path(ev, tc, np.concatenate([np.full(m - 1, sign), [-sign]]), n)


def test_lone_and_repeated_events():
    T, _, _ = geo()
    n = 2 * T + 1
    v, c = check_path([n - 2], [n - 1], [0.75], n)                        # ends on the last tick
    assert c.sum() == 1 and v[n - 2] == 0.75
    v, c = check_path([T], [T], [0.75], n)                                # a skipped label: never open
    assert not c.any() and not v.any() and not np.signbit(v).any()
    v, c = check_path([0], [n - 1], [-0.3], n)
    assert np.all(c[:-1] == 1)
    v, c = check_path([7] * 1000, [T + 9] * 1000, [0.123456789] * 1000, n)          # the mean of equal signals is the signal's unit value
    assert np.all(c[7:T + 9] == 1000) and np.all(v[7:T + 9] == R.quantise(0.123456789) * 2.0 ** -30)


def test_units():
    n = 40
    for k, m in enumerate(R.UNIT_SIGNALS):
        v, _ = check_path([3], [9], [m], n)
        assert v[3] == R.quantise(m) * 2.0 ** -30 and not (v[3] == 0.0 and np.signbit(v[3])), m
    v, _ = check_path([0, 0], [5, 5], [2.0 ** -31, 3 * 2.0 ** -31], n)     # a tie gives 0 units, 3 half units give 2
    assert v[0] == 2.0 ** -30
    v, _ = check_path([0, 0, 0], [5, 5, 5], [-0.0, 0.0, -(2.0 ** -31)], n)
    assert v[0] == 0.0 and not np.signbit(v[0])
    rng = np.random.default_rng(1)
    sig = rng.choice(R.UNIT_SIGNALS, 400)
    ev = rng.integers(0, n, 400)
    check_path(ev, np.minimum(ev + rng.integers(0, 9, 400), n - 1), sig, n)


# ---------------------------------------------------------------------------------------------- refusals on the device
def small_valid_call():
    ev, tc, sig = np.array([1, 3, 3], np.int64), np.array([6, 5, 3], np.int64), np.array([0.5, -1.0, 1.0])
    v, c = check_path(ev, tc, sig, 9)
    assert v.tolist() == [0.0, 0.5, 0.5, -0.25, -0.25, 0.5, 0.0, 0.0, 0.0] and c.tolist() == [0, 1, 1, 2, 2, 1, 0, 0, 0]
    check_budget(ev, tc, [1, -1, 1], 9)


@pytest.mark.parametrize("count", [32768, 65535, 65536, 65537, 1 << 17])
def test_concurrency_above_int16_is_refused(count):
    """32 768 is the first count above the bound; the others are where a 16- or 17-bit count field would wrap to 0, 1 or a sign"""
    from finmlkit_amd.label import bet_size_at, bet_size_budget, bet_size_path
    T, _, _ = geo()
    n = 2 * T + 1
    ev, tc = np.full(count, T - 1, np.int64), np.full(count, T, np.int64)             # all of them open on one tick
    ev[0], tc[0] = 0, n - 1
    sig = np.where(np.arange(count) % 2, 1.0, -1.0)                        # the sum stays near zero: only the count tells
    with pytest.raises(ValueError, match=rf"concurrency of {count} "):
        bet_size_path(ev, tc, sig, n=n)
    with pytest.raises(ValueError, match=rf"concurrency of {count} "):
        bet_size_path(ev, tc, sig, n=n, step=0.5, return_count=True)
    with pytest.raises(ValueError, match=rf"concurrency of {count} "):
        bet_size_at(ev, tc, sig, n=n)
    for s in (1, -1):
        with pytest.raises(ValueError, match=rf"concurrency of {count} "):
            bet_size_budget(ev, tc, np.full(count, s, np.int8), n=n)
    small_valid_call()
    if count == 32768:                                                     # one fewer is served
        v, c = check_path(ev[1:], tc[1:], sig[1:], n)
        assert c[T - 1] == 32767
        check_budget(ev[1:], tc[1:], np.ones(count - 1, np.int8), n)


def c_abi(ev, tc, sig, n, step=0.0):
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import c_f64, c_i64, ptr
    ev, tc, sig = np.ascontiguousarray(ev, np.int64), np.ascontiguousarray(tc, np.int64), np.ascontiguousarray(sig, np.float64)
    v, c = np.empty(n), np.empty(n, np.int16)
    _ffi.default_context().call("fmk_bet_size_path", ptr(ev), ptr(tc), ptr(sig), c_i64(len(ev)), c_i64(n), c_f64(step), ptr(v), ptr(c))
    return v, c


def test_bad_signals_and_spans_are_counted_on_the_device():
    """the Python layer looks at host arrays itself, so these go to the C entries and to the resident methods"""
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.engine import DeviceTrades
    rng = np.random.default_rng(8)
    n, m = 5000, 10 ** 4
    ev = rng.integers(0, n - 50, m).astype(np.int64)
    tc = ev + rng.integers(0, 50, m)
    sig = rng.uniform(-1, 1, m)
    t = DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), np.ones(n), np.ones(n, np.float32))
    A = lambda a: DeviceArray.from_host(t.ctx, a)
    for bad, pattern in ((float("nan"), "1 signals are NaN"), (1.0000000000000002, "1 signals are NaN"), (-2.0, "1 signals are NaN")):
        s2 = sig.copy()
        s2[m // 2] = bad
        with pytest.raises(ValueError, match=pattern):
            c_abi(ev, tc, s2, n)
        with pytest.raises(ValueError, match=pattern):
            t.bet_size_path(A(ev), A(tc), A(s2))
        with pytest.raises(ValueError, match=pattern):
            t.bet_size_at(A(ev), A(tc), A(s2))
        small_valid_call()
    for e2, t2, pattern in ((ev[17] + 1, ev[17], "1 events outside"), (-1, 5, "1 events outside"), (n - 1, n, "1 events outside")):
        ev2, tc2 = ev.copy(), tc.copy()
        ev2[17], tc2[17] = e2, t2
        with pytest.raises(ValueError, match=pattern):
            c_abi(ev2, tc2, sig, n)
        with pytest.raises(ValueError, match=pattern):
            t.bet_size_path(A(ev2), A(tc2), A(sig))
        with pytest.raises(ValueError, match=pattern):
            t.bet_size_budget(A(ev2), A(tc2), A(np.ones(m, np.int8)))
        small_valid_call()
    with pytest.raises(ValueError, match="2 indices outside"):
        t.bet_size_at(A(ev), A(tc), A(sig), A(np.array([0, n, -1, n - 1], np.int64)))
    for step in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="step"):
            c_abi(ev, tc, sig, n, step)
    for ne, nn in ((0, n), (m, 0), (m, (1 << 32) + 1), (1 << 31, n)):
        from finmlkit_amd import _ffi
        from finmlkit_amd._ffi import c_f64, c_i64, ptr
        with pytest.raises(ValueError, match="must be between"):
            _ffi.default_context().call("fmk_bet_size_path", ptr(ev), ptr(tc), ptr(sig), c_i64(ne), c_i64(nn), c_f64(0.0), None, None)
    v, c = c_abi(ev, tc, sig, n)                                          # and the same arrays, untouched, are served
    want = R.path_cumulative(ev, tc, sig, n)
    assert np.array_equal(v, want[0]) and np.array_equal(c, want[1])


# ---------------------------------------------------------------------------------------------- against the existing kernel
def test_count_equals_label_concurrency_of_the_half_open_spans():
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import c_i64, ptr
    from finmlkit_amd.label import bet_size_path
    T, _, _ = geo()
    rng = np.random.default_rng(21)
    n, m = 3 * T + 77, 6000
    ev, tc, sig = R.random_case(rng, n, m, max_len=300)
    _, count = bet_size_path(ev, tc, sig, n=n, return_count=True)
    live = tc > ev
    lev, ltc = np.ascontiguousarray(ev[live]), np.ascontiguousarray(tc[live] - 1)
    conc = np.zeros(n, np.int16)
    _ffi.default_context().call("fmk_label_concurrency", ptr(lev), ptr(ltc), c_i64(len(lev)), c_i64(n), ptr(conc))
    assert (~live).any() and count.max() > 50
    assert np.array_equal(count, conc)


# ---------------------------------------------------------------------------------------------- budget
def test_budget():
    T, _, _ = geo()
    n = 2 * T + 100
    rng = np.random.default_rng(2)
    ev = rng.integers(0, n - 1, 500).astype(np.int64)
    tc = np.minimum(ev + rng.integers(0, 400, 500), n - 1)
    m, ml, ms = check_budget(ev, tc, np.ones(500, np.int8), n)            # all long
    assert ms == 0 and ml > 1 and m.max() == 1.0 and m.min() == 0.0
    m, ml, ms = check_budget(ev, tc, -np.ones(500, np.int8), n)           # all short
    assert ml == 0 and ms > 1 and m.min() == -1.0 and m.max() == 0.0
    m, ml, ms = check_budget(ev, tc, np.zeros(500, np.int8), n)           # side 0 counts nowhere
    assert (ml, ms) == (0, 0) and not m.any() and not np.signbit(m).any()
    # the maxima are attained in the last tile only
    ev2 = np.concatenate([ev % T, np.full(40, 2 * T + 10), np.full(60, 2 * T + 20)]).astype(np.int64)
    tc2 = np.concatenate([np.minimum(ev % T + 5, n - 1), np.full(40, 2 * T + 50), np.full(60, 2 * T + 60)]).astype(np.int64)
    side2 = np.concatenate([np.where(np.arange(500) % 2, 1, -1), np.ones(40), -np.ones(60)]).astype(np.int8)
    m, ml, ms = check_budget(ev2, tc2, side2, n)
    assert ml >= 40 and ms >= 60 and m[2 * T + 15] == 1.0 and m[2 * T + 55] == -1.0
    m, ml, ms = check_budget(ev2, tc2, side2 * 5, n)                      # only the sign of a side counts


@pytest.mark.parametrize("chunk", range(2))
def test_budget_campaign(chunk):
    T, _, _ = geo()
    rng = np.random.default_rng(300 + chunk)
    for k in range(60):
        n = int(rng.integers(1, 3 * T + 1))
        ne = int(rng.integers(1, 3000))
        ev, tc, _ = R.random_case(rng, n, ne, max_len=int(rng.integers(1, 600)))
        check_budget(ev, tc, rng.integers(-1, 2, ne), n)


# ---------------------------------------------------------------------------------------------- the campaign
@pytest.mark.parametrize("chunk", range(4))
def test_campaign(chunk):
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64
    T, _, _ = geo()
    ctx = _ffi.default_context()
    rng = np.random.default_rng(100 + chunk)
    steps = [0.0] + R.STEPS
    for k in range(75):
        n = int(rng.integers(1, 3 * T + 1))
        ne = int(rng.integers(1, 4000))
        ev, tc, sig = R.random_case(rng, n, ne, max_len=int(rng.integers(1, 800)))
        step = steps[(k + chunk) % len(steps)]
        v, c = check_path(ev, tc, sig, n, step)
        if k % 3 == 0:                                                     # the resident entry on the same case
            d = [DeviceArray.from_host(ctx, a) for a in (ev, tc, sig)]
            dv, dc = DeviceArray(ctx, n, np.float64), DeviceArray(ctx, n, np.int16)
            ctx.call("fmk_bet_size_path_dev", d[0].p, d[1].p, d[2].p, c_i64(ne), c_i64(n), c_f64(step), dv.p, dc.p)
            assert same_bits(dv.to_host(), v) and np.array_equal(dc.to_host(), c)
            # output pointers that are 8 but not 16 bytes aligned take the element-wise stores
            ov, oc = DeviceArray(ctx, n + 1, np.float64), DeviceArray(ctx, n + 1, np.int16)
            ctx.call("fmk_bet_size_path_dev", d[0].p, d[1].p, d[2].p, c_i64(ne), c_i64(n), c_f64(step), ov.view(1).p, oc.view(1).p)
            assert same_bits(ov.to_host()[1:], v) and np.array_equal(oc.to_host()[1:], c)


def test_runs_are_reproducible():
    from finmlkit_amd.label import bet_size_path
    T, _, _ = geo()
    rng = np.random.default_rng(77)
    n = 3 * T
    ev, tc, sig = R.random_case(rng, n, 20000, max_len=2000)               # heavy contention on the atomics
    first = bet_size_path(ev, tc, sig, n=n)
    for _ in range(3):
        assert same_bits(bet_size_path(ev, tc, sig, n=n), first)
    order = rng.permutation(len(ev))
    assert same_bits(bet_size_path(ev[order], tc[order], sig[order], n=n), first)


# ---------------------------------------------------------------------------------------------- gather
def test_gather():
    from finmlkit_amd.label import avg_active_signals, bet_size_at
    T, _, _ = geo()
    rng = np.random.default_rng(5)
    n = T + 300
    ev, tc, sig = R.random_case(rng, n, 800, max_len=200)
    ev[0], tc[0] = 0, n - 1
    for step in (0.0, 0.1):
        path, _ = R.path_cumulative(ev, tc, sig, n, step)
        assert same_bits(bet_size_at(ev, tc, sig, n=n, step=step), path[ev])           # the default: each event's own tick
        at = np.array([0, n - 1, 5, 5, 5, n - 1, 0, T, T - 1], np.int64)                 # first and last tick, repeats
        assert same_bits(bet_size_at(ev, tc, sig, at, n=n, step=step), path[at])
        empty = bet_size_at(ev, tc, sig, np.zeros(0, np.int64), n=n, step=step)
        assert empty.shape == (0,) and empty.dtype == np.float64
        every = np.arange(n, dtype=np.int64)
        assert same_bits(bet_size_at(ev, tc, sig, every, n=n, step=step), path)
        points, values = avg_active_signals(ev, tc, sig, n=n, step=step)
        assert np.array_equal(points, np.union1d(ev, tc)) and same_bits(values, path[points])
    points, values = avg_active_signals(ev, tc, sig)
    bp, bm = R.book_avg_active_signals(ev, tc, sig)
    assert np.array_equal(points, bp) and float(np.max(np.abs(values - bm))) <= 2.0 ** -30


# ---------------------------------------------------------------------------------------------- the resident forms and the kit
def test_resident_forms_and_kit_after_triple_barrier():
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.engine import DeviceTrades
    from finmlkit_amd.label import BetSizing, signal_from_probability
    n = 60_000
    t = DeviceTrades.synth(n, seed=7)
    ev = np.arange(100, n - 100, 37, dtype=np.int64)
    m = len(ev)
    A = lambda a: DeviceArray.from_host(t.ctx, a)
    d_ev = A(ev)
    out = t.triple_barrier(d_ev, A(np.full(m, 2e-4)), (1.0, 1.0), 20.0, 0.0)
    d_tc = out[1]
    tc = d_tc.to_host()
    assert np.all(tc >= ev) and (tc > ev).sum() > m // 2 and np.unique(tc - ev).size > 5
    rng = np.random.default_rng(9)
    prob = rng.uniform(0.34, 1.0, m)
    pred = rng.choice([-1, 1], m)
    sig = signal_from_probability(prob, pred, n_classes=3)
    side = pred.astype(np.int8)
    for step in (0.0, 0.05):
        want_v, want_c = R.path_cumulative(ev, tc, sig, n, step)
        v, c = t.bet_size_path(d_ev, d_tc, A(sig), step, return_count=True)
        assert isinstance(v, DeviceArray) and v.n == c.n == n and v.dtype == np.float64 and c.dtype == np.int16
        assert same_bits(v.to_host(), want_v) and np.array_equal(c.to_host(), want_c)
        assert same_bits(t.bet_size_path(d_ev, d_tc, A(sig), step).to_host(), want_v)
        assert same_bits(t.bet_size_at(d_ev, d_tc, A(sig), step=step).to_host(), want_v[ev])
        at = np.array([0, n - 1, geo()[0], geo()[0]], np.int64)             # first and last tick, a tile seam twice
        assert same_bits(t.bet_size_at(d_ev, d_tc, A(sig), A(at), step).to_host(), want_v[at])
        # the kit on the frame of the labels; its axis ends at the last touch, which changes nothing at the events
        frame = pd.DataFrame({"event_idx": ev, "touch_idx": tc}, index=pd.to_datetime(ev))
        got = BetSizing.from_probabilities(frame, prob, pred, n_classes=3, step=step)
        assert list(got.columns) == ["signal", "bet_size"] and got.index.equals(frame.index)
        assert same_bits(got["signal"].values, sig) and same_bits(got["bet_size"].values, want_v[ev])
        frame["side"] = side                                               # meta labels: the side multiplies the signal
        meta = BetSizing.from_probabilities(frame, prob, n_classes=3, step=step)
        assert same_bits(meta["signal"].values, sig) and same_bits(meta["bet_size"].values, want_v[ev])
    assert want_c.max() > 3
    bm, bl, bs = R.budget_cumulative(ev, tc, side, n)
    d_m, d_max = t.bet_size_budget(d_ev, d_tc, A(side))
    assert same_bits(d_m.to_host(), bm) and d_max.to_host().tolist() == [bl, bs] and d_max.dtype == np.int64
    with pytest.raises(ValueError, match="same length"):
        t.bet_size_path(d_ev, d_tc, A(sig[:-1]))
    with pytest.raises(TypeError, match="float64"):
        t.bet_size_path(d_ev, d_tc, A(sig.astype(np.float32)))
    with pytest.raises(TypeError, match="int64"):
        t.bet_size_path(A(ev.astype(np.int32)), d_tc, A(sig))
    with pytest.raises(TypeError, match="int8"):
        t.bet_size_budget(d_ev, d_tc, A(side.astype(np.int64)))
    with pytest.raises(ValueError, match="step"):
        t.bet_size_at(d_ev, d_tc, A(sig), step=2.0)
