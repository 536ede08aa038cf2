"""Triple-barrier labels and sample weights on the MI355X where the data is not clean: zero, negative, NaN, infinite and subnormal
prices at event ticks and on paths, odd targets, side 0, odd barrier multipliers (tests/golden/labels_odd.*, recorded from the
reference), planted geometry for the table walk, the second table level past one full wave of 64 entries, and weights whose
whole-block sums hold concurrency <= 0 and odd prices.  Yardstick: tests/_label_ref.py."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import _counts
from tests import _label_ref as H
from tests.test_gpu_labels import BLOCK, assert_bits, diag_last, forced
from tests.test_labels_host import ODD, ODD_WEIGHTS

pytestmark = pytest.mark.gpu

FAN = 64                # table entries per entry of the second level (csrc/fmk_label.hip)
NAMES = ("labels", "touch_idx", "returns", "ratios")


def assert_events(got, want, ev, what):
    """All four outputs of every event bit for bit (NaN == NaN, the sign of an infinity counts); names the first event that
    differs, with its tick and both sets of outputs."""
    bad = np.zeros(len(ev), bool)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, what
        bad |= (g != w) & ~(np.isnan(g) & np.isnan(w)) if g.dtype.kind == "f" else g != w
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        print(f"{what}: {int(bad.sum())} of {len(ev)} events differ; first: event {i} at tick {int(ev[i])}: got "
              f"{[np.asarray(g)[i].item() for g in got]}, want {[np.asarray(w)[i].item() for w in want[:4]]}")
    for g, w, k in zip(got, want, NAMES):
        assert_bits(g, w, f"{what}/{k}")
    assert not bad.any(), what


def run_tb(ts, px, ev, tg, hb, vb, mc, side, min_ret, schedule):
    from finmlkit_amd import _ffi, label
    with forced(schedule), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # skipped events announce themselves
        got = label.triple_barrier(ts, px, ev, tg, hb, vb, mc, side, min_ret)
    d = diag_last(_ffi.default_context())
    assert d["events"] == len(ev)
    if schedule:
        assert d["schedule"] == (schedule == "long")
    return got, d


# ---------------------------------------------------------------------------------------------- (a) the recorded fixture
@pytest.mark.parametrize("schedule", ["direct", "long", None])
@pytest.mark.parametrize("name", sorted(ODD))
def test_odd_fixture_replay(name, schedule):
    c = ODD[name]
    args = (c["ts"], c["close"], c["event_idx"], c["targets"], c["hb"], c["vb"], c["mc"], c["side"], c["min_ret"])
    got, d = run_tb(*args, schedule)
    assert d["skipped"] == c["n_skipped"] == c["skipped"].sum()
    want = [c[k].copy() for k in NAMES]
    out = ~c["recorded"]                                         # side=None with a NaN final return: the yardstick alone
    if out.any():
        y = H.triple_barrier_scalar(c["ts"], c["close"], c["event_idx"][out], c["targets"][out], c["hb"], c["vb"], c["mc"], None,
                                    c["min_ret"])
        for w, v in zip(want, y):
            w[out] = v
    assert_events(got, want, c["event_idx"], f"odd/{name}/{schedule}")
    _counts.record(f"labels_odd/replay/{name}/{schedule or 'default'}", events_compared=len(out), events_left_out=0,
                   events_skipped=int(c["skipped"].sum()), against_yardstick_only=int(out.sum()))


# ---------------------------------------------------------------------------------------------- (b) planted geometry
def plain_tape(blocks=8, extra=100, seed=3):
    n = blocks * BLOCK + extra
    rng = np.random.default_rng(seed)
    ts = 1_700_000_000_000_000_000 + np.arange(n, dtype=np.int64) * 1_000_000
    px = np.round(100.0 * np.exp(np.cumsum(rng.normal(0, 1e-4, n))), 2)
    return ts, px


def check_planted(ts, px, ev, tg, hb, vb, mc, side, min_ret, schedule, name):
    ev, tg = np.asarray(ev, np.int64), np.asarray(tg, np.float64)
    side = None if side is None else np.asarray(side, np.int8)
    want = H.triple_barrier_scalar(ts, px, ev, tg, hb, vb, mc, side, min_ret)
    assert not want[4].any()
    got, d = run_tb(ts, px, ev, tg, hb, vb, mc, side, min_ret, schedule)
    assert d["skipped"] == 0
    assert_events(got, want, ev, f"planted/{name}/{schedule}")
    return want


@pytest.mark.parametrize("schedule", ["direct", "long"])
def test_planted_geometry(schedule):
    inf, nan = np.inf, np.nan
    compared = 0
    k = 3
    # an event on a zero (an infinite) price at the last tick of a block; the next block holds one more such price and otherwise
    # positive ones, two more whole blocks follow: the touch is the first positive tick of block k, ret = +inf (-inf)
    for odd, sign in ((0.0, 1.0), (-0.0, 1.0), (inf, -1.0)):
        for second in (0, 1, 500, BLOCK - 1):                    # where in block k the second odd price sits
            ts, px = plain_tape()
            px[k * BLOCK - 1] = odd
            px[k * BLOCK + second] = odd
            first = k * BLOCK + (1 if second == 0 else 0)
            for side, hb in ((None, (1.0, 1.0)), ([1], (1.0, 1.0)), ([-1], (1.0, 1.0)), (None, (inf, 1.0)), (None, (1.0, inf))):
                w = check_planted(ts, px, [k * BLOCK - 1], [0.01], hb, inf, 0.0, side, 0.0, schedule, f"base{odd}/{second}")
                s = 1.0 if side is None else side[0]
                assert w[1][0] == first and w[2][0] == sign * s * inf and w[3][0] == 1.0
                compared += 1
    # side 0 with target 0: +-0.0 reaches both barriers at the first evaluable tick, a zero price (NaN * 0) does not
    for zero_at in (0, 300):
        ts, px = plain_tape()
        px[k * BLOCK + zero_at] = 0.0
        w = check_planted(ts, px, [k * BLOCK - 1, k * BLOCK - 500, 5], [0.0, 0.0, 0.0], (1.0, 1.0), inf, 0.0, [0, 0, 0], 0.0,
                          schedule, f"side0/{zero_at}")
        assert w[1][0] == k * BLOCK + (zero_at == 0) and w[1][2] == 6
        w = check_planted(ts, px, [k * BLOCK - 1, k * BLOCK - 500, 5], [0.02, -0.02, nan], (1.0, 1.0), inf, 0.0, [0, 0, 0], 0.0,
                          schedule, f"side0_targets/{zero_at}")
        assert w[1][0] == len(ts) - 1 and np.isnan(w[3][2])
        compared += 6
    # side 0, target 0, a block that opens with a zero price and holds an infinite one: its extrema are (-inf, +inf), both images
    # NaN, and still its first finite tick has ret = +-0.0 and touches
    ts, px = plain_tape()
    px[k * BLOCK], px[k * BLOCK + 1], px[k * BLOCK + 700] = 0.0, -2.0, inf
    w = check_planted(ts, px, [k * BLOCK - 1, k * BLOCK - 1], [0.0, -0.01], (1.0, 1.0), inf, 0.0, [0, 0], 0.0, schedule, "side0/both")
    assert w[1][0] == k * BLOCK + 2 and w[1][1] == k * BLOCK + 2
    compared += 2
    # an all-NaN block and an all-zero block in the middle of a window
    ts, px = plain_tape()
    px[2 * BLOCK:3 * BLOCK] = nan
    px[4 * BLOCK:5 * BLOCK] = 0.0
    ev = [100, 100, 100, BLOCK - 1, 2 * BLOCK - 1, 2 * BLOCK + 7, 3 * BLOCK - 1, 4 * BLOCK - 1, 4 * BLOCK, 5 * BLOCK - 1]
    tg = [10.0, nan, 1e-3, 10.0, 10.0, 10.0, nan, 10.0, 10.0, 10.0]
    for side in (None, [1, -1, 1, -1, 1, 0, 1, -1, 1, -1]):
        for hb in ((1.0, 1.0), (inf, 1.0), (1.0, inf)):
            w = check_planted(ts, px, ev, tg, hb, inf, 0.0, side, 0.0, schedule, f"blocks/{hb}")
            compared += len(ev)
    assert w[1][1] == len(ts) - 1                                # NaN barriers: over both blocks to the end
    w = check_planted(ts, px, ev, tg, (1.0, 1.0), 5.5, 0.0025, None, 0.0, schedule, "blocks/vb")
    compared += len(ev)
    # a NaN where the window's maximum was: the extrema leave out that tick and nothing else
    ts, px = plain_tape()
    top = 5 * BLOCK + 333
    px[top] = px.max() + 0.5                                     # the one tick that carries the window's maximum
    px[-1] = px[100] * 1.0001                                    # the path ends above its base: the ratio is max / U
    clean = H.triple_barrier_scalar(ts, px, np.array([100]), np.array([0.5]), (1.0, 1.0), inf, 0.0, None, 0.0)
    px[top] = nan
    for e in (100, BLOCK - 1, BLOCK):
        w = check_planted(ts, px, [e], [0.5], (1.0, 1.0), inf, 0.0, None, 0.0, schedule, "nan_at_max")
        assert w[1][0] == len(ts) - 1 and 0.0 < w[3][0] < 1.0
        compared += 1
    w = check_planted(ts, px, [100], [0.5], (1.0, 1.0), inf, 0.0, None, 0.0, schedule, "nan_at_max")
    assert w[3][0] < clean[3][0]                                 # the planted tick did carry the maximum
    second = np.nanmax(H.log_column(px[101:])) - H.host_log(px[100])
    assert w[3][0] == (second / 0.5) / (1 + w_lower(px, 100, 0.5))
    _counts.record(f"labels_odd/planted/{schedule}", events_compared=compared, events_left_out=0)


def w_lower(px, i0, tgt):
    lc = H.log_column(px[i0:])
    return max(0.0, float(np.nanmin(lc[1:]) - lc[0]) / -tgt)


# ---------------------------------------------------------------------------------------------- (c) level 2 at full fan-out
N_BIG = 67 * FAN * BLOCK + 1500
GROUP = FAN * BLOCK                                              # ticks per entry of the second level
DOWN_1, UP_2, UP_3 = 64 * GROUP, 65 * GROUP + GROUP - 1, 67 * GROUP + BLOCK + 200
BAND = 1e-3


@pytest.fixture(scope="module")
def big_tape():
    """log prices folded into [-BAND, BAND] on a grid of 1e-4 in price, three spikes: down at the first tick of group 64, up at the
    last tick of group 65, a taller one up in the tail behind the last whole block."""
    rng = np.random.default_rng(12)
    x = np.cumsum(rng.normal(0, 1e-5, N_BIG))
    x = np.abs((x + BAND) % (4 * BAND) - 2 * BAND) - BAND
    px = np.round(100.0 * np.exp(x), 4)
    px[DOWN_1], px[UP_2], px[UP_3] = np.round(100.0 * np.exp([-0.010, 0.010, 0.020]), 4)
    px[-1] = 100.0
    values, inverse = np.unique(px, return_inverse=True)
    lc = H.log_column(values)[inverse]                           # the host's log once per distinct price
    ts = np.arange(N_BIG, dtype=np.int64) * 1_000_000
    rel = lc - H.host_log(100.0)
    assert abs(rel[UP_2] - 0.010) < 1e-6 and np.abs(np.delete(rel, [DOWN_1, UP_2, UP_3])).max() < BAND + 1e-6
    return ts, px, lc


def big_events(rng, call):
    """-> event ticks, targets, index ranges (short, planted, to_end)"""
    fixed = np.array([0, 1, GROUP - 1, GROUP, GROUP + 1], np.int64)
    short = np.concatenate([fixed, rng.choice(np.arange(2, DOWN_1 - 10_000), 295, replace=False)])
    t_short = 3e-4 * (0.5 + rng.random(len(short)))
    # targets between the band and the spikes: the first touch is a spike, whole groups away
    planted = np.concatenate([fixed, rng.choice(DOWN_1 - 1, 15, replace=False), [DOWN_1 - 1, DOWN_1 - BLOCK, DOWN_1 + 1,
                              DOWN_1 + 2 * GROUP - 2 * BLOCK, UP_2 - 1, UP_2 + 1, 66 * GROUP, 67 * GROUP + BLOCK - 1, UP_3 - 1]])
    t_planted = np.where(rng.random(len(planted)) < 0.5, 5e-3, 15e-3) * (1 + 0.2 * rng.random(len(planted)))
    t_planted[:2] = 5e-3, 15e-3
    to_end = np.concatenate([fixed, rng.choice(N_BIG - 2, {"A": 15, "B": 35, "C": 15}[call], replace=False), [UP_3 + 1]])
    t_end = 0.05 * (1 + rng.random(len(to_end)))
    ev = np.concatenate([short, planted, to_end]).astype(np.int64)
    tg = np.concatenate([t_short, t_planted, t_end])
    a, b = len(short), len(short) + len(planted)
    return ev, tg, slice(0, a), slice(a, b), slice(b, len(ev))


@pytest.mark.parametrize("call", ["A", "B", "C"])
def test_second_level_at_full_fan_out(big_tape, call):
    ts, px, lc = big_tape
    inf = np.inf
    rng = np.random.default_rng({"A": 1, "B": 2, "C": 3}[call])
    ev, tg, short, planted, to_end = big_events(rng, call)
    hb, mc, side = {"A": ((1.0, 1.0), 0.0, None), "B": ((inf, 1.0), 0.0025, rng.choice([-1, 1], len(ev)).astype(np.int8)),
                    "C": ((1.0, inf), 0.0, None)}[call]
    if side is not None:
        side[planted] = 1
        side[to_end.start:to_end.start + 3] = 0                  # side 0 reaches no barrier: to the last tick
    min_ret = 0.0 if side is None else 1e-5
    want = H.triple_barrier(ts, px, ev, tg, hb, inf, mc, side, min_ret, log_close=lc)
    assert not want[4].any()
    at_end = want[1] == N_BIG - 1
    assert 10 <= at_end.sum() <= 64                              # the events that cost the CPU a pass over the tape
    pinned = at_end & ~np.isnan(want[3]) & (want[3] > 0) & (want[3] < 1)
    assert pinned.sum() >= 10                                    # their ratio is a table extremum over U or L, bit for bit
    touches = set(want[1][planted].tolist())
    assert {"A": {DOWN_1, UP_2, UP_3}, "B": {UP_2, UP_3}, "C": {DOWN_1}}[call] <= touches
    if call == "B":                                              # min_close_time moved a first open tick past a block boundary
        assert H.first_open(ts, GROUP - 1, N_BIG - 1, mc * 1e9) == GROUP + 2
    whole_groups = (want[1] // GROUP - (ev + GROUP) // GROUP)[planted]
    assert whole_groups[0] >= 63 and whole_groups[1] >= 63       # from ticks 0 and 1: a full wave of second-level entries
    for schedule in ("long", None):
        got, d = run_tb(ts, px, ev, tg, hb, inf, mc, side, min_ret, schedule)
        assert_events(got, want, ev, f"fanout/{call}/{schedule}")
        assert d["schedule"] == 1 and d["skipped"] == 0 and d["opened"] <= len(ev)
        # a head of under 1 024 ticks, at most one opened block, a tail of under 1 024 ticks: geometry, not a measurement
        assert d["walked"] < 3 * BLOCK * len(ev)
        _counts.record(f"labels_odd/fanout/{call}/{schedule or 'default'}", events_compared=len(ev), events_left_out=0,
                       to_the_last_tick=int(at_end.sum()), ratio_pins_extremum=int(pinned.sum()), opened=d["opened"],
                       walked=d["walked"])
    s = short
    got, d = run_tb(ts, px, ev[s], tg[s], hb, inf, mc, None if side is None else side[s], min_ret, "direct")
    assert_events(got, [w[s] for w in want[:4]], ev[s], f"fanout/{call}/direct")
    _counts.record(f"labels_odd/fanout/{call}/direct", events_compared=len(ev[s]), events_left_out=0)


# ---------------------------------------------------------------------------------------------- (d) weights through block sums
def abi_weights(px, conc, ev, tch):
    """fmk_label_weights with the caller's concurrency column -> (average uniqueness, return attribution)"""
    from finmlkit_amd import _ffi
    px, conc = np.ascontiguousarray(px, np.float64), np.ascontiguousarray(conc, np.int16)
    ev, tch = np.ascontiguousarray(ev, np.int64), np.ascontiguousarray(tch, np.int64)
    avg, att = np.empty(len(ev)), np.empty(len(ev))
    _ffi.default_context().call("fmk_label_weights", _ffi.ptr(px), _ffi.ptr(conc), C.c_int64(len(px)), _ffi.ptr(ev), _ffi.ptr(tch),
                                C.c_int64(len(ev)), _ffi.ptr(avg), _ffi.ptr(att))
    return avg, att


def compare_weights(got, want, tol, what):
    """finite yardstick: within tol; +-inf or NaN: the same infinity or NaN.  -> events compared (all of them)"""
    got, want, tol = np.asarray(got), np.asarray(want), np.asarray(tol)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got[fin] - want[fin])
    worst = float(np.max(err / np.maximum(tol[fin], 1e-300))) if fin.any() else 0.0
    print(f"{what}: {int(fin.sum())} finite, max err / tol {worst:.3g}; {int((~fin).sum())} not finite")
    assert np.all(np.isfinite(got[fin])) and np.all(err <= tol[fin]), what
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    return int(fin.sum()), int((~fin).sum())


def check_weights_given(px, conc, ev, tch, name, want_att=None):
    """the C ABI and label.return_attribution under a concurrency column of the caller's"""
    from finmlkit_amd import label
    wavg, scale = H.uniqueness_given(conc, ev, tch)
    watt, bound = H.return_attribution(ev, tch, px, conc, False)
    if want_att is not None:
        watt = want_att
    avg, att = abi_weights(px, conc, ev, tch)
    f1, o1 = compare_weights(avg, wavg, 1e-9 * scale, name + "/avg_uniqueness")
    f2, o2 = compare_weights(att, watt, bound, name + "/attribution")
    att2 = label.return_attribution(ev, tch, px, conc, False)
    assert_bits(att2, att, name + "/package == ABI")
    assert f1 + o1 == len(ev) and f2 + o2 == len(ev)
    _counts.record(f"labels_odd/weights/{name}", events_compared=len(ev), events_left_out=0, avg_not_finite=o1,
                   attribution_not_finite=o2)
    return o1, o2


@pytest.mark.parametrize("name", sorted(ODD_WEIGHTS))
def test_weights_fixture(name):
    from finmlkit_amd import label
    w = ODD_WEIGHTS[name]
    ts, px, ev, tch = w["ts"], w["close"], w["event_idx"], w["touch_idx"]
    avg, conc = label.average_uniqueness(ts, ev, tch)
    assert_bits(conc, w["concurrency"], name + "/concurrency")
    _, scale = H.uniqueness_given(conc, ev, tch)
    compare_weights(avg, w["avg_uniqueness"], 1e-9 * scale, name + "/avg_uniqueness")
    o1, o2 = check_weights_given(px, w["concurrency"], ev, tch, name + "/own", w["return_attribution"])
    assert o1 == 0 and o2 >= 20
    o1, o2 = check_weights_given(px, w["hand_concurrency"], ev, tch, name + "/hand", w["return_attribution_hand"])
    assert o1 >= 20 and o2 >= 20


def test_weights_on_odd_prices_and_concurrency(orc):
    n = 200_000
    ts, px, _, _ = orc.synth(21, 0, n)
    rng = np.random.default_rng(21)
    ne = 1500
    ev = rng.choice(n - 2, ne, replace=False).astype(np.int64)
    length = np.where(rng.random(ne) < 0.3, rng.integers(0, 60_000, ne), rng.integers(0, 3000, ne))
    tch = np.minimum(ev + length, n - 1)
    ev[:4], tch[:4] = [0, BLOCK - 1, BLOCK, 150 * BLOCK], [n - 1, BLOCK, 2 * BLOCK - 1, 150 * BLOCK]
    px = px.copy()
    odd = [0.0, -0.0, np.nan, -7.0, np.inf, 5e-324]
    for i, b in enumerate(range(20, 100, 4)):                    # around block boundaries, in the first half of the tape
        for off in (-1, 0, 1):
            px[b * BLOCK + off] = odd[(i + off) % 6]
    px[rng.choice(n // 2, 40, replace=False)] = np.nan
    conc = H.concurrency(n, ev, tch)
    o1, o2 = check_weights_given(px, conc, ev, tch, "tape/own")
    assert o1 == 0 and 20 <= o2 <= ne - 200
    hand = conc.copy()
    for b in range(100, 190, 6):                                 # runs of 0 and of negative counts across block boundaries
        hand[b * BLOCK - 300:b * BLOCK + 200] = 0 if b % 12 else -3
    hand[120 * BLOCK + 17:127 * BLOCK + 5] = -32768              # whole blocks of a wrapped-around count
    hand[130 * BLOCK:132 * BLOCK] = 0                            # whole blocks of zeros
    o1, o2 = check_weights_given(px, hand, ev, tch, "tape/hand")
    assert 20 <= o1 <= ne - 200 and o2 >= 20
