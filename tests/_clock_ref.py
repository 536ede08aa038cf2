"""NumPy restatement of the bar-clock, run-length and opening-range features (finmlkit_amd/feature/core/clock.py, csrc/fmk_clock.hip)
and the seeded inputs of their tests.  tools/gen_clock_golden.py holds every function here against the untouched reference before it
writes tests/golden/clock.npz; tests/test_clock_host.py and tests/test_gpu_clock.py regenerate the inputs from the recorded sources.

  bar_duration(ts, periods)        (ts[i] - ts[i - periods]) / 10**9 where the lagged row exists, NaN elsewhere
  bar_duration_ewma(ts, span)      NaN at 0; u = d + (1 - alpha) u, v = 1 + (1 - alpha) v from (d[1], 1), u / v (a sequential loop)
  bar_rate(ts, window_sec)         (i - searchsorted(ts, ts[i] - w, 'left') + 1) / window_sec * 3600, w = Timedelta(seconds=...).value
  dir_run_len(x)                   a running maximum over the indices where a run starts; the low 8 bits as int8
  orb_break(ts, high, low, close)  the same running maximum over day starts; fmax / fmin over the four opening rows
"""
import hashlib

import numpy as np
import pandas as pd

DAY = 86_400_000_000_000
MINUTE = 60_000_000_000
SECOND = 1_000_000_000
BASE = 1_704_067_200_000_000_000          # 2024-01-01T00:00:00Z
FUNCTIONS = ("dur", "dew", "rate", "run", "orb")
EXACT = {"dur": True, "dew": False, "rate": True, "run": True, "orb": True}
DEW_BOUND = 1e-9                          # the project's contract for recurrence scans (README, parity contract)


# ---------------------------------------------------------------------------------------------------------------- restatement
def bar_duration(ts, periods=1):
    ts = np.asarray(ts, np.int64)
    n = len(ts)
    out = np.full(n, np.nan)
    ii = np.arange(n)
    ii = ii[(ii - int(periods) >= 0) & (ii - int(periods) < n)]
    out[ii] = (ts[ii] - ts[ii - int(periods)]) / 10**9
    return out


def bar_duration_ewma(ts, span=20):
    if not float(span) >= 1.0:
        raise ValueError("span size is less than or equal to 1. Please provide a span size greater than 1.")
    ts = np.asarray(ts, np.int64)
    n = len(ts)
    out = np.full(n, np.nan)
    if n < 2:
        return out
    d = ((ts[1:] - ts[:-1]) / 10**9).tolist()
    a = 1.0 - 2.0 / (float(span) + 1.0)
    u, v = d[0], 1.0
    res = [u / v]
    for x in d[1:]:
        u = x + a * u
        v = 1.0 + a * v
        res.append(u / v)
    out[1:] = res
    return out


def window_ns(window_sec):
    return int(pd.Timedelta(seconds=float(window_sec)).value)


def bar_rate(ts, window_sec):
    w = window_ns(window_sec)
    if w < 1:
        raise ValueError("bar_rate: the window must be at least one nanosecond.")
    ts = np.asarray(ts, np.int64)
    lb = np.searchsorted(ts, ts - w, side="left")
    return (np.arange(len(ts)) - lb + 1).astype(np.float64) / float(window_sec) * 3600.0


def _last_head(head):
    idx = np.arange(len(head))
    return np.maximum.accumulate(np.where(head, idx, 0))


def dir_run_len(x):
    x = np.asarray(x, np.float64)
    n = len(x)
    if n == 0:
        return np.zeros(0, np.int8)
    with np.errstate(invalid="ignore"):
        s = np.sign(x)
    head = np.zeros(n, bool)
    head[1:] = s[1:] != s[:-1]                      # a NaN is unequal to everything
    if n > 1:
        head[1] = True
    head[0] = False
    run = np.where(s != 0, np.arange(n) - _last_head(head) + 1, 0)
    run[0] = 0
    return (run & 0xFF).astype(np.uint8).view(np.int8)


def orb_break(ts, high, low, close):
    ts = np.asarray(ts, np.int64)
    high, low, close = (np.asarray(a, np.float64) for a in (high, low, close))
    n = len(ts)
    if n == 0:
        return np.zeros(0, bool), np.zeros(0, bool)
    day = ts // DAY                                 # floor, also before 1970
    head = np.ones(n, bool)
    head[1:] = day[1:] != day[:-1]
    s = _last_head(head)
    idx = np.arange(n)
    ok = (ts[s] - day * DAY < MINUTE) & (idx - s >= 4)
    rows = [np.minimum(s + k, n - 1) for k in range(4)]
    hi = np.fmax.reduce([high[r] for r in rows])    # NaN skipped; NaN when all four are
    lo = np.fmin.reduce([low[r] for r in rows])
    with np.errstate(invalid="ignore"):
        return ok & (close > hi), ok & (close < lo)


def call(fn, inputs, args):
    f = {"dur": bar_duration, "dew": bar_duration_ewma, "rate": bar_rate, "run": dir_run_len, "orb": orb_break}[fn]
    out = f(*inputs, *args)
    return out if isinstance(out, tuple) else (out,)


# ---------------------------------------------------------------------------------------------------------------- comparison
def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def dew_deviation(got, want):
    """The largest relative deviation of bar_duration_ewma, or None where the NaN positions differ; where want is 0.0 got must be."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return None
    m = ~np.isnan(want)
    z = m & (want == 0.0)
    if np.any(got[z] != 0.0):
        return np.inf
    m &= want != 0.0
    return float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m]))) if m.any() else 0.0


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + b"|" + a.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
def stamps(n, seed, dup=0.15, step=1_000_000, max_steps=2000, start=BASE + 37 * 3_600 * SECOND + 123_456_789):
    """Non-decreasing stamps: gaps of 1 .. max_steps steps of `step` ns, a fraction `dup` of them zero (duplicate stamps)."""
    rng = np.random.default_rng(seed)
    gaps = rng.integers(1, max_steps + 1, size=n).astype(np.int64) * step
    gaps[rng.random(n) < dup] = 0
    gaps[:1] = 0
    return (start + np.cumsum(gaps),)


def regular(n, step_ns):
    return (BASE + np.arange(n, dtype=np.int64) * int(step_ns),)


def stamps_dup_at(n, seed, at, run):
    """`stamps` without duplicates but for one run of `run` equal stamps that starts at row `at`."""
    (ts,) = stamps(n, seed, dup=0.0)
    gaps = np.diff(ts, prepend=ts[:1])
    gaps[at + 1:at + run] = 0
    return (ts[0] + np.cumsum(gaps),)


def wide_stamps():
    return (np.array([-(2**62), -5, 0, 2**53 + 1, 2**62 + 7, 2**62 + 7, 2**62 + 2**40 + 1], np.int64),)


def returns(n, seed, p_flip=0.35, odd=0.08):
    """Returns with runs of one sign, and zeros, -0.0, NaN and +-inf mixed in."""
    rng = np.random.default_rng(seed)
    flips = rng.random(n) < p_flip
    sign = np.where(np.cumsum(flips) % 2 == 0, 1.0, -1.0)
    x = sign * rng.integers(1, 1000, size=n) / 1024.0
    kind = rng.random(n)
    pick = rng.integers(0, 5, size=n)
    spot = kind < odd
    x[spot] = np.array([0.0, -0.0, np.nan, np.inf, -np.inf])[pick[spot]]
    return (x,)


def run_pattern(lengths, first=1.0, lead=1):
    """`lead` zeros, then runs of the given lengths with alternating signs starting with `first`."""
    parts, s = [np.zeros(lead)], first
    for k in lengths:
        parts.append(np.full(int(k), s * 0.5))
        s = -s
    return (np.concatenate(parts),)


def edited(source, edits):
    """The arrays of `source` with (array, row, value) edits; the value as a string ("nan", "-0.0", "inf")."""
    arrays = [np.array(a) for a in generate(source)]
    for k, row, value in edits:
        arrays[k][row] = float(value)
    return tuple(arrays)


def hlc(n, seed):
    """high / low / close on a quarter grid, so that a close meets the opening range exactly now and then."""
    rng = np.random.default_rng(seed)
    mid = 100.0 + np.cumsum(rng.integers(-2, 3, size=n)) * 0.25
    high = mid + rng.integers(0, 3, size=n) * 0.25
    low = mid - rng.integers(0, 3, size=n) * 0.25
    close = low + rng.integers(0, 5, size=n) * (high - low) / 4.0
    return high, low, close


def orb_tape(spec, seed):
    """Days as [day number, offset of the first row in ns, rows, step in ns] -> (ts, high, low, close), strictly increasing stamps."""
    ts = np.concatenate([d * DAY + off + np.arange(rows, dtype=np.int64) * step for d, off, rows, step in spec])
    assert np.all(np.diff(ts) > 0)
    return (ts, *hlc(len(ts), seed))


def orb_walk(n, seed, day0=19_800):
    """n rows in days of 1 .. 12 rows that start 0 s, 30 s, 59.999999999 s or 60 s into the day, a calendar day skipped now and then;
    the first day is day0 (days since 1970)."""
    rng = np.random.default_rng(seed)
    spec, day, left = [], int(day0), n
    while left > 0:
        rows = int(min(left, rng.integers(1, 13)))
        off = int(np.array([0, 30 * SECOND, MINUTE - 1, MINUTE])[rng.integers(0, 4)])
        spec.append([day, off, rows, 15 * MINUTE])
        day += int(rng.integers(1, 3))
        left -= rows
    return orb_tape(spec, seed)


GENERATORS = {"stamps": stamps, "regular": regular, "stamps_dup_at": stamps_dup_at, "wide_stamps": wide_stamps, "returns": returns,
              "run_pattern": run_pattern, "edited": edited, "orb_tape": orb_tape, "orb_walk": orb_walk}


def generate(source):
    name, args = source
    return tuple(GENERATORS[name](*args))


# ---------------------------------------------------------------------------------------------------------------- the cases
def lengths(geo):
    t = geo["scan_tile"]
    return (1, 2, 3, 4, 5, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1)


def second_trip_length(geo):
    """One length that needs a second trip of the scans' aggregate pass."""
    return geo["scan_tile"] * geo["scan_trip_tiles"] + 3


def cases(geo):
    """name -> dict(fn, source, args, reference): the cases of tests/golden/clock.npz.  `geo`: the kernels' tile sizes
    (clock.geometry()); reference False: the untouched reference cannot run the case (DirRunLen's int8 store overflows under the
    interpreter from a run of 128 on, and it reads x[1] of a single element), the restatement alone pins it."""
    t, rt, cap = geo["scan_tile"], geo["rate_tile"], geo["rate_stage"]
    out = {}

    def add(name, fn, source, args=(), reference=True):
        out[name] = dict(fn=fn, source=source, args=list(args), reference=reference)

    for k, n in enumerate(lengths(geo)):
        add(f"dur.n{n}", "dur", ["stamps", [n, 2100 + k]], [1])
        add(f"rate.n{n}", "rate", ["stamps", [n, 2300 + k]], [5.0])
        add(f"run.n{n}", "run", ["returns", [n, 2400 + k]], reference=n > 1)        # one element: the reference reads x[1]
        add(f"orb.n{n}", "orb", ["orb_walk", [n, 2500 + k]])
        if n in (1, 2, 3, 5, 64, 65, t - 1, t + 1, 2 * t + 1):
            add(f"dew.n{n}", "dew", ["stamps", [n, 2200 + k]], [20])
    # bar_duration: periods, and a difference above 2^53 ns
    for p in (3, 0, -2, 300, 301):
        add(f"dur.p{p}", "dur", ["stamps", [300, 2120]], [p])
    add("dur.wide", "dur", ["wide_stamps", []], [1])
    add("dur.wide_p2", "dur", ["wide_stamps", []], [2])
    # bar_duration_ewma: spans, zero durations
    for span in (1, 2, 20, 2000):
        add(f"dew.span{span}", "dew", ["stamps", [300, 2220]], [span])
    add("dew.zeros", "dew", ["stamps", [300, 2221, 0.7]], [20])
    add("dew.wide", "dew", ["wide_stamps", []], [3])
    # bar_rate: the windows
    n_rate = 4 * rt + 17
    add("rate.below_every_gap", "rate", ["stamps", [n_rate, 2320, 0.0]], [1e-6])
    add("rate.whole_tape", "rate", ["stamps", [n_rate, 2321]], [1e7])
    add("rate.stage_fits", "rate", ["regular", [n_rate, SECOND]], [float(cap - rt)])              # the closed left edge, exactly
    add("rate.stage_exceeded", "rate", ["regular", [n_rate, SECOND]], [float(cap - rt + 1)])
    add("rate.dups_over_tile_edge", "rate", ["stamps_dup_at", [2 * rt + 9, 2322, rt - 3, 7]], [3.0])
    add("rate.dups_over_tile_edge_tiny", "rate", ["stamps_dup_at", [2 * rt + 9, 2322, rt - 3, 7]], [1e-6])
    for k, w in enumerate((1e-6, 1e-3, 0.25, 60.0, 360.0, 1800.0)):
        add(f"rate.w{w}", "rate", ["stamps", [1500, 2330 + k]], [w])
    # dir_run_len
    add("run.nan_at_1", "run", ["edited", [["returns", [200, 2420]], [[0, 1, "nan"]]]])
    seg = [100] * ((t - 2) // 100) + ([(t - 2) % 100] if (t - 2) % 100 else [])                       # rows 1 .. t - 2 after the lead
    add("run.heads_at_tile_edges", "run", ["run_pattern", [seg + [1, 1] + seg + [1, 1, 50]]])         # heads at t - 1, t, 2t - 1, 2t
    add("run.no_change_100", "run", ["run_pattern", [[100]]])
    add("run.r127", "run", ["run_pattern", [[5, 127, 3]]])
    for r in (128, 255, 256, 257):
        add(f"run.r{r}", "run", ["run_pattern", [[5, r, 3]]], reference=False)
    add("run.no_change", "run", ["run_pattern", [[700], -1.0, 0]], reference=False)
    add("run.alive_over_a_tile", "run", ["run_pattern", [[90, 2 * t + 50, 7], 1.0, 10]], reference=False)
    # orb_break
    q = 15 * MINUTE
    add("orb.day_starts", "orb", ["orb_tape", [[[19_900, 12 * 3_600 * SECOND, 8, q], [19_901, 0, 7, q], [19_902, MINUTE - 1, 7, q],
                                                [19_903, MINUTE, 7, q], [19_904, 0, 3, q], [19_905, 0, 4, q], [19_906, 0, 5, q],
                                                [19_908, 0, 9, q]], 2520]])                             # 19 907: an empty day
    add("orb.before_1970", "orb", ["orb_tape", [[[-3, 0, 9, q], [-2, 30 * SECOND, 9, q], [-1, MINUTE, 9, q], [0, 0, 9, q]], 2521]])
    add("orb.long_day", "orb", ["orb_tape", [[[19_910, 0, t - 2, 30 * SECOND], [19_911, 0, 2 * t + 100, 15 * SECOND]], 2522]])
    base = ["orb_tape", [[[19_920, 0, 12, q], [19_921, 0, 12, q], [19_922, 0, 12, q], [19_923, 0, 12, q]], 2523]]
    hi, lo, cl = 1, 2, 3                                                                                # (ts, high, low, close)
    edits = [[hi, 1, "nan"], [lo, 2, "nan"],                                                            # one opening high, one low
             [hi, 12, "nan"], [hi, 13, "nan"], [hi, 14, "nan"], [hi, 15, "nan"],                       # all four highs of day 2
             [lo, 24, "nan"], [lo, 25, "nan"], [lo, 26, "nan"], [lo, 27, "nan"],                       # all four lows of day 3
             [cl, 30, "nan"],                                                                           # a NaN close
             [hi, 36, "110.0"], [hi, 37, "112.0"], [hi, 38, "111.0"], [hi, 39, "109.0"],
             [cl, 41, "112.0"], [cl, 42, "112.25"], [cl, 43, "111.75"]]                                # a close equal to the range's high
    add("orb.values", "orb", ["edited", [base, edits]])
    return out
