"""Plain restatement of the reference's windowed order statistics -- comp_burst_ratio and pct_change (feature/core/utils.py), roc
and stoch_k (feature/core/momentum.py) -- in two forms that must agree bit for bit: a scalar loop over `sorted(window)`
(`form="scalar"`) and a NumPy form over sliding windows (`form="vector"`: np.sort / np.min / np.max along the window axis, in chunks
of rows so that large cases fit in memory; what large GPU cases are compared with).  A median, a minimum and a maximum are
selections: there is no evaluation order to restate, only the rules around them.

  burst ratio  NaN before window - 1; a window with a NaN gives NaN (np.median); med = the middle element of the sorted window, or
               (a + b) / 2.0 over the two middle ones; series[i] / med when med > 0, NaN otherwise
  %K           NaN before length - 1; lo = min(low window), hi = max(high window); (100.0 * (close[t] - lo)) / (hi - lo) when
               hi > lo, NaN otherwise.  A NaN in either window gives NaN: the project's rule, the reference is path-dependent there
  roc          NaN before period; ((p[i] - p[i - period]) / p[i - period]) * 100.0, IEEE on a zero divisor
  pct_change   NaN before periods; base = x[t - periods]; (x[t] - base) / base when base > 0, NaN otherwise
Reads nothing outside the repository."""
import hashlib
import math
import sys

import numpy as np

from tests._break_ref import grid_walk  # noqa: F401 -- part of this module's interface

WINDOW_MESSAGE = "window must be at least 1."
LENGTH_MESSAGE = "stoch_k: length must be at least 1."
SHAPE_MESSAGE = "stoch_k: close, low and high must have the same length."
PERIOD_MESSAGE = "roc: period must not be negative."
PERIODS_MESSAGE = "pct_change: periods must not be negative."
NAN = math.nan
CHUNK = 1 << 22                       # window elements per chunk of the vector form

LEVELS = (0.001, 0.002, 0.01, 0.05, 0.1, 0.25, 1.0, 5.0)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def tie_sizes(n, seed):
    """A trade-size series drawn from 8 levels: most windows have duplicates straddling the median rank."""
    return np.array(LEVELS)[np.random.default_rng(seed).integers(0, len(LEVELS), n)]


def distinct_sizes(n, seed):
    """n different values (a permutation of the eighths 0.125, 0.25, ...): no ties anywhere."""
    return (np.random.default_rng(seed).permutation(n) + 1) / 8.0


SUBNORMAL = 5e-324                    # the smallest positive float64
HOSTILE = (0.0, -0.0, SUBNORMAL, -2.5e-310, math.inf, -math.inf, sys.float_info.max)


def _magnitudes(rng, n):
    """exp(normal(0, 3)): all-distinct full-mantissa values over some twenty binades."""
    return np.exp(rng.normal(0.0, 3.0, n))


def signed_sizes(n, seed, share=0.01):
    """All-distinct full-mantissa magnitudes, about 45 % of them negated, then `share` of the elements each overwritten with 0.0,
    -0.0, the smallest subnormal, a negative subnormal, +inf, -inf and DBL_MAX.  No NaN."""
    rng = np.random.default_rng(seed)
    x = _magnitudes(rng, n)
    x[rng.random(n) < 0.45] *= -1.0
    cls = rng.random(n)
    for k, v in enumerate(HOSTILE):
        x[(cls >= k * share) & (cls < (k + 1) * share)] = v
    return x


def alternating_sizes(n, seed):
    """The same magnitudes, negative at even indices and positive at odd ones: the median of an odd window alternates between the
    largest negative and the smallest positive element, that of an even window is their mean."""
    x = _magnitudes(np.random.default_rng(seed), n)
    x[0::2] *= -1.0
    return x


def signed_ohlc_walk(n, seed, hostile=False):
    """-> (close, low, high) around zero: a cumulative sum of normals that crosses it, `low` / `high` at random distances, -inf
    planted once in `low` (index 40) and +inf once in `high` (index n - 41; both only where n >= 100).  hostile: `low` and `high`
    are signed_sizes series instead, sorted into order element by element, and `close` lies between them or on one of them."""
    rng = np.random.default_rng(seed)
    if hostile:
        a, b = signed_sizes(n, seed + 1, 0.02), signed_sizes(n, seed + 2, 0.02)
        low, high = np.minimum(a, b), np.maximum(a, b)
        pick = rng.integers(0, 3, n)
        with np.errstate(all="ignore"):
            mid = low / 2.0 + high / 2.0
        close = np.where(pick == 0, low, np.where(pick == 1, high, np.where(np.isnan(mid), 0.0, mid)))
        return close, low, high
    close = np.cumsum(rng.normal(0.0, 1.0, n))
    close -= close[n // 2]                                       # zero in the middle: both signs occur
    low, high = close - rng.exponential(0.5, n), close + rng.exponential(0.5, n)
    if n >= 100:
        low[40], high[n - 41] = -math.inf, math.inf
    return close, low, high


def nan_canonical(a):
    """a with every NaN replaced by the canonical quiet NaN (what the hashes of large outputs are taken over)."""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a


def ohlc_walk(n, seed, step=35, spread=30, hold=0.0):
    """-> (close, low, high) on a 0.01 grid in integer arithmetic: a walk and non-negative distances below and above it.  With
    probability `hold` a bar repeats the close and has low == high == close."""
    rng = np.random.default_rng(seed)
    moves = rng.integers(-step, step + 1, n)
    below, above = rng.integers(0, spread + 1, n), rng.integers(0, spread + 1, n)
    held = rng.random(n) < hold
    moves[held] = 0
    below[held] = 0
    above[held] = 0
    cents = np.maximum(10_000 + np.cumsum(moves), 100)
    return cents / 100.0, (cents - below) / 100.0, (cents + above) / 100.0


def _div(a, b):
    """a / b as IEEE gives it (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _rows(x, window):
    """The windows of x as chunks of rows: (first output index, 2-D view of shape (rows, window))."""
    view = np.lib.stride_tricks.sliding_window_view(x, window)
    per = max(1, CHUNK // window)
    for a in range(0, len(view), per):
        yield window - 1 + a, view[a:a + per]


# ---------------------------------------------------------------------------------------------------------------- burst ratio
def comp_burst_ratio(series, window, form="vector"):
    if int(window) < 1:
        raise ValueError(WINDOW_MESSAGE)
    x = np.asarray(series, np.float64)
    n = len(x)
    out = np.full(n, np.nan)
    if window > n:
        return out
    half = window // 2
    if form == "scalar":
        xs = x.tolist()
        for i in range(window - 1, n):
            w = xs[i - window + 1:i + 1]
            if any(v != v for v in w):
                continue
            s = sorted(w)
            med = s[half] if window % 2 else _div(s[half - 1] + s[half], 2.0)
            if med > 0:
                out[i] = _div(xs[i], med)
        return out
    with np.errstate(all="ignore"):
        for first, rows in _rows(x, window):
            s = np.sort(rows, axis=1)                            # NaN last
            med = s[:, half] if window % 2 else (s[:, half - 1] + s[:, half]) / 2.0
            ok = ~np.isnan(s[:, -1]) & (med > 0)
            cur = x[first:first + len(rows)]
            out[first:first + len(rows)] = np.where(ok, cur / np.where(ok, med, 1.0), np.nan)
    return out


# ---------------------------------------------------------------------------------------------------------------- %K
def stoch_k(close, low, high, length, form="vector"):
    if int(length) < 1:
        raise ValueError(LENGTH_MESSAGE)
    c, lo_a, hi_a = (np.asarray(a, np.float64) for a in (close, low, high))
    if not len(c) == len(lo_a) == len(hi_a):
        raise ValueError(SHAPE_MESSAGE)
    n = len(c)
    out = np.full(n, np.nan)
    if length > n:
        return out
    if form == "scalar":
        cs, ls, hs = c.tolist(), lo_a.tolist(), hi_a.tolist()
        for t in range(length - 1, n):
            wl, wh = ls[t - length + 1:t + 1], hs[t - length + 1:t + 1]
            if any(v != v for v in wl) or any(v != v for v in wh):
                continue
            lo, hi = sorted(wl)[0], sorted(wh)[-1]
            if hi > lo:
                with np.errstate(all="ignore"):
                    out[t] = float((np.float64(100.0) * (np.float64(cs[t]) - np.float64(lo))) / (np.float64(hi) - np.float64(lo)))
        return out
    with np.errstate(all="ignore"):
        for (first, rl), (_, rh) in zip(_rows(lo_a, length), _rows(hi_a, length)):
            bad = np.isnan(rl).any(axis=1) | np.isnan(rh).any(axis=1)
            lo, hi = np.min(rl, axis=1), np.max(rh, axis=1)
            ok = ~bad & (hi > lo)
            cur = c[first:first + len(rl)]
            out[first:first + len(rl)] = np.where(ok, (100.0 * (cur - lo)) / np.where(ok, hi - lo, 1.0), np.nan)
    return out


# ---------------------------------------------------------------------------------------------------------------- roc, pct_change
def roc(price, period, form="vector"):
    if int(period) < 0:
        raise ValueError(PERIOD_MESSAGE)
    p = np.asarray(price, np.float64)
    n = len(p)
    out = np.full(n, np.nan)
    if period >= n:
        return out
    if form == "scalar":
        ps = p.tolist()
        for i in range(period, n):
            out[i] = _div(ps[i] - ps[i - period], ps[i - period]) * 100.0
        return out
    with np.errstate(all="ignore"):
        base = p[:n - period]
        out[period:] = ((p[period:] - base) / base) * 100.0
    return out


def pct_change(x, periods, form="vector"):
    if int(periods) < 0:
        raise ValueError(PERIODS_MESSAGE)
    v = np.asarray(x, np.float64)
    n = len(v)
    out = np.full(n, np.nan)
    if periods >= n:
        return out
    if form == "scalar":
        vs = v.tolist()
        for t in range(periods, n):
            base = vs[t - periods]
            if base > 0:
                out[t] = _div(vs[t] - base, base)
        return out
    with np.errstate(all="ignore"):
        base = v[:n - periods]
        ok = base > 0
        out[periods:] = np.where(ok, (v[periods:] - base) / np.where(ok, base, 1.0), np.nan)
    return out


def call(fn, inputs, arg, form="vector", mod=None):
    """One fixture case on this module (or on `mod`, which has the reference's names and takes no `form`).  `inputs`: the series, or
    (close, low, high) for "stoch"."""
    kw = {} if mod is not None else {"form": form}
    mod = mod or sys.modules[__name__]
    if fn == "burst":
        return mod.comp_burst_ratio(inputs, arg, **kw)
    if fn == "stoch":
        return mod.stoch_k(inputs[0], inputs[1], inputs[2], arg, **kw)
    if fn == "roc":
        return mod.roc(inputs, arg, **kw)
    return mod.pct_change(inputs, arg, **kw)
