"""Plain restatement of the Chu-Stinchcombe-White CUSUM test on levels (finmlkit/feature/core/structural_break/cusum.py) in the
reference's evaluation order, in two forms: a scalar loop (`form="scalar"`) and a NumPy form vectorised over n_rel
(`form="vector"`, what large GPU cases are compared with).  Both use math.log (libm: the project's `log` contract), elementwise
IEEE operations, np.cumsum for the variance sum and np.argmax for the first maximum.  Reads nothing outside the repository.

Per output t with window start `base`: T = t - base, S = d2[base] + ... + d2[t-1] in that order, sigma = sqrt(S / (T - 1));
sigma <= 0 -> (-1e-6, -1e-6, 0.0, 0.0); for n_rel = 1 .. T-2, k = T - n_rel: dyn = y[t] - y[base + n_rel], den = sigma * sqrt(k),
skipped when den <= 1e-16, s_up = max(dyn, 0) / den, s_down = max(-dyn, 0) / den; a side takes a strictly greater value only,
and with it the critical value sqrt(4.6 + log(k))."""
import math

import numpy as np

START = -1e-6
B_ALPHA = 4.6
DEN_MIN = 1e-16
WARMUP_MESSAGE = "warmup_period must be at least 2."
LAST_MESSAGE = "cusum_test_last needs at least 3 elements."
POSITIVE_MESSAGE = "All close prices must be positive."


def grid_walk(n, seed, step=35, hold=0.0):
    """A seeded walk on a 0.01 price grid around 100, in integer arithmetic so that every machine regenerates the same bits: each
    move is uniform in -step .. step cents, and with probability `hold` there is no move (long runs of equal prices)."""
    rng = np.random.default_rng(seed)
    moves = rng.integers(-step, step + 1, n)
    moves[rng.random(n) < hold] = 0
    cents = np.maximum(10_000 + np.cumsum(moves), 100)
    return cents / 100.0


def host_log(x):
    """log of every element as libm gives it: -inf at 0, NaN below (no exception)."""
    out = np.empty(len(x), np.float64)
    for i, v in enumerate(np.asarray(x, np.float64).tolist()):
        if v > 0.0:
            out[i] = math.log(v) if v != math.inf else math.inf
        elif v == 0.0:
            out[i] = -math.inf
        else:
            out[i] = math.nan
    return out


def prepare(x):
    """-> (y, d2): y = log(x), d2[i] = (y[i+1] - y[i])**2 with the difference rounded first."""
    y = host_log(x)
    with np.errstate(all="ignore"):
        d = y[1:] - y[:-1]
        return y, d * d


def crit(k):
    return math.sqrt(B_ALPHA + math.log(k))


def window_scalar(y, d2, base, t, stats=None):
    T = t - base
    S = 0.0
    for j in range(base, t):
        S = S + float(d2[j])
    q = S / (T - 1)
    sigma = math.sqrt(q) if q >= 0.0 else math.nan
    up = down = START
    c_up = c_down = 0.0
    if sigma <= 0.0:
        return up, down, c_up, c_down
    yt = float(y[t])
    for n_rel in range(1, T - 1):
        k = T - n_rel
        dyn = yt - float(y[base + n_rel])
        den = sigma * math.sqrt(k)
        if stats is not None:
            stats["pairs"] += 1
        if den <= DEN_MIN:
            if stats is not None:
                stats["skipped"] += 1
            continue
        s_up = _div(dyn if dyn > 0.0 else 0.0, den)
        s_down = _div(-dyn if dyn < 0.0 else 0.0, den)
        if s_up > up:
            up, c_up = s_up, crit(k)
        if s_down > down:
            down, c_down = s_down, crit(k)
    return up, down, c_up, c_down


def _div(a, b):
    """a / b as IEEE gives it (Python raises on a zero divisor; den > 1e-16 or NaN here, so only inf / inf needs care)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _first_max(s, k, ok):
    """The maximum of s over the accepted pairs and the critical value at its first position; NaN never wins."""
    s = np.where(ok & ~np.isnan(s), s, -np.inf)
    if len(s) == 0:
        return START, 0.0
    i = int(np.argmax(s))
    if not s[i] > START:
        return START, 0.0
    return float(s[i]), crit(int(k[i]))


def window_vector(y, d2, base, t, stats=None):
    T = t - base
    with np.errstate(all="ignore"):
        S = np.cumsum(d2[base:t])[-1]
        sigma = np.sqrt(S / np.float64(T - 1))
        if sigma <= 0.0:
            return START, START, 0.0, 0.0
        k = T - np.arange(1, T - 1, dtype=np.int64)
        dyn = y[t] - y[base + 1:t - 1]
        den = sigma * np.sqrt(k.astype(np.float64))
        ok = ~(den <= DEN_MIN)
        if stats is not None:
            stats["pairs"] += len(k)
            stats["skipped"] += int((~ok).sum())
        s_up = np.where(dyn > 0.0, dyn, 0.0) / den
        s_down = np.where(dyn < 0.0, -dyn, 0.0) / den
    up, c_up = _first_max(s_up, k, ok)
    down, c_down = _first_max(s_down, k, ok)
    return up, down, c_up, c_down


def _full_windows(y, d2, window, t_lo, t_hi, out, stats):
    """Outputs t_lo <= t < t_hi, all with base = t - window > 0: the same operations as window_vector on a (t, n_rel) matrix."""
    from numpy.lib.stride_tricks import sliding_window_view
    T = window
    k = T - np.arange(1, T - 1, dtype=np.int64)
    sqk = np.sqrt(k.astype(np.float64))
    D = sliding_window_view(d2, T)                   # row b: d2[b .. b+T-1]
    Y = sliding_window_view(y, T - 2)                # row b: y[b .. b+T-3]
    step = max(1, (1 << 21) // T)
    for a in range(t_lo, t_hi, step):
        b = min(a + step, t_hi)
        base = np.arange(a, b) - window
        with np.errstate(all="ignore"):
            S = np.cumsum(D[base], axis=1)[:, -1]
            sigma = np.sqrt(S / np.float64(T - 1))
            go = ~(sigma <= 0.0)
            dyn = y[a:b, None] - Y[base + 1]
            den = sigma[:, None] * sqk[None, :]
            ok = ~(den <= DEN_MIN) & go[:, None]
            s_up = np.where(dyn > 0.0, dyn, 0.0) / den
            s_down = np.where(dyn < 0.0, -dyn, 0.0) / den
        if stats is not None:
            stats["pairs"] += int(go.sum()) * len(k)
            stats["skipped"] += int(((den <= DEN_MIN) & go[:, None]).sum())
        for s, o, c in ((s_up, out[0], out[2]), (s_down, out[1], out[3])):
            s = np.where(ok & ~np.isnan(s), s, -np.inf)
            i = np.argmax(s, axis=1)
            v = s[np.arange(b - a), i]
            win = v > START
            o[a:b] = np.where(win, v, START)
            c[a:b] = [crit(int(k[j])) if w else 0.0 for j, w in zip(i, win)]


WINDOW = {"scalar": window_scalar, "vector": window_vector}


def _run(x, base_of, first, form, stats):
    x = np.asarray(x, np.float64)
    n = len(x)
    out = [np.full(n, np.nan) for _ in range(4)]
    if n == 0:
        return tuple(out)
    y, d2 = prepare(x)
    t = first
    while t < n:
        base = base_of(t)
        if form == "vector" and base > 0 and t - base >= 3:
            _full_windows(y, d2, t - base, t, n, out, stats)      # every later window is as long
            break
        r = WINDOW[form](y, d2, base, t, stats)
        for o, v in zip(out, r):
            o[t] = v
        t += 1
    return tuple(out)


def cusum_test_developing(y, warmup_period=30, form="vector", stats=None):
    if warmup_period < 2:
        raise ValueError(WARMUP_MESSAGE)
    return _run(y, lambda t: 0, warmup_period, form, stats)


def cusum_test_last(y, form="vector"):
    if len(y) < 3:
        raise ValueError(LAST_MESSAGE)
    yy, d2 = prepare(np.asarray(y, np.float64))
    return tuple(float(v) for v in WINDOW[form](yy, d2, 0, len(yy) - 1))


def cusum_test_rolling(close_prices, window_size=1000, warmup_period=30, form="vector", stats=None):
    """`stats`: a dict with "pairs" and "skipped" that is added to (the pairs walked, and those the den <= 1e-16 test dropped)."""
    x = np.asarray(close_prices, np.float64)
    if warmup_period < 2:
        raise ValueError(WARMUP_MESSAGE)
    if np.any(x <= 0):
        raise ValueError(POSITIVE_MESSAGE)
    window_size = max(window_size, warmup_period + 2)
    if len(x) < warmup_period + 2:
        return tuple(np.full(len(x), np.nan) for _ in range(4))
    return _run(x, lambda t: max(0, t - window_size), warmup_period, form, stats)


def cusum_transform(up, down, crit_up, crit_down, max_age=144):
    """The six outputs of the CUSUMTest transform from the four arrays (transforms.py:675-698): scores (statistic minus critical
    value, clipped to +-10), flags (score > 0), ages (elements since the last flag, or since the start; clipped to max_age, uint8)."""
    with np.errstate(invalid="ignore"):
        brk = [np.asarray(up) - np.asarray(crit_up), np.asarray(down) - np.asarray(crit_down)]
        flags = [b > 0 for b in brk]
        scores = [np.clip(b, -10, 10) for b in brk]
    ages = []
    for f in flags:
        age, run = np.empty(len(f), np.int64), -1                   # the count starts at 0 on the first element, flagged or not
        for i, v in enumerate(f.tolist()):
            run = 0 if v else run + 1
            age[i] = run
        ages.append(np.clip(age, 0, max_age).astype(np.uint8))
    return scores[0], scores[1], flags[0], flags[1], ages[0], ages[1]
