"""Plain restatement of the reference's rolling-window moments -- sma (feature/core/ma.py), comp_zscore (feature/core/utils.py),
rolling_variance_nb and variance_ratio_1_4_core (feature/core/volatility.py) -- in the evaluation order the reference has when
Numba compiles it: every window summed on its own, left to right, one rounded addition per element.  Two forms: a scalar loop
(`form="scalar"`) and a NumPy form vectorised over the outputs (`form="vector"`: `window` additions of whole columns, which keeps
the order per output; what large GPU cases are compared with).  The log is libm's (math.log / tests/_break_ref.host_log: the
project's `log` contract).  Reads nothing outside the repository."""
import hashlib
import math
import sys

import numpy as np

from tests._break_ref import grid_walk, host_log  # noqa: F401 -- grid_walk is part of this module's interface

WINDOW_MESSAGE = "window must be at least 1."
ZSCORE_MESSAGE = "comp_zscore: window - ddof must be positive."
NAN = math.nan


def walk_returns(n, seed, step=35, hold=0.0):
    """n log returns of a grid walk of n + 1 prices (the host's log of the rounded quotient)."""
    w = grid_walk(n + 1, seed, step, hold)
    return host_log(w[1:] / w[:-1])


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _div(a, b):
    """a / b as IEEE gives it (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else NAN


def _log1(v):
    return float(host_log(np.array([v]))[0])


def _check(window):
    if int(window) < 1:
        raise ValueError(WINDOW_MESSAGE)


def _columns(x, window):
    """The outputs' windows as `window` columns: column p holds element p of every window."""
    m = len(x) - window + 1
    return m, (x[p:p + m] for p in range(window))


# ---------------------------------------------------------------------------------------------------------------- sma
def sma(array, window, form="vector"):
    _check(window)
    x = np.asarray(array, np.float64)
    n = len(x)
    out = np.full(n, np.nan)
    if window > n:
        return out
    inv = 1.0 / window
    if form == "scalar":
        xs = x.tolist()
        for i in range(window - 1, n):
            s = 0.0
            for j in range(i - window + 1, i + 1):
                s = s + xs[j]
            out[i] = inv * s
        return out
    with np.errstate(all="ignore"):
        m, cols = _columns(x, window)
        s = np.zeros(m)
        for c in cols:
            s = s + c
        out[window - 1:] = inv * s
    return out


# ---------------------------------------------------------------------------------------------------------------- z-score
def comp_zscore(x, window, ddof, form="vector"):
    _check(window)
    if window - ddof <= 0:
        raise ValueError(ZSCORE_MESSAGE)
    x = np.asarray(x, np.float64)
    n = len(x)
    out = np.full(n, np.nan)
    if window > n:
        return out
    if form == "scalar":
        xs = x.tolist()
        for i in range(window - 1, n):
            s = 0.0
            for j in range(i - window + 1, i + 1):
                s = s + xs[j]
            mean = s / window
            acc = 0.0
            for j in range(i - window + 1, i + 1):
                d = xs[j] - mean
                acc = acc + d * d
            std = _sqrt(acc / (window - ddof))
            if std != 0:
                out[i] = _div(xs[i] - mean, std)
        return out
    with np.errstate(all="ignore"):
        m, cols = _columns(x, window)
        s = np.zeros(m)
        for c in cols:
            s = s + c
        mean = s / np.float64(window)
        acc = np.zeros(m)
        for c in _columns(x, window)[1]:
            d = c - mean
            acc = acc + d * d
        std = np.sqrt(acc / np.float64(window - ddof))
        out[window - 1:] = np.where(std != 0, (x[window - 1:] - mean) / std, np.nan)
    return out


# ---------------------------------------------------------------------------------------------------------------- variance
def rolling_variance_nb(series, window, ddof=1, min_periods=1, form="vector"):
    _check(window)
    x = np.asarray(series, np.float64)
    n = len(x)
    out = np.full(n, np.nan)
    if n < window:
        return out
    if form == "scalar":
        xs = x.tolist()
        for i in range(window - 1, n):
            cnt, s, q = 0, 0.0, 0.0
            for j in range(i - window + 1, i + 1):
                v = xs[j]
                if v == v:
                    cnt += 1
                    s = s + v
                    q = q + v * v
            if cnt >= min_periods and cnt > ddof:
                mean = _div(s, cnt)
                var = _div(q, cnt) - mean * mean
                var = var * (cnt / (cnt - ddof))
                out[i] = var if var > 0.0 else 0.0               # max(0.0, var): a NaN var gives 0.0
        return out
    with np.errstate(all="ignore"):
        m, cols = _columns(x, window)
        cnt, s, q = np.zeros(m, np.int64), np.zeros(m), np.zeros(m)
        for c in cols:
            ok = ~np.isnan(c)
            s = np.where(ok, s + c, s)
            q = np.where(ok, q + c * c, q)
            cnt += ok
        good = (cnt >= min_periods) & (cnt > ddof)
        fc = cnt.astype(np.float64)
        mean = s / fc
        var = q / fc - mean * mean
        var = var * (fc / (cnt - ddof).astype(np.float64))
        out[window - 1:] = np.where(good, np.where(var > 0.0, var, 0.0), np.nan)
    return out


# ---------------------------------------------------------------------------------------------------------------- variance ratio
def returns_1(price, is_log, form="vector"):
    p = np.asarray(price, np.float64)
    n = len(p)
    r1 = np.full(n, np.nan)
    if form == "scalar":
        ps = p.tolist()
        for i in range(1, n):
            c, b = ps[i], ps[i - 1]
            if c != c or b != b or b <= 0 or (is_log and c <= 0):
                continue
            r1[i] = _log1(c / b) if is_log else c / b - 1.0
        return r1
    if n < 2:
        return r1
    with np.errstate(all="ignore"):
        c, b = p[1:], p[:-1]
        ok = ~np.isnan(c) & ~np.isnan(b) & ~(b <= 0)
        if is_log:
            ok &= ~(c <= 0)
        ratio = np.where(ok, c, 1.0) / np.where(ok, b, 1.0)
        r1[1:] = np.where(ok, host_log(ratio) if is_log else ratio - 1.0, np.nan)
    return r1


def returns_4(r1, form="vector"):
    n = len(r1)
    r4 = np.full(n, np.nan)
    if form == "scalar":
        rs = r1.tolist()
        for i in range(4, n):
            if rs[i] == rs[i] and rs[i - 1] == rs[i - 1] and rs[i - 2] == rs[i - 2] and rs[i - 3] == rs[i - 3]:
                r4[i] = ((rs[i] + rs[i - 1]) + rs[i - 2]) + rs[i - 3]
        return r4
    if n > 4:
        with np.errstate(all="ignore"):
            r4[4:] = ((r1[4:] + r1[3:-1]) + r1[2:-2]) + r1[1:-3]     # NaN when one of the four is
    return r4


def variance_ratio_1_4_core(price, window, ddof, ret_type, form="vector"):
    _check(window)
    p = np.asarray(price, np.float64)
    n = len(p)
    out = np.full(n, np.nan)
    if n < window + 4:
        return out
    r1 = returns_1(p, ret_type == "log", form)
    v1 = rolling_variance_nb(r1, window, ddof, 1, form)
    v4 = rolling_variance_nb(returns_4(r1, form), window, ddof, 1, form)
    with np.errstate(all="ignore"):
        ok = ~np.isnan(v1) & ~np.isnan(v4) & (v4 > 0)
        out[ok] = v1[ok] / (v4[ok] / 4)
    return out


FUNCTIONS = {"sma": sma, "zscore": comp_zscore, "variance": rolling_variance_nb, "ratio": variance_ratio_1_4_core}


def call(fn, x, window, ddof=None, min_periods=None, ret_type=None, form="vector", mod=None):
    """One fixture case on this module (or on `mod`, which has the reference's names and takes no `form`)."""
    kw = {} if mod is not None else {"form": form}
    mod = mod or sys.modules[__name__]
    if fn == "sma":
        return mod.sma(x, window, **kw)
    if fn == "zscore":
        return mod.comp_zscore(x, window, ddof, **kw)
    if fn == "variance":
        return mod.rolling_variance_nb(x, window, ddof, min_periods, **kw)
    return mod.variance_ratio_1_4_core(x, window, ddof, ret_type, **kw)
