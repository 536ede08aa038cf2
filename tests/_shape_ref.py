"""Plain restatement of the four window statistics of the reference's transforms.py -- KurtosisTransform (:900-933), TrendSlope
(:936-988), HurstExponent (:1341-1397), BiPowerVariation (:1551-1602) -- as functions (x, window) -> float64 array, in two forms: a
sequential one (`form="scalar"`: one window after the other, Python floats) and a NumPy form in the kernel's order
(`form="vector"`: vectorised over the outputs, looped over the position in the window; what large GPU cases are compared with).
Reads nothing outside the repository.

With w the window; a window that reads a NaN or an infinity gives NaN:
    kurtosis  t >= w-1 over x[t-w+1 .. t]: m = mean, m2 = mean((x-m)^2), m4 = mean(((x-m)^2)^2), m4 / (m2 * m2) - 3 (0 / 0 -> NaN)
    slope     t >= w-1 over y = ln x (x finite and > 0): atan(sum((p - (w-1)/2) * (y_p - mean y)) / (w (w^2-1) / 12)) * 180 / pi
    hurst     t >= w-1, w >= 9: tau_k = sqrt(population variance of the w-k sums of k consecutive elements of x[t-w+2 .. t]),
              k = 1, 2, 4, 8; all > 0: (-1.5 ln tau_1 - 0.5 ln tau_2 + 0.5 ln tau_4 + 1.5 ln tau_8) / (5 ln 2), else NaN
    bipower   t >= w over x[t-w .. t]: sqrt(pi / 2) * sum(|x[j]| * |x[j-1]|, j = t-w+1 .. t)
A window without a statistic gives NaN: kurtosis where the w elements all compare equal (==, so +0 and -0 are equal), hurst where for
some k the w - k sums of k elements, as they are held in float64, all compare equal.  The elements and sums themselves are compared,
not their deviations from a rounded mean, which would leave m2 = delta^2 or tau_k = delta on a held 99.55.
The sums of k elements are formed as a tree ((a + b) + (c + d)) + ..., oldest first inside a pair, the way the kernel's loader forms
them; the logarithm of a price is libm's (math.log), which the kernel restates."""
import hashlib
import math

import numpy as np

from tests._break_ref import grid_walk  # noqa: F401 -- part of this module's interface

WINDOW_MESSAGE = "window must be at least 1."
HURST_WINDOW_MESSAGE = "hurst_exponent: window must be at least 9."
HURST_MIN_WINDOW = 9
LAGS = (1, 2, 4, 8)
NAN = math.nan
BV_SCALE = math.sqrt(math.pi / 2.0)
DEGREES = 180.0 / math.pi
FUNCTIONS = ("kurtosis", "slope", "hurst", "bipower")
PRODUCT_NAMES = {"kurtosis": "rolling_kurtosis", "slope": "trend_slope", "hurst": "hurst_exponent", "bipower": "bipower_variation"}
RELATIVE = {"kurtosis": False, "slope": False, "hurst": False, "bipower": True}     # how a statistic is compared


def dyadic_returns(n, seed, jump=0.01):
    """n seeded returns on a 2^-20 grid within +-2^-10, a fraction `jump` of them 30 times larger (integer arithmetic: every machine
    regenerates the same bits, and every sum of a window is exact)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-(1 << 10), (1 << 10) + 1, n)
    k[rng.random(n) < jump] *= 30
    return k / float(1 << 20)


def mantissa_returns(n, seed):
    """n seeded returns of either sign within +-2^-9 that use all 53 bits of the mantissa (integer arithmetic, exact conversion):
    no sum or product of a window is exact."""
    rng = np.random.default_rng(seed)
    k = rng.integers(1 << 52, 1 << 53, n).astype(np.float64) * 2.0 ** -62
    return np.where(rng.integers(0, 2, n) == 1, k, -k)


def grid_normal(n, seed, base, denom):
    """base + k / denom with k a seeded bell-shaped integer of standard deviation 101 (the sum of four uniform draws: integer
    arithmetic and one correctly rounded division, so every machine regenerates the same bits): prices like 100 + round(z, 2)."""
    k = np.random.default_rng(seed).integers(-87, 88, (n, 4)).sum(axis=1)
    return base + k / float(denom)


def held_series(n, seed, base, denom, runs=()):
    """grid_normal values, each held for a seeded run of 1 .. 140 elements, cut to n; then every (start, length) of `runs` holds
    x[start] for `length` elements (a run laid where the walk changes hands)."""
    lens = np.random.default_rng(seed + 1).integers(1, 141, n)
    x = np.repeat(grid_normal(n, seed, base, denom), lens)[:n].copy()
    for start, length in runs:
        x[start:start + length] = x[start]
    return x


def levels(n, seed, base, denom, count):
    """base + k / denom, k seeded and uniform on 0 .. count - 1."""
    return base + np.random.default_rng(seed).integers(0, count, n) / float(denom)


def constant(n, value):
    return np.full(n, float(value))


def one_odd(n, value, pos, odd):
    """A constant series with one other element."""
    x = np.full(n, float(value))
    x[pos] = odd
    return x


def periodic(n, values):
    return np.resize(np.asarray(values, np.float64), n)


GENERATORS = {"grid_walk": grid_walk, "dyadic_returns": dyadic_returns, "mantissa_returns": mantissa_returns,
              "grid_normal": grid_normal, "held_series": held_series, "levels": levels, "constant": constant, "one_odd": one_odd,
              "periodic": periodic}


def generate(source):
    """The input of a case's `source`: [generator, args]."""
    return GENERATORS[source[0]](*source[1])


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def first_output(fn, window):
    return window if fn == "bipower" else window - 1


def _input(fn, x, window):
    if int(window) < 1:
        raise ValueError(WINDOW_MESSAGE)
    if fn == "hurst" and int(window) < HURST_MIN_WINDOW:
        raise ValueError(HURST_WINDOW_MESSAGE)
    return np.ascontiguousarray(x, dtype=np.float64)


def _finite(x):
    return np.where(np.isfinite(x), x, np.nan)


def _log_prices(x):
    """libm's log of every finite price > 0, NaN elsewhere."""
    return np.array([math.log(v) if 0.0 < v < math.inf else NAN for v in x.tolist()], np.float64)


def _tree(e):
    """The sum of 1, 2, 4 or 8 values, oldest first, as the loader's tree."""
    if len(e) == 1:
        return e[0]
    if len(e) == 2:
        return e[0] + e[1]
    if len(e) == 4:
        return (e[0] + e[1]) + (e[2] + e[3])
    return ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]))


# ------------------------------------------------------------------------------------------------ one window after the other
def _scalar_window(fn, win, w):
    """One output from the w (bipower: w + 1) elements of its window, all finite."""
    if fn == "kurtosis":
        if all(v == win[-1] for v in win):                             # a held value has no kurtosis, whatever fl(sum / w) is
            return NAN
        s = 0.0
        for v in win:
            s = s + v
        m = s / w
        q2 = q4 = 0.0
        for v in win:
            d2 = (v - m) * (v - m)
            q2 = q2 + d2
            q4 = q4 + d2 * d2
        m2, m4 = q2 / w, q4 / w
        return m4 / (m2 * m2) - 3.0 if m2 != 0.0 else NAN
    if fn == "slope":
        if any(not v > 0.0 for v in win):
            return NAN
        y = [math.log(v) for v in win]
        s = 0.0
        for v in y:
            s = s + v
        m = s / w
        acc = 0.0
        for p, v in enumerate(y):
            acc = acc + (p - (w - 1.0) / 2.0) * (v - m)
        ssx = w * (float(w) * w - 1.0) / 12.0
        return math.atan(acc / ssx) * DEGREES if ssx != 0.0 else NAN
    if fn == "hurst":
        logs = []
        for k in LAGS:
            d = [_tree(win[j + 1:j + k + 1]) for j in range(w - k)]
            if all(v == d[-1] for v in d):                             # tau_k is 0 for the sums as they are held
                return NAN
            s = 0.0
            for v in d:
                s = s + v
            m = s / (w - k)
            q = 0.0
            for v in d:
                q = q + (v - m) * (v - m)
            tau = math.sqrt(q / (w - k))
            if not tau > 0.0:
                return NAN
            logs.append(math.log(tau))
        return (-1.5 * logs[0] - 0.5 * logs[1] + 0.5 * logs[2] + 1.5 * logs[3]) / (5.0 * math.log(2.0))
    s = 0.0
    for j in range(1, w + 1):
        s = s + abs(win[j]) * abs(win[j - 1])
    return BV_SCALE * s


def _scalar(fn, x, w):
    n = len(x)
    out = np.full(n, np.nan)
    xs = x.tolist()
    reach = w + 1 if fn == "bipower" else w
    for t in range(reach - 1, n):
        win = xs[t - reach + 1:t + 1]
        if all(math.isfinite(v) for v in win):
            out[t] = _scalar_window(fn, win, w)
    return out


# ------------------------------------------------------------------------------------------------ the kernel's order
def _vector(fn, x, w):
    n = len(x)
    out = np.full(n, np.nan)
    first = first_output(fn, w)
    m = n - first                                                  # outputs first .. n - 1
    if m <= 0:
        return out
    fw = float(w)
    with np.errstate(all="ignore"):
        if fn in ("kurtosis", "slope"):
            v = _finite(x) if fn == "kurtosis" else _log_prices(x)
            s, differs = np.zeros(m), np.zeros(m, bool)
            for p in range(w):
                s = s + v[p:p + m]
                if fn == "kurtosis":
                    differs |= v[p:p + m] != v[w - 1:w - 1 + m]         # against the window's last element; a NaN differs
            mean = s / fw
            if fn == "kurtosis":
                q2, q4 = np.zeros(m), np.zeros(m)
                for p in range(w):
                    d = v[p:p + m] - mean
                    d2 = d * d
                    q2 = q2 + d2
                    q4 = q4 + d2 * d2
                m2, m4 = q2 / fw, q4 / fw
                out[first:] = np.where(differs, m4 / (m2 * m2) - 3.0, np.nan)
            else:
                acc, centre = np.zeros(m), (fw - 1.0) / 2.0
                for p in range(w):
                    acc = acc + (float(p) - centre) * (v[p:p + m] - mean)
                out[first:] = np.arctan(acc / (fw * (fw * fw - 1.0) / 12.0)) * DEGREES
        elif fn == "bipower":
            f = np.abs(_finite(x))
            prod = np.full(n, np.nan)
            prod[1:] = f[1:] * f[:-1]
            s = np.zeros(m)
            for p in range(w):
                s = s + prod[p + 1:p + 1 + m]
            out[first:] = BV_SCALE * s
        else:
            f = _finite(x)
            e = [np.concatenate((np.zeros(k), f[:n - k])) for k in range(8)]      # e[k][i] = x[i - k], 0.0 below the series
            d1 = np.where(np.isnan(e[1]), np.nan, e[0])                # carries the finiteness of x[i - 1]
            d2 = e[1] + e[0]
            d4 = (e[3] + e[2]) + d2
            d8 = ((e[7] + e[6]) + (e[5] + e[4])) + d4
            words = (d1, d2, d4, d8)
            sums = [np.zeros(m) for _ in LAGS]
            varies = [np.zeros(m, bool) for _ in LAGS]                 # some D_k of the window != its last one (a NaN differs)
            for p in range(w - 1):                                     # output j walks words j + 1 .. j + w - 1
                for c, k in enumerate(LAGS):
                    if p >= k - 1:
                        sums[c] = sums[c] + words[c][p + 1:p + 1 + m]
                        varies[c] |= words[c][p + 1:p + 1 + m] != words[c][w - 1:w - 1 + m]
            means = [sums[c] / (fw - k) for c, k in enumerate(LAGS)]
            sq = [np.zeros(m) for _ in LAGS]
            for p in range(w - 1):
                for c, k in enumerate(LAGS):
                    if p >= k - 1:
                        dev = words[c][p + 1:p + 1 + m] - means[c]
                        sq[c] = sq[c] + dev * dev
            tau = [np.sqrt(sq[c] / (fw - k)) for c, k in enumerate(LAGS)]
            good = (tau[0] > 0) & (tau[1] > 0) & (tau[2] > 0) & (tau[3] > 0) & varies[0] & varies[1] & varies[2] & varies[3]
            safe = [np.where(good, t, 1.0) for t in tau]
            logs = [np.array([math.log(v) for v in t.tolist()]) for t in safe]
            h = (-1.5 * logs[0] - 0.5 * logs[1] + 0.5 * logs[2] + 1.5 * logs[3]) / (5.0 * math.log(2.0))
            out[first:] = np.where(good, h, np.nan)
    return out


def call(fn, x, window, form="vector"):
    xx = _input(fn, x, window)
    return _scalar(fn, xx, int(window)) if form == "scalar" else _vector(fn, xx, int(window))


def rolling_kurtosis(x, window, form="vector"):
    return call("kurtosis", x, window, form)


def trend_slope(x, window, form="vector"):
    return call("slope", x, window, form)


def hurst_exponent(x, window, form="vector"):
    return call("hurst", x, window, form)


def bipower_variation(x, window, form="vector"):
    return call("bipower", x, window, form)


# ------------------------------------------------------------------------------------------------ comparing
def deviation(fn, got, want):
    """The largest deviation of `got` from `want` in the statistic's measure (absolute; bipower: relative to |want|, an exact
    match counting 0), or None when the NaN positions differ."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return None
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    d = np.abs(got[ok] - want[ok])
    if RELATIVE[fn]:
        d = np.where(d == 0.0, 0.0, d / np.where(want[ok] == 0.0, 1.0, np.abs(want[ok])))
        d = np.where((want[ok] == 0.0) & (got[ok] != 0.0), np.inf, d)
    return float(d.max())


def tolerance_from(dev):
    """16 times a measured deviation, rounded up to a power of ten (0 stays 0)."""
    return 0.0 if dev == 0.0 else 10.0 ** math.ceil(math.log10(16.0 * dev))
