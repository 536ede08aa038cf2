"""Plain restatement of the rolling approximate entropy -- the reference's ApproximateEntropy (transforms.py:1400-1457), which is
pandas' rolling.apply around antropy.app_entropy(x, order=m, metric="chebyshev", tolerance=tolerance * np.std(x)) -- as a function
(x, window, m, tolerance) -> float64 array, in two forms.  Reads nothing outside the repository and needs no `antropy`: it restates
that function's published algorithm.

For the window x_0 .. x_{w-1} = x[t-w+1 .. t], t >= w - 1; a window that reads a NaN or an infinity gives NaN:
    r = tolerance * std(window) (population); for k in (m, m + 1): N_k = w - k + 1 vectors (x_i .. x_{i+k-1}),
    C_k[i] = #{j : max_q |x_{i+q} - x_{j+q}| <= r} (inclusive, j = i counts), phi_k = mean_i ln(C_k[i] / N_k); out = phi_m - phi_{m+1}
`form="scalar"`: one window after the other in the reference's arithmetic -- np.std, brute-force distances between the embedded
vectors, np.mean(np.log(C / N)).  `form="vector"`: the kernel's order (csrc/fmk_entropy.hip), vectorised over the outputs -- the sum
and the sum of squared deviations oldest first, r = tolerance * sqrt(that / w), the counts from the element-pair comparisons,
phi_k = (sum_i (ln C_k[i] - ln N_k)) / N_k with i ascending and ln k from a table of libm's log (math.log), ln 0 = NaN.

`knife_edge` marks the windows in which some pair of elements lies within 2^-40 * r of r: there a few-ulp difference in r between
two summation orders would flip an integer count and move the output discontinuously, which no tolerance covers (2^-40 is about
8000 ulp of r; the orders differ by a few ulp)."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests._shape_ref import dyadic_returns, generate, mantissa_returns, sha256, tolerance_from  # noqa: F401 -- part of the interface

MAX_M = 4
MAX_WINDOW = 1024
M_MESSAGE = "approximate_entropy: m must be at least 1."
MAX_M_MESSAGE = "approximate_entropy: m must be at most 4."
WINDOW_MESSAGE = "approximate_entropy: window must be at least m + 1."
MAX_WINDOW_MESSAGE = "approximate_entropy: window must be at most 1024."
TOLERANCE_MESSAGE = "approximate_entropy: tolerance must be finite and not negative."
MESSAGES = (M_MESSAGE, MAX_M_MESSAGE, WINDOW_MESSAGE, MAX_WINDOW_MESSAGE, TOLERANCE_MESSAGE)
KNIFE = 2.0 ** -40
_BLOCK_CELLS = 1 << 22               # outputs x window x window cells handled at once


def check_arguments(window, m, tolerance):
    if int(m) < 1:
        raise ValueError(M_MESSAGE)
    if int(m) > MAX_M:
        raise ValueError(MAX_M_MESSAGE)
    if int(window) < int(m) + 1:
        raise ValueError(WINDOW_MESSAGE)
    if int(window) > MAX_WINDOW:
        raise ValueError(MAX_WINDOW_MESSAGE)
    if not (float(tolerance) >= 0.0 and float(tolerance) < math.inf):
        raise ValueError(TOLERANCE_MESSAGE)


def _finite(x):
    return np.where(np.isfinite(x), x, np.nan)


# ------------------------------------------------------------------------------------------------ one window after the other
def window_counts(win, m, r):
    """(C_m, C_{m+1}) of one window by brute force: the Chebyshev distance between every two embedded vectors against r."""
    win = np.asarray(win, np.float64)
    apart = np.abs(win[:, None] - win[None, :])                     # |x_i - x_j|
    out = []
    for k in (m, m + 1):
        nk = len(win) - k + 1
        dist = apart[:nk, :nk]
        for q in range(1, k):
            dist = np.maximum(dist, apart[q:q + nk, q:q + nk])
        out.append((dist <= r).sum(axis=1))
    return out[0], out[1]


def scalar_window(win, m, tolerance):
    """One output from the finite elements of its window, in the reference's arithmetic."""
    r = tolerance * np.std(win)
    cm, cm1 = window_counts(win, m, r)
    return float(np.mean(np.log(cm / len(cm))) - np.mean(np.log(cm1 / len(cm1))))


def _scalar(x, w, m, tolerance):
    n = len(x)
    out = np.full(n, np.nan)
    for t in range(w - 1, n):
        win = x[t - w + 1:t + 1]
        if np.isfinite(win).all():
            out[t] = scalar_window(win, m, tolerance)
    return out


# ------------------------------------------------------------------------------------------------ the kernel's order
def _windows(x, w):
    """(the windows of the outputs w - 1 .. n - 1 as rows, non-finite elements NaN; r of every window in the kernel's order)."""
    win = sliding_window_view(_finite(x), w)
    fw = float(w)
    with np.errstate(all="ignore"):
        s = np.zeros(len(win))
        for p in range(w):
            s = s + win[:, p]
        mean = s / fw
        q = np.zeros(len(win))
        for p in range(w):
            d = win[:, p] - mean
            q = q + d * d
    return win, q / fw


def _blocks(count, w):
    step = max(1, _BLOCK_CELLS // (w * w))
    return [(a, min(count, a + step)) for a in range(0, count, step)]


def _vector(x, w, m, tolerance):
    n = len(x)
    out = np.full(n, np.nan)
    if n < w:
        return out
    win, var = _windows(x, w)
    with np.errstate(all="ignore"):
        r = tolerance * np.sqrt(var)
    nm, nm1 = w - m + 1, w - m
    table = np.array([math.nan] + [math.log(k) for k in range(1, w + 1)])
    res = np.empty(len(win))
    for a, b in _blocks(len(win), w):
        v = win[a:b]
        with np.errstate(all="ignore"):
            near = np.abs(v[:, :, None] - v[:, None, :]) <= r[a:b, None, None]      # near[o, i, j]: |x_i - x_j| <= r
        both = near[:, :nm, :nm].copy()
        for q in range(1, m):
            both &= near[:, q:q + nm, q:q + nm]
        cm = both.sum(axis=2)
        cm1 = (both[:, :nm1, :nm1] & near[:, m:m + nm1, m:m + nm1]).sum(axis=2)
        sm, sm1 = np.zeros(b - a), np.zeros(b - a)
        for i in range(nm):
            sm = sm + (table[cm[:, i]] - table[nm])
        for i in range(nm1):
            sm1 = sm1 + (table[cm1[:, i]] - table[nm1])
        res[a:b] = sm / float(nm) - sm1 / float(nm1)
    out[w - 1:] = res
    return out


def approximate_entropy(x, window, m=2, tolerance=0.2, form="vector"):
    check_arguments(window, m, tolerance)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    if form == "scalar":
        return _scalar(xx, int(window), int(m), float(tolerance))
    return _vector(xx, int(window), int(m), float(tolerance))


def knife_edge(x, window, m=2, tolerance=0.2):
    """The mask, over the outputs, of the windows in which some pair of elements has | |x_a - x_b| - r | <= 2^-40 * r, r > 0 in the
    kernel's order.  r = 0 (tolerance 0, a constant window of dyadic values) is 0 in every order and no edge."""
    check_arguments(window, m, tolerance)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    w, n = int(window), len(xx)
    mask = np.zeros(n, bool)
    if n < w:
        return mask
    win, var = _windows(xx, w)
    with np.errstate(all="ignore"):
        r = float(tolerance) * np.sqrt(var)
        for a, b in _blocks(len(win), w):
            v, rr = win[a:b], r[a:b, None, None]
            d = np.abs(v[:, :, None] - v[:, None, :])
            mask[w - 1 + a:w - 1 + b] = ((np.abs(d - rr) <= KNIFE * rr) & (rr > 0.0)).any(axis=(1, 2))
    return mask


def margin(x, window, m=2, tolerance=0.2):
    """The smallest | |x_a - x_b| - r | / r over all windows with r > 0 and finite (inf when there is none): how far the series
    stays from a knife edge."""
    xx = np.ascontiguousarray(x, dtype=np.float64)
    w = int(window)
    if len(xx) < w:
        return math.inf
    win, var = _windows(xx, w)
    best = math.inf
    with np.errstate(all="ignore"):
        r = float(tolerance) * np.sqrt(var)
        for a, b in _blocks(len(win), w):
            v, rr = win[a:b], r[a:b, None, None]
            rel = np.abs(np.abs(v[:, :, None] - v[:, None, :]) - rr) / rr
            rel = rel[np.broadcast_to((rr > 0.0) & np.isfinite(rr), rel.shape) & np.isfinite(rel)]
            if rel.size:
                best = min(best, float(rel.min()))
    return best


# ------------------------------------------------------------------------------------------------ comparing
def deviation(got, want):
    """The largest absolute deviation of `got` from `want`, or None when the NaN positions differ."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return None
    ok = ~np.isnan(want)
    return float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
