"""Plain sequential restatement of the reference's running-sum indicators -- bollinger_percent_b and parkinson_range
(feature/core/volatility.py), vwap_distance (feature/core/reversion.py), comp_flow_acceleration and vpin (feature/core/volume.py) --
that must agree with the reference in its pure-Python mode bit for bit (with the host's log in place of NumPy's own).  Every sum is
a loop over Python floats (IEEE float64, one rounded operation each) in the reference's order, every output the reference's
expression; `** 2` is a product.

  bollinger_percent_b  window < 1 refused; NaN before window - 1; T = window * mean * mean at window - 1, window * (mean * mean) after
  vwap_distance        n_periods < 1 refused; the first window is the simple form in either mode; where vsum > 0 is false the
                       output before
  comp_flow_accel.     negative recent_periods refused; NaN everywhere when n < window or recent_periods >= window
  vpin                 negative window refused; float32; a bar with a NaN adds 0.0 to the sums and 1 to the count
  parkinson_range      log(high / low) ** 2 / (log(2.0) * 4.0)
The generators are in integer arithmetic and seeded; zero_lot_volumes has zero-volume bars among volumes that are not exactly summable.
`sums=True` returns the internal sums beside the output (for the condition number of the Bollinger variance).
Reads nothing outside the repository."""
import math
import sys

import numpy as np

from tests._order_ref import _div, grid_walk, nan_canonical, sha256  # noqa: F401 -- part of this module's interface
from tests._recur_ref import hlc_walk  # noqa: F401

BOLLINGER_MESSAGE = "bollinger_percent_b: window must be at least 1."
VWAP_MESSAGE = "vwap_distance: n_periods must be at least 1."
VWAP_SHAPE_MESSAGE = "vwap_distance: close and volume must have the same length."
FLOW_MESSAGE = "comp_flow_acceleration: recent_periods must not be negative."
VPIN_MESSAGE = "vpin: window must not be negative."
VPIN_SHAPE_MESSAGE = "vpin: volume_buy and volume_sell must have the same length."
PARKINSON_MESSAGE = "parkinson_range: high and low must have the same length."
NAN = math.nan
EPS = 1e-12


# ---------------------------------------------------------------------------------------------------------------- inputs
def grid64_walk(n, seed, step=35, hold=0.0):
    """A seeded walk on a 1/64 price grid around 100, in integer arithmetic: every price, square and difference is exact."""
    rng = np.random.default_rng(seed)
    moves = rng.integers(-step, step + 1, n)
    moves[rng.random(n) < hold] = 0
    return np.maximum(6_400 + np.cumsum(moves), 64) / 64.0


def int_volumes(n, seed, runs=()):
    """Integer volumes 0 .. 49 with zeros planted over each (start, length) of `runs`."""
    v = np.random.default_rng(seed).integers(0, 50, n).astype(np.float64)
    for start, length in runs:
        v[start:start + length] = 0.0
    return v


def lot_volumes(n, seed):
    """Volumes 0.01 .. 50.00 on a 0.01 grid: not exactly summable."""
    return np.random.default_rng(seed).integers(1, 5001, n) / 100.0


def zero_lot_volumes(n, seed, runs=(), share=0.3):
    """Volumes 1.01 .. 51.00 on a 0.01 grid (not exactly summable) with zero-volume bars: a `share` of the bars at seeded places and
    every bar of each (start, length) of `runs` is 0.0.  The floor of 1.01 keeps every window sum that is not zero far above the
    rounding noise of a prefix sum (about 3e-11 at these totals)."""
    v = np.random.default_rng(seed).integers(1, 5001, n) / 100.0 + 1.0
    v[np.random.default_rng(seed + 1000).random(n) < share] = 0.0
    for start, length in runs:
        v[start:start + length] = 0.0
    return v


def zero_lot_kilo(n, seed, runs=(), share=0.3):
    """zero_lot_volumes x 1024 (exact): totals of 1e8, where one unit in the last place of a prefix sum exceeds vpin's 1e-9."""
    return zero_lot_volumes(n, seed, runs, share) * 1024.0


def zero_lot_nan(n, seed, runs, at):
    """zero_lot_volumes with a NaN in element `at`: every prefix sum behind it is NaN, over zero bars as well."""
    v = zero_lot_volumes(n, seed, runs)
    v[at] = NAN
    return v


GENERATORS = {
    "grid_walk": grid_walk, "grid64_walk": grid64_walk, "int_volumes": int_volumes, "lot_volumes": lot_volumes,
    "zero_lot_volumes": zero_lot_volumes, "zero_lot_kilo": zero_lot_kilo, "zero_lot_nan": zero_lot_nan,
    "hlc_high": lambda *a: hlc_walk(*a)[0], "hlc_low": lambda *a: hlc_walk(*a)[1], "hlc_close": lambda *a: hlc_walk(*a)[2],
}


def generate(source):
    """The inputs of a fixture case from its `source`: one [generator name, arguments] per input."""
    return tuple(GENERATORS[g](*a) for g, a in source)


def _log(v):
    """The host's log: -inf at 0, NaN below (no exception)."""
    if v > 0.0:
        return math.log(v) if v != math.inf else math.inf
    return -math.inf if v == 0.0 else NAN


# ---------------------------------------------------------------------------------------------------------------- the functions
def bollinger_percent_b(close, window, num_std, sums=False):
    w = int(window)
    if w < 1:
        raise ValueError(BOLLINGER_MESSAGE)
    c = np.asarray(close, np.float64).tolist()
    n = len(c)
    out = np.full(n, np.nan)
    sq, var_ = np.full(n, np.nan), np.full(n, np.nan)
    if n >= w:
        s = q = 0.0
        for k in range(w):
            s += c[k]
            q += c[k] * c[k]
        for i in range(w - 1, n):
            if i >= w:
                s += c[i] - c[i - w]
                q += c[i] * c[i] - c[i - w] * c[i - w]
            mean = s / w
            t = w * mean * mean if i == w - 1 else w * (mean * mean)
            var = _div(q - t, w - 1)
            sd = math.sqrt(max(var, 0.0))
            lower, upper = mean - num_std * sd, mean + num_std * sd
            out[i] = (c[i] - lower) / (upper - lower) if upper > lower else NAN
            sq[i], var_[i] = q, var
    return (out, sq, var_) if sums else out


def vwap_distance(close, volume, n_periods, is_log, sums=False):
    w = int(n_periods)
    if w < 1:
        raise ValueError(VWAP_MESSAGE)
    c, v = np.asarray(close, np.float64).tolist(), np.asarray(volume, np.float64).tolist()
    if len(c) != len(v):
        raise ValueError(VWAP_SHAPE_MESSAGE)
    n = len(c)
    out = np.full(n, np.nan)
    held = np.zeros(n, bool)
    if n >= w:
        ws = vs = 0.0
        for k in range(w):
            ws += c[k] * v[k]
            vs += v[k]
        if vs > 0:
            out[w - 1] = _div(c[w - 1], ws / vs) - 1.0
        else:
            held[w - 1] = True
        for i in range(w, n):
            ws += c[i] * v[i] - c[i - w] * v[i - w]
            vs += v[i] - v[i - w]
            if vs > 0:
                q = _div(c[i], ws / vs)
                out[i] = _log(q) if is_log else q - 1.0
            else:
                out[i] = out[i - 1]
                held[i] = True
    return (out, held) if sums else out


def comp_flow_acceleration(volumes, window, recent_periods):
    w, r = int(window), int(recent_periods)
    if r < 0:
        raise ValueError(FLOW_MESSAGE)
    v = np.asarray(volumes, np.float64).tolist()
    n = len(v)
    out = np.full(n, np.nan)
    if n < w or r >= w:
        return out
    s = [0.0] * (n + 1)
    for i in range(n):
        s[i + 1] = s[i] + v[i]
    for i in range(w - 1, n):
        recent = s[i + 1] - s[i + 1 - r]
        past = s[i + 1 - r] - s[i + 1 - w]
        out[i] = _log(_div(recent + EPS, past + EPS))
    return out


def vpin(volume_buy, volume_sell, window, sums=False):
    w = int(window)
    if w < 0:
        raise ValueError(VPIN_MESSAGE)
    b, s = np.asarray(volume_buy, np.float64).tolist(), np.asarray(volume_sell, np.float64).tolist()
    if len(b) != len(s):
        raise ValueError(VPIN_SHAPE_MESSAGE)
    n = len(b)
    out = np.full(n, np.nan, np.float32)
    quot = np.full(n, np.nan)
    bc, sc, ac, nc = [0.0] * (n + 1), [0.0] * (n + 1), [0.0] * (n + 1), [0] * (n + 1)
    for i in range(n):
        bad = b[i] != b[i] or s[i] != s[i]
        bc[i + 1] = bc[i] + (0.0 if bad else b[i])
        sc[i + 1] = sc[i] + (0.0 if bad else s[i])
        ac[i + 1] = ac[i] + (0.0 if bad else abs(b[i] - s[i]))
        nc[i + 1] = nc[i] + bad
        if i >= w - 1 and nc[i + 1] - nc[i + 1 - w] == 0:
            tot = (bc[i + 1] - bc[i + 1 - w]) + (sc[i + 1] - sc[i + 1 - w])
            if tot > 1e-9:
                quot[i] = (ac[i + 1] - ac[i + 1 - w]) / tot
                out[i] = np.float32(quot[i])
    return (out, quot) if sums else out


def parkinson_range(high, low):
    h, lo = np.asarray(high, np.float64).tolist(), np.asarray(low, np.float64).tolist()
    if len(h) != len(lo):
        raise ValueError(PARKINSON_MESSAGE)
    ln2 = math.log(2.0) * 4.0
    out = np.empty(len(h), np.float64)
    for i in range(len(h)):
        lg = _log(_div(h[i], lo[i]))
        out[i] = (lg * lg) / ln2
    return out


def flat_windows(close, window):
    """Where the window that ends at i holds equal elements only (a true variance of zero); False before window - 1."""
    c = np.asarray(close, np.float64)
    flat = np.zeros(len(c), bool)
    if window >= 1 and len(c) >= window:
        view = np.lib.stride_tricks.sliding_window_view(c, window)
        flat[window - 1:] = (view == view[:, :1]).all(axis=1)
    return flat


def zero_windows(v, window):
    """Where the window that ends at i holds zeros only (the twin of flat_windows); False before window - 1."""
    v = np.asarray(v, np.float64)
    zero = np.zeros(len(v), bool)
    if window >= 1 and len(v) >= window:
        zero[window - 1:] = (np.lib.stride_tricks.sliding_window_view(v, window) == 0.0).all(axis=1)
    return zero


NAMES = {"boll": "bollinger_percent_b", "vwap": "vwap_distance", "flow": "comp_flow_acceleration", "vpin": "vpin",
         "park": "parkinson_range"}
N_INPUTS = {"boll": 1, "vwap": 2, "flow": 1, "vpin": 2, "park": 2}


def call(fn, inputs, args, mod=None):
    """One fixture case on this module (or on `mod`, which has the reference's names).  `inputs`: a tuple of series; `args`: the
    arguments after them."""
    mod = mod or sys.modules[__name__]
    return getattr(mod, NAMES[fn])(*inputs, *args)
