"""Plain sequential restatement of the reference's recursive indicators -- ewma (feature/core/ma.py), rsi_wilder
(feature/core/momentum.py), true_range and atr (feature/core/volatility.py), adx_core (feature/core/trend.py) -- that must agree
with the reference in its pure-Python mode bit for bit.  Every recurrence is a loop over Python floats (IEEE float64, one rounded
operation each) with the reference's own per-step expression; what is elementwise (true range, +-DM, the directional indices) is
NumPy, which rounds the same way.  Two sums of adx_core are the reference's own calls: np.sum / np.mean over the seed windows (NumPy
adds pairwise there; the kernels add in index order, which is inside their tolerance).  The SMA mode of atr adds each window left
to right, one position of all windows at a time.

  ewma         span < 1 refused; u = y[t] + (1 - alpha) * u, v = 1 + (1 - alpha) * v from (y[0], 1), u / v
  rsi_wilder   window < 1 refused; NaN before window; the first window's gains and losses over window, then
               ((window - 1) * avg + x) / window; 100 - 100 / (1 + g / l) where l > 0, NaN otherwise
  true_range   bar 0: high - low; max(high - low, |high - close[i-1]|, |low - close[i-1]|); NaN where an input is
  atr          negative window refused; SMA: mean of the window's non-NaN true ranges, NaN at bar 2 when its three prices are NaN;
               EMA: mean of the first window's, then ((window - 1) * atr + tr) / window, NaN for good after a NaN
  adx_core     length < 1 refused; 0.0 before 2 * length - 1
Reads nothing outside the repository."""
import math
import sys

import numpy as np

from tests._order_ref import grid_walk, nan_canonical, ohlc_walk, sha256  # noqa: F401 -- part of this module's interface

SPAN_MESSAGE = "span size is less than or equal to 1. Please provide a span size greater than 1."
RSI_WINDOW_MESSAGE = "rsi_wilder: window must be at least 1."
ATR_WINDOW_MESSAGE = "atr: window must not be negative."
HLC_MESSAGE = "The length of high, low, and close prices must be the same."
ADX_LENGTH_MESSAGE = "adx_core: length must be at least 1."
ADX_SHAPE_MESSAGE = "adx_core: high, low and close must have the same length."
NAN = math.nan


def hlc_walk(n, seed, step=35, spread=30, hold=0.0):
    """ohlc_walk in the order the indicators take their columns: (high, low, close)."""
    close, low, high = ohlc_walk(n, seed, step, spread, hold)
    return high, low, close


def longest_loss_free_run(close):
    """The longest run of consecutive differences of `close` that are not negative (NaN counts as none)."""
    d = np.diff(np.asarray(close, np.float64))
    best = cur = 0
    for neg in (d < 0).tolist():
        cur = 0 if neg else cur + 1
        best = max(best, cur)
    return best


def _max3(a, b, c):
    """Python's max(a, b, c) elementwise: the first of the largest, a NaN staying where it comes first."""
    with np.errstate(invalid="ignore"):
        m = np.where(b > a, b, a)
        return np.where(c > m, c, m)


def ewma(y, span):
    if not span >= 1:
        raise ValueError(SPAN_MESSAGE)
    ys = np.asarray(y, np.float64).tolist()
    out = np.empty(len(ys), np.float64)
    if not ys:
        return out                     # (the reference raises IndexError here)
    alpha = 2.0 / (span + 1.0)
    u, v = ys[0], 1.0
    out[0] = u / v
    for t in range(1, len(ys)):
        u = ys[t] + (1.0 - alpha) * u
        v = 1.0 + (1.0 - alpha) * v
        out[t] = u / v
    return out


def rsi_wilder(close, window):
    if int(window) < 1:
        raise ValueError(RSI_WINDOW_MESSAGE)
    c = np.asarray(close, np.float64).tolist()
    n = len(c)
    out = np.full(n, np.nan)
    if n <= window:
        return out
    g = lo = 0.0
    for i in range(1, window + 1):
        diff = c[i] - c[i - 1]
        if diff > 0.0:
            g += diff
        else:
            lo += -diff
    g, lo = g / window, lo / window
    out[window] = 100.0 - 100.0 / (1.0 + g / lo) if lo > 0 else NAN
    for i in range(window + 1, n):
        diff = c[i] - c[i - 1]
        gain = diff if diff > 0.0 else 0.0
        loss = -diff if diff < 0.0 else 0.0
        g = ((window - 1) * g + gain) / window
        lo = ((window - 1) * lo + loss) / window
        out[i] = 100.0 - 100.0 / (1.0 + g / lo) if lo > 0 else NAN
    return out


def _hlc(high, low, close, message):
    h, lo, c = (np.asarray(a, np.float64) for a in (high, low, close))
    if not len(h) == len(lo) == len(c):
        raise ValueError(message)
    return h, lo, c


def true_range(high, low, close):
    h, lo, c = _hlc(high, low, close, HLC_MESSAGE)
    tr = np.empty(len(h), np.float64)
    if not len(h):
        return tr
    tr[0] = NAN if (np.isnan(h[0]) or np.isnan(lo[0])) else h[0] - lo[0]
    with np.errstate(invalid="ignore"):
        cp = c[:-1]
        m = _max3(h[1:] - lo[1:], np.abs(h[1:] - cp), np.abs(lo[1:] - cp))
    tr[1:] = np.where(np.isnan(h[1:]) | np.isnan(lo[1:]) | np.isnan(cp), np.nan, m)
    return tr


def atr(high, low, close, window, ema_based=False, normalize=False):
    if int(window) < 0:
        raise ValueError(ATR_WINDOW_MESSAGE)
    h, lo, c = _hlc(high, low, close, HLC_MESSAGE)
    n = len(h)
    tr = true_range(h, lo, c)
    out = np.full(n, np.nan)
    if n < window or window == 0 or n == 0:
        return out                     # (window 0: every window of the reference is empty)
    if ema_based:
        trs = tr.tolist()
        s, cnt = 0.0, 0
        for i in range(window):
            if trs[i] == trs[i]:
                s += trs[i]
                cnt += 1
        prev = s / cnt if cnt > 0 else NAN
        out[window - 1] = prev
        for i in range(window, n):
            prev = NAN if (trs[i] != trs[i] or prev != prev) else ((window - 1) * prev + trs[i]) / window
            out[i] = prev
    else:
        view = np.lib.stride_tricks.sliding_window_view(tr, window)
        s = np.zeros(len(view))
        cnt = np.zeros(len(view), np.int64)
        for j in range(window):                                      # position j of every window: left to right per window
            col = view[:, j]
            ok = ~np.isnan(col)
            s = np.where(ok, s + np.where(ok, col, 0.0), s)
            cnt += ok
        with np.errstate(invalid="ignore", divide="ignore"):
            out[window - 1:] = np.where(cnt > 0, s / np.where(cnt > 0, cnt, 1), np.nan)
        if window <= 3 and n > 2 and np.isnan(h[2]) and np.isnan(lo[2]) and np.isnan(c[2]):
            out[2] = NAN
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            mid = (h + lo) / 2.0
            ok = ~np.isnan(out) & ~np.isnan(mid) & (mid > 0)
            out = np.where(ok, out / np.where(ok, mid, 1.0), out)
    return out


def adx_core(high, low, close, length):
    if int(length) < 1:
        raise ValueError(ADX_LENGTH_MESSAGE)
    h, lo, c = _hlc(high, low, close, ADX_SHAPE_MESSAGE)
    size = len(h)
    tr, pdm, mdm = np.zeros(size), np.zeros(size), np.zeros(size)
    if size > 1:
        with np.errstate(invalid="ignore"):
            tr[1:] = _max3(h[1:] - lo[1:], np.abs(h[1:] - c[:-1]), np.abs(lo[1:] - c[:-1]))
            hd, ld = h[1:] - h[:-1], lo[:-1] - lo[1:]
            pdm[1:] = np.where((hd > ld) & (hd > 0), hd, 0.0)
            mdm[1:] = np.where((ld > hd) & (ld > 0), ld, 0.0)
    sm = [np.zeros(size), np.zeros(size), np.zeros(size)]
    if size >= length + 1:
        for k, x in enumerate((tr, pdm, mdm)):
            xs = x.tolist()
            s = float(np.sum(x[1:length + 1]))
            col = sm[k]
            col[length] = s
            for i in range(length + 1, size):
                s = s - (s / length) + xs[i]
                col[i] = s
    str_, spdm, smdm = sm
    pdi, mdi, dx = np.zeros(size), np.zeros(size), np.zeros(size)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = str_ > 0
        ok[:length] = False
        den = np.where(ok, str_, 1.0)
        pdi = np.where(ok, 100 * (spdm / den), 0.0)
        mdi = np.where(ok, 100 * (smdm / den), 0.0)
        tot = pdi + mdi
        ok = tot > 0
        ok[:length] = False
        dx = np.where(ok, 100 * (np.abs(pdi - mdi) / np.where(ok, tot, 1.0)), 0.0)
    adx = np.zeros(size)
    if size >= 2 * length:
        a = float(np.mean(dx[length:2 * length]))
        adx[2 * length - 1] = a
        dxs = dx.tolist()
        for i in range(2 * length, size):
            a = ((a * (length - 1)) + dxs[i]) / length
            adx[i] = a
    return adx


def call(fn, inputs, args, mod=None):
    """One fixture case on this module (or on `mod`, which has the reference's names).  `inputs`: a tuple of series, (y,) or
    (close,) or (high, low, close); `args`: the arguments after them."""
    mod = mod or sys.modules[__name__]
    f = {"ewma": "ewma", "rsi": "rsi_wilder", "tr": "true_range", "atr": "atr", "adx": "adx_core"}[fn]
    return getattr(mod, f)(*inputs, *args)
