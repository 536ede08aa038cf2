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
Reads nothing outside the repository.

For the inputs on which the carried state is all there is -- flat, one-sided and rangeless runs -- the module also has the generator
run_series, the same recurrences in np.longdouble (exact_states: the states per channel and the output), the step up to which a
decaying state keeps all its bits (horizon) and, from the long-double states alone, the elements at which an output can be held
against the reference at all (compare_mask): where every live state is exactly 0.0 or at least 2^-969."""
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


# ---------------------------------------------------------------------------------------------- runs: the carried state alone
RUN_KINDS = ("flat", "rising", "falling", "zeros", "from_start")
STATE_FLOOR_LOG2 = -969              # 2^-1022 * 2^53: above it gradual underflow costs no bits in either evaluation order
TAINT_LOG2 = -60                     # adx_core's last average: what is left of a dx that could not be compared (see compare_mask)


def run_series(kind, n, seed, start, length, step=35, spread=30, after=None):
    """-> (high, low, close) of n bars on a 0.01 grid in integer arithmetic: the walk of hlc_walk, with a run of `length` bars from
    bar `start`, after which the walk goes on from the held level.
      flat        the close repeated and high == low == close: no gain, no loss, no range
      rising      moves of 0 or 1 cent: no loss; the distances to high and low stay
      falling     moves of 0 or -1 cent: no gain
      zeros       flat, and the three series are 0.0 on the run (a series of terms, for ewma)
      from_start  flat from bar 0 (`start` must be 0)
    after: the move in cents of the first bar behind the run, where a test wants the state to change exactly there."""
    if kind not in RUN_KINDS:
        raise ValueError(kind)
    if kind == "from_start" and start != 0:
        raise ValueError("from_start: the run begins at bar 0")
    if not (0 <= start and 0 <= length and start + length <= n):
        raise ValueError("run outside the series")
    rng = np.random.default_rng(seed)
    moves = rng.integers(-step, step + 1, n)
    below, above = rng.integers(0, spread + 1, n), rng.integers(0, spread + 1, n)
    unit = rng.integers(0, 2, n)
    run = slice(start, start + length)
    if kind == "rising":
        moves[run] = unit[run]
    elif kind == "falling":
        moves[run] = -unit[run]
    else:
        moves[run] = 0
        below[run] = 0
        above[run] = 0
    if after is not None and start + length < n:
        moves[start + length] = after
    cents = 10_000 + np.cumsum(moves)
    assert cents.min() > 100, "the walk reached the floor"
    high, low, close = (cents + above) / 100.0, (cents - below) / 100.0, cents / 100.0
    if kind == "zeros":
        for a in (high, low, close):
            a[run] = 0.0
    return high, low, close


def horizon(a):
    """ln(2^-969) / ln(a): the last step at which a state that started near 1 and decays by `a` per step is still 2^-969 or more."""
    return round(STATE_FLOOR_LOG2 / math.log2(a))


def _ld():
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 here"
    return np.longdouble


def exact_states(fn, inputs, args):
    """The recurrences of `fn` in np.longdouble on the reference's own float64 terms (differences, true ranges, +-DM: what is
    elementwise stays as the reference rounds it) -> (states, out): states[k, i] is channel k behind bar i, 0 before its seed;
    out the output from them, all in long double.  Channels: ewma u, v; rsi gain, loss; atr (EMA mode) one; adx_core the three
    sums and the last average.  A few microseconds per element: for the generator and the host tests only."""
    LD = _ld()
    if fn == "ewma":
        ys = np.asarray(inputs[0], np.float64)
        n = len(ys)
        a = LD(1.0 - 2.0 / (args[0] + 1.0))                          # the coefficient the reference multiplies by
        st = np.zeros((2, n), LD)
        u, v, one = LD(ys[0]), LD(1.0), LD(1.0)
        st[0, 0], st[1, 0] = u, v
        yl = ys.astype(LD)
        for t in range(1, n):
            u = yl[t] + a * u
            v = one + a * v
            st[0, t], st[1, t] = u, v
        return st, st[0] / st[1]
    if fn == "rsi":
        c = np.asarray(inputs[0], np.float64)
        n, w = len(c), int(args[0])
        st = np.zeros((2, n), LD)
        out = np.full(n, np.nan, LD)
        if n <= w:
            return st, out
        d = np.zeros(n)
        d[1:] = c[1:] - c[:-1]
        gain, loss = np.where(d > 0, d, 0.0).astype(LD), np.where(d < 0, -d, 0.0).astype(LD)
        wl, wm1 = LD(w), LD(w - 1)
        g, lo = LD(0.0), LD(0.0)
        for i in range(1, w + 1):
            if d[i] > 0.0:
                g = g + gain[i]
            else:
                lo = lo + LD(-d[i])
        g, lo = g / wl, lo / wl
        st[0, w], st[1, w] = g, lo
        for i in range(w + 1, n):
            g = (wm1 * g + gain[i]) / wl
            lo = (wm1 * lo + loss[i]) / wl
            st[0, i], st[1, i] = g, lo
        with np.errstate(invalid="ignore", divide="ignore"):
            out[w:] = np.where(st[1, w:] > 0, LD(100.0) - LD(100.0) / (LD(1.0) + st[0, w:] / np.where(st[1, w:] > 0, st[1, w:], LD(1.0))),
                               LD(np.nan))
        return st, out
    if fn == "atr":
        w, ema, norm = int(args[0]), bool(args[1]), bool(args[2])
        assert ema and w >= 1, "the EMA mode is the recurrence"
        h, lo, c = (np.asarray(a, np.float64) for a in inputs)
        n = len(h)
        tr = true_range(h, lo, c)
        assert not np.isnan(tr).any()
        st = np.zeros((1, n), LD)
        out = np.full(n, np.nan, LD)
        if n < w:
            return st, out
        trl = tr.astype(LD)
        wl, wm1 = LD(w), LD(w - 1)
        s = LD(0.0)
        for i in range(w):
            s = s + trl[i]
        s = s / wl
        st[0, w - 1] = s
        for i in range(w, n):
            s = (wm1 * s + trl[i]) / wl
            st[0, i] = s
        out[w - 1:] = st[0, w - 1:]
        if norm:
            mid = (h + lo) / 2.0
            assert (mid > 0).all()
            out[w - 1:] = out[w - 1:] / mid[w - 1:].astype(LD)
        return st, out
    if fn == "adx":
        L = int(args[0])
        h, lo, c = (np.asarray(a, np.float64) for a in inputs)
        n = len(h)
        tr, pdm, mdm = np.zeros(n), np.zeros(n), np.zeros(n)
        tr[1:] = _max3(h[1:] - lo[1:], np.abs(h[1:] - c[:-1]), np.abs(lo[1:] - c[:-1]))
        hd, ld = h[1:] - h[:-1], lo[:-1] - lo[1:]
        pdm[1:] = np.where((hd > ld) & (hd > 0), hd, 0.0)
        mdm[1:] = np.where((ld > hd) & (ld > 0), ld, 0.0)
        st = np.zeros((4, n), LD)
        out = np.zeros(n, LD)
        if n < L + 1:
            return st, out
        Ll = LD(L)
        for k, x in enumerate((tr, pdm, mdm)):
            xl = x.astype(LD)
            s = LD(0.0)
            for i in range(1, L + 1):
                s = s + xl[i]
            st[k, L] = s
            for i in range(L + 1, n):
                s = s - (s / Ll) + xl[i]
                st[k, i] = s
        hundred = LD(100.0)
        ok = st[0] > 0
        den = np.where(ok, st[0], LD(1.0))
        pdi, mdi = np.where(ok, hundred * (st[1] / den), LD(0.0)), np.where(ok, hundred * (st[2] / den), LD(0.0))
        tot = pdi + mdi
        ok = tot > 0
        dx = np.where(ok, hundred * (np.abs(pdi - mdi) / np.where(ok, tot, LD(1.0))), LD(0.0))
        if n >= 2 * L:
            a = LD(0.0)
            for i in range(L, 2 * L):
                a = a + dx[i]
            a = a / Ll
            st[3, 2 * L - 1] = a
            Lm1 = LD(L - 1)
            for i in range(2 * L, n):
                a = ((a * Lm1) + dx[i]) / Ll
                st[3, i] = a
        out[:] = st[3]
        return st, out
    raise ValueError(fn)


def compare_mask(fn, args, states):
    """From the long-double states alone: the elements at which the output can be held against the reference.  Every live state is
    exactly 0.0 or at least 2^-969 there.  Below that the reference loses bits to gradual underflow and stalls at the smallest
    subnormal while a composed a^len goes to 0.0; neither is the recurrence any more.  adx_core's last average is a mean of dx, and
    dx is a quotient of the three sums: a dx of a bar that is left out may be anything in 0 .. 100, and what it leaves in the
    average L bars later is at most 100 a^t after t bars.  Such an element is compared again once that is below 2^-60 (1e-18 on
    the 0 - 100 scale: nothing against a bound of 1e-11), which the long-double sums decide as well."""
    LD = _ld()
    s = np.abs(states)
    ok = ((s == 0) | (s >= LD(2.0) ** STATE_FLOOR_LOG2) | np.isnan(s)).all(axis=0)
    if fn == "adx":
        L = int(args[0])
        a, taint, limit = (L - 1) / L, 0.0, 2.0 ** TAINT_LOG2
        sums = ok.copy()
        for i in range(len(ok)):
            taint = 100.0 if not sums[i] else taint * a
            ok[i] = sums[i] and taint < limit
    return ok


def mask_ranges(mask):
    """The True stretches of a mask as [first, behind the last] pairs."""
    m = np.concatenate(([False], np.asarray(mask, bool), [False]))
    edges = np.flatnonzero(m[1:] != m[:-1])
    return [[int(a), int(b)] for a, b in zip(edges[::2], edges[1::2])]


def ranges_mask(ranges, n):
    m = np.zeros(n, bool)
    for a, b in ranges:
        m[a:b] = True
    return m


def deviation(fn, got, want, mask):
    """The largest deviation of `got` from `want` (either may be long double) over `mask` in the measure of `fn`: absolute for rsi and
    adx, relative for ewma and atr where want is not 0.0; elements where want is NaN are not measured."""
    LD = _ld()
    g, w = np.asarray(got).astype(LD), np.asarray(want).astype(LD)
    use = np.asarray(mask, bool) & ~np.isnan(w)
    if fn in ("ewma", "atr"):
        use &= w != 0
    if not use.any():
        return 0.0
    d = np.abs(g[use] - w[use])
    if fn in ("ewma", "atr"):
        d = d / np.abs(w[use])
    return float(d.max())
