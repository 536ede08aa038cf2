"""Plain NumPy restatement of the label loops (finmlkit/label/tbm.py, label/weights.py) in the reference's evaluation order, with
math.log per element for the logarithms (libm: the project's `log` contract).  What GPU results are compared with on tapes that
have no fixture.  Reads nothing outside the repository."""
import math

import numpy as np

CHUNK = 1 << 16


def log_column(close):
    return np.fromiter((math.log(x) for x in close), np.float64, len(close))


def triple_barrier(timestamps, close, event_idxs, targets, horizontal_barriers, vertical_barrier, min_close_time_sec, side,
                   min_ret, log_close=None):
    """-> (labels, touch_idxs, rets, max_rb_ratios, skipped): `skipped` marks the events the reference leaves out
    (t1_idx <= event_idx: label 0, NaN, and -- this project's definition -- the event's own index as touch index)."""
    ts = np.asarray(timestamps, np.int64)
    lc = log_column(close) if log_close is None else log_close
    tsf = ts.astype(np.float64)
    ne = len(event_idxs)
    is_meta = side is not None
    bottom, top = horizontal_barriers
    vb_ns, mc_ns = vertical_barrier * 1e9, min_close_time_sec * 1e9
    labels = np.zeros(ne, np.int8)
    touch = np.empty(ne, np.int64)
    rets = np.full(ne, np.nan)
    ratios = np.full(ne, np.nan)
    skipped = np.zeros(ne, bool)
    for i in range(ne):
        i0 = int(event_idxs[i])
        with np.errstate(invalid="ignore"):
            upper = np.float64(targets[i]) * np.float64(top)
            lower = -np.float64(targets[i]) * np.float64(bottom)
        uv = bool(np.isfinite(upper) and upper != 0.0)
        lv = bool(np.isfinite(lower) and lower != 0.0)
        t0 = ts[i0]
        t1 = int(np.searchsorted(tsf, np.float64(t0) + vb_ns, side="right")) - 1
        if t1 <= i0:
            skipped[i] = True
            touch[i] = i0
            continue
        s = np.float64(side[i]) if is_meta else np.float64(1.0)
        # the ticks min_close_time holds back are a prefix of the window (sorted timestamps)
        js = i0 + 1 + int(np.searchsorted((ts[i0 + 1:t1 + 1] - t0).astype(np.float64), mc_ns, side="left"))
        ret, hit, tch = 0.0, False, t1
        rmax, rmin = -np.inf, np.inf
        j = js
        while j <= t1 and not hit:
            e = min(j + CHUNK, t1 + 1)
            r = (lc[j:e] - lc[i0]) * s
            m = (r >= upper) | (r <= lower)
            if m.any():
                k = int(np.argmax(m))
                hit, tch = True, j + k
                r = r[:k + 1]
            rmax, rmin, ret = max(rmax, float(r.max())), min(rmin, float(r.min())), float(r[-1])
            j = e
        touch[i] = tch
        rets[i] = ret
        if is_meta:
            labels[i] = 1 if ret >= min_ret else 0
        else:
            labels[i] = -1 if ret < 0 else 1
        if tch == t1:
            with np.errstate(all="ignore"):
                urbr = max(0.0, float(np.float64(rmax) / upper)) if (uv and rmax > 0.0) else 0.0
                lrbr = max(0.0, float(np.float64(rmin) / lower)) if (lv and rmin < 0.0) else 0.0
            if ret > 0.:
                rb = urbr / (1 + lrbr) if uv else np.nan
            else:
                rb = lrbr / (1 + urbr) if lv else np.nan
            ratios[i] = 1. if 1. < rb else rb
        else:
            ratios[i] = 1.
    return labels, touch, rets, ratios, skipped


def concurrency(n, event_idxs, touch_idxs):
    d = np.zeros(n + 1, np.int64)
    np.add.at(d, np.asarray(event_idxs, np.int64), 1)
    np.add.at(d, np.asarray(touch_idxs, np.int64) + 1, -1)
    return np.cumsum(d[:n]).astype(np.int16)             # the reference adds in int16: the same value mod 2^16


def average_uniqueness(timestamps, event_idxs, touch_idxs):
    n, ne = len(timestamps), len(event_idxs)
    conc = concurrency(n, event_idxs, touch_idxs)
    w = np.zeros(ne, np.float64)
    for i in range(ne):
        w[i] = np.mean(1.0 / conc[int(event_idxs[i]):int(touch_idxs[i]) + 1])
    return w, conc


def attribution_terms(close, conc):
    """term_j = log(close[j] / close[j-1]) / concurrency[j], 0 where the reference adds nothing (weights.py:76-92)."""
    close = np.asarray(close, np.float64)
    n = len(close)
    lr = np.full(n, np.nan)
    for j in range(1, n):
        if close[j - 1] != 0.0:
            q = close[j] / close[j - 1]
            if 0.0 < q < math.inf:
                lr[j] = math.log(q)
            else:
                with np.errstate(all="ignore"):
                    lr[j] = np.log(np.float64(q))
    ok = (np.asarray(conc) > 0) & ~np.isnan(lr)
    term = np.zeros(n, np.float64)
    term[ok] = lr[ok] / np.asarray(conc)[ok]
    return term


def return_attribution(event_idxs, touch_idxs, close, conc, normalize, terms=None):
    """-> (weights, bound): the serial sum per event, and L * 2^-52 * sum|term| of the event (the re-association bound)."""
    term = attribution_terms(close, conc) if terms is None else terms
    ne = len(event_idxs)
    w, bound = np.zeros(ne), np.zeros(ne)
    for i in range(ne):
        t = term[int(event_idxs[i]):int(touch_idxs[i]) + 1]
        w[i] = abs(np.cumsum(t)[-1]) if len(t) else 0.0          # cumsum adds in order, like the loop
        bound[i] = len(t) * 2.0 ** -52 * np.abs(t).sum()
    if normalize:
        total = np.sum(w)
        if total <= 0.:
            raise ValueError("Sum of weights is zero or negative, cannot normalize.")
        w *= ne / total
    return w, bound
