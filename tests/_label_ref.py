"""Plain NumPy restatement of the label loops (finmlkit/label/tbm.py, label/weights.py) in the reference's evaluation order, with
math.log per element for the logarithms (libm: the project's `log` contract).  What GPU results are compared with on tapes that
have no fixture.  Reads nothing outside the repository."""
import math

import numpy as np

CHUNK = 1 << 16


def host_log(x):
    """math.log extended the way glibc and csrc/fmk_log.h define it: +-0 -> -inf, negative -> NaN, NaN -> NaN, +inf -> +inf."""
    x = float(x)
    if x > 0.0:
        return math.log(x)
    return -math.inf if x == 0.0 else math.nan


def log_column(close):
    return np.fromiter((host_log(x) for x in close), np.float64, len(close))


def first_open(ts, i0, t1, mc_ns):
    """first j in (i0, t1] with float64(ts[j] - ts[i0]) >= mc_ns (tbm.py:111-114), t1 + 1 when there is none.  The ticks held back
    are a prefix of the window (sorted timestamps) and int -> float64 is monotone, so the condition is ts[j] - t0 >= d for the
    smallest integer d whose float64 reaches mc_ns: one search on the integer column."""
    if mc_ns <= 0.0:
        return i0 + 1
    t0 = ts[i0]
    if not mc_ns < 2.0 ** 53:
        return i0 + 1 + int(np.searchsorted((ts[i0 + 1:t1 + 1] - t0).astype(np.float64), mc_ns, side="left"))
    d = int(math.ceil(mc_ns))                                   # exact below 2^53
    return min(t1 + 1, max(i0 + 1, int(np.searchsorted(ts, int(t0) + d, side="left"))))


def triple_barrier(timestamps, close, event_idxs, targets, horizontal_barriers, vertical_barrier, min_close_time_sec, side,
                   min_ret, log_close=None):
    """-> (labels, touch_idxs, rets, max_rb_ratios, skipped): `skipped` marks the events the reference leaves out
    (t1_idx <= event_idx: label 0, NaN, and -- this project's definition -- the event's own index as touch index).
    A tick whose return is NaN touches nothing and is left out of the two extrema, that tick alone (tbm.py:119-132: every
    comparison with NaN is false); `ret` is the value at the last evaluated tick, NaN included.  Project definition: with
    side=None and a NaN final return the reference cannot answer (interpreted it raises `cannot convert float NaN to integer`,
    compiled it stores an undefined int8); the label is then 1, what `ret < 0 ? -1 : 1` gives."""
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
        js = first_open(ts, i0, t1, mc_ns)
        ret, hit, tch = 0.0, False, t1
        rmax, rmin = -np.inf, np.inf
        j = js
        while j <= t1 and not hit:
            e = min(j + CHUNK, t1 + 1)
            with np.errstate(invalid="ignore"):
                r = (lc[j:e] - lc[i0]) * s
            m = (r >= upper) | (r <= lower)
            if m.any():
                k = int(np.argmax(m))
                hit, tch = True, j + k
                r = r[:k + 1]
            with np.errstate(invalid="ignore"):                  # an all-NaN chunk: NaN, which max / min below leave out
                rmax, rmin = max(rmax, float(np.fmax.reduce(r))), min(rmin, float(np.fmin.reduce(r)))
            ret = float(r[-1])
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


def triple_barrier_scalar(timestamps, close, event_idxs, targets, horizontal_barriers, vertical_barrier, min_close_time_sec, side,
                          min_ret):
    """The reference's loop tick by tick (tbm.py:77-156 line for line, Python floats: the same IEEE operations), for small tapes.
    Same outputs and the same two project definitions as triple_barrier above."""
    ts = np.asarray(timestamps, np.int64)
    tsf = ts.astype(np.float64)                                 # searchsorted(int64 column, float64 key) compares in float64
    lc = [host_log(x) for x in close]
    ne = len(event_idxs)
    is_meta = side is not None
    bottom_mult, top_mult = float(horizontal_barriers[0]), float(horizontal_barriers[1])
    vertical_barrier_ns = vertical_barrier * 1e9
    min_close_time_ns = min_close_time_sec * 1e9
    labels = np.zeros(ne, np.int8)
    touch = np.empty(ne, np.int64)
    rets = np.full(ne, np.nan)
    ratios = np.full(ne, np.nan)
    skipped = np.zeros(ne, bool)
    tsl = ts.tolist()
    for i in range(ne):
        t0_idx = int(event_idxs[i])
        tgt = float(targets[i])
        upper_barrier = tgt * top_mult
        lower_barrier = -tgt * bottom_mult
        upper_valid = math.isfinite(upper_barrier) and upper_barrier != 0.0
        lower_valid = math.isfinite(lower_barrier) and lower_barrier != 0.0
        t0 = tsl[t0_idx]
        t1 = float(t0) + vertical_barrier_ns
        t1_idx = int(np.searchsorted(tsf, t1, side="right")) - 1
        if t1_idx <= t0_idx:
            skipped[i] = True
            touch[i] = t0_idx
            continue
        side_mult = float(side[i]) if is_meta else 1.0
        touch_idx = t1_idx
        max_urbr = 0.0
        max_lrbr = 0.0
        base_price = lc[t0_idx]
        ret = 0.
        for j in range(t0_idx + 1, t1_idx + 1):
            dur_ns = tsl[j] - t0
            if float(dur_ns) < min_close_time_ns:
                continue
            ret = (lc[j] - base_price) * side_mult
            if ret > 0.0 and upper_valid:
                max_urbr = max(max_urbr, ret / upper_barrier)
            elif ret < 0.0 and lower_valid:
                max_lrbr = max(max_lrbr, ret / lower_barrier)
            if ret >= upper_barrier:
                touch_idx = j
                break
            if ret <= lower_barrier:
                touch_idx = j
                break
        touch[i] = touch_idx
        rets[i] = ret
        if is_meta:
            labels[i] = 1 if ret >= min_ret else 0
        else:
            labels[i] = -1 if ret < 0 else 1                    # sign(ret), 1 for 0 -- and 1 for NaN (project definition)
        if touch_idx == t1_idx:
            if ret > 0.:
                max_rbr = max_urbr / (1 + max_lrbr)
                max_rbr = max_rbr if upper_valid else math.nan
            else:
                max_rbr = max_lrbr / (1 + max_urbr)
                max_rbr = max_rbr if lower_valid else math.nan
            ratios[i] = min(max_rbr, 1.)
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


def uniqueness_given(conc, event_idxs, touch_idxs):
    """weights.py:41-47 on a concurrency column the caller supplies -> (weights, mean |1 / c| per event: the scale of the 1e-9
    contract, on the absolute terms so that cancelling negative 1 / c cannot hide an error)."""
    ne = len(event_idxs)
    w, scale = np.zeros(ne), np.zeros(ne)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(ne):
            inv = 1.0 / np.asarray(conc)[int(event_idxs[i]):int(touch_idxs[i]) + 1]
            w[i], scale[i] = np.mean(inv), np.mean(np.abs(inv))
    return w, scale


def attribution_terms(close, conc):
    """term_j = log(close[j] / close[j-1]) / concurrency[j], 0 where the reference adds nothing (weights.py:76-92)."""
    close = np.asarray(close, np.float64)
    n = len(close)
    lr = np.full(n, np.nan)
    for j in range(1, n):
        if close[j - 1] != 0.0:
            with np.errstate(all="ignore"):
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
        with np.errstate(invalid="ignore"):                      # +inf and -inf terms in one event: NaN, like the loop
            w[i] = abs(np.cumsum(t)[-1]) if len(t) else 0.0      # cumsum adds in order, like the loop
            bound[i] = len(t) * 2.0 ** -52 * np.abs(t).sum()
    if normalize:
        total = np.sum(w)
        if total <= 0.:
            raise ValueError("Sum of weights is zero or negative, cannot normalize.")
        w *= ne / total
    return w, bound
