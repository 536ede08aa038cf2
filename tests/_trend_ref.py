"""The definition of trend scanning (include/fmk.h) restated in NumPy, with left-to-right cumulative sums.
Evaluated in np.longdouble it is the reference the GPU results are compared with; evaluated in float64 it serves one purpose only,
measuring how far float64 arithmetic alone moves a t-value (the tolerance of tests/test_gpu_trend.py).  Reads nothing outside the
repository."""
import numpy as np

EXACT_U = 2.0 ** -26            # u at or below this: the fit counts as exact, t = copysign(inf, Sxy)


def spans(min_len, max_len, step):
    return np.arange(min_len, max_len + 1, step, dtype=np.int64)


def t_table(y, t0, min_len, max_len, step, dtype=np.longdouble):
    """t(L) of every span of the events t0 (all of them fit: t0 + max_len <= len(y)) -> an array [event, span] of `dtype`."""
    y = np.asarray(y, np.float64)
    t0 = np.asarray(t0, np.int64)
    L = spans(min_len, max_len, step)
    w = y[t0[:, None] + np.arange(max_len)[None, :]].astype(dtype)
    with np.errstate(all="ignore"):
        d = w - w[:, :1]
        j = np.arange(max_len).astype(dtype)[None, :]
        S1 = np.cumsum(d, axis=1)[:, L - 1]                      # add.accumulate: strictly left to right
        Sx = np.cumsum(j * d, axis=1)[:, L - 1]
        S2 = np.cumsum(d * d, axis=1)[:, L - 1]
        l = L.astype(dtype)[None, :]
        Sxx = l * (l * l - 1) / 12
        Sxy = Sx - (l - 1) / 2 * S1
        Syy = S2 - S1 * S1 / l
        den = Sxx * Syy
        u = 1 - Sxy * Sxy / den
        t = Sxy / np.sqrt(den) * np.sqrt((l - 2) / u)
        t = np.where(u <= dtype(EXACT_U), np.copysign(dtype(np.inf), Sxy), t)       # rule 3 (a NaN u fails the comparison)
        t = np.where(S2 == 0, dtype(0.0), t)                                        # rule 2 comes before it (a NaN S2 is not 0)
    return t


def trend_scanning(y, event_idxs, min_len, max_len, step, dtype=np.longdouble):
    """-> dict: labels int8, t_value (dtype), touch_idx int64, ret float64, skipped bool per event, n_skipped; and for the events
    that fit, `fit` (their positions in event_idxs), `table` (t_table of them), `spans`.  ret is float64 arithmetic whatever the
    dtype: the correctly rounded quotient, then the subtraction."""
    y = np.asarray(y, np.float64)
    ev = np.asarray(event_idxs, np.int64)
    n, ne = len(y), len(ev)
    assert min_len >= 3 and max_len >= min_len and step >= 1 and np.all((ev >= 0) & (ev < n))
    L = spans(min_len, max_len, step)
    labels = np.zeros(ne, np.int8)
    tval = np.full(ne, np.nan, dtype)
    touch = ev.copy()
    ret = np.full(ne, np.nan)
    fit = np.flatnonzero(ev + max_len <= n)
    table = t_table(y, ev[fit], min_len, max_len, step, dtype) if len(fit) else np.zeros((0, len(L)), dtype)
    if len(fit):
        a = np.abs(table)
        key = np.where(np.isnan(a), dtype(-1.0), a)
        k = np.argmax(key, axis=1)                               # the first of equals: the smallest L
        rows = np.arange(len(fit))
        live = key[rows, k] >= 0                                 # at least one span is not NaN
        f, kk = fit[live], k[live]
        tval[f] = table[rows[live], kk]
        labels[f] = np.sign(tval[f]).astype(np.int8)
        touch[f] = ev[f] + L[kk] - 1
        with np.errstate(all="ignore"):
            ret[f] = y[touch[f]] / y[ev[f]] - 1.0
    skipped = np.ones(ne, bool)
    skipped[fit] = False
    skipped |= np.isnan(tval)
    return dict(labels=labels, t_value=tval, touch_idx=touch, ret=ret, skipped=skipped, n_skipped=int(skipped.sum()), fit=fit,
                table=table, spans=L)


def relative_error(y, event_idxs, min_len, max_len, step):
    """The largest relative error of the float64 restatement's t_value against the longdouble reference's, over the events whose
    reference t_value is finite and not zero and whose two evaluations chose the same span -> (error, events compared, events
    whose span differs)."""
    ref = trend_scanning(y, event_idxs, min_len, max_len, step, np.longdouble)
    f64 = trend_scanning(y, event_idxs, min_len, max_len, step, np.float64)
    same = ref["touch_idx"] == f64["touch_idx"]
    ok = np.isfinite(ref["t_value"]) & (ref["t_value"] != 0) & same & ~ref["skipped"]
    moved = int((~same).sum())
    if not ok.any():
        return 0.0, 0, moved
    r = ref["t_value"][ok]
    err = np.abs(f64["t_value"][ok].astype(np.longdouble) - r) / np.abs(r)
    return float(err.max()), int(ok.sum()), moved
