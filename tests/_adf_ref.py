"""The definition of the ADF / SADF statistic (include/fmk.h) restated in NumPy, vectorised over the end points:
for each window length m the row t - m + 1 of every end point t is added to the running moments at once, so Python loops only over m
and over the k^2 moments.  dtype=np.longdouble is the reference the GPU is compared with; dtype=np.float64 is the same recurrence in
the device's number format (left-to-right sums, where the device sums 64-row blocks plus a carry), whose distance from the reference
sizes the GPU tolerance (tests/test_adf_host.py)."""
import numpy as np

DEGENERATE = 2.0 ** -26              # csrc/fmk_sadf.hip: SADF_DEGENERATE
EXACT = 2.0 ** -26                   # csrc/fmk_sadf.hip: SADF_EXACT
BAND_HIGH, BAND_LOW = 2.0 ** -20, 2.0 ** -32       # no test input may put a pivot or a fit between these
TRENDS = {"c": 0, "ct": 1}


def regressors(lags, trend):
    return lags + 2 + TRENDS[trend]


def _solve(A, k, m, dtype):
    """The elimination of include/fmk.h on a (k+1) x (k+1) lower triangle of arrays (destroyed) -> (stat, degenerate, smallest
    relative pivot, in_band, fit ratio).  stat is NaN where the window is degenerate or holds a NaN."""
    yy = A[k][k].copy()
    g = [A[j][j].copy() for j in range(k)]
    shape = yy.shape
    degenerate = np.zeros(shape, bool)
    min_rel = np.full(shape, np.inf)
    in_band = np.zeros(shape, bool)
    with np.errstate(all="ignore"):
        for j in range(k):
            d = A[j][j]
            degenerate |= ~(d > dtype(DEGENERATE) * g[j])
            rel = np.where(g[j] == 0, 0.0, (d / g[j])).astype(np.float64)
            firm = degenerate | in_band                  # decided by an earlier pivot: what follows is not looked at
            in_band |= ~firm & (rel >= BAND_LOW) & (rel <= BAND_HIGH)
            min_rel = np.where(~firm & (rel > BAND_HIGH), np.minimum(min_rel, rel), min_rel)
            inv = dtype(1) / d
            for i in range(j + 1, k + 1):
                l = A[i][j] * inv
                for r in range(j + 1, i + 1):
                    A[i][r] = A[i][r] - l * A[r][j]
        z, dl, ssr = A[k][k - 1], A[k - 1][k - 1], A[k][k]
        ratio = ssr / yy
        stat = z / np.sqrt(dl * ssr / dtype(m - k))
        stat = np.where(ratio <= dtype(EXACT), np.copysign(dtype(np.inf), z), stat)
        stat = np.where(degenerate, dtype(np.nan), stat)
    return stat, degenerate, min_rel, in_band, np.where(degenerate, np.nan, ratio.astype(np.float64))


def sadf(y, end_idxs, min_len, max_len, step=1, lags=1, trend="c", dtype=np.longdouble):
    """-> dict: stat (float64), start (int64), n_skipped, lengths (the window lengths m), table (end points x lengths: every ADF(s, t)
    in `dtype`, NaN where the window does not exist, is degenerate or holds a NaN), runner_up (the second largest statistic of the end
    point, NaN without one), min_pivot (the smallest relative pivot of its windows that lies above the band), min_fit (the smallest
    SSR / sum dy^2 above the band), band (how many of its windows have a pivot or a fit INSIDE [2^-32, 2^-20])."""
    dtype = np.dtype(dtype).type
    y64 = np.asarray(y, dtype=np.float64)
    n = len(y64)
    with np.errstate(invalid="ignore"):
        yv = np.where(np.isfinite(y64), y64, np.nan).astype(dtype)
    t = np.arange(n, dtype=np.int64) if end_idxs is None else np.asarray(end_idxs, dtype=np.int64).reshape(-1)
    E, L, ct = len(t), lags, TRENDS[trend]
    k = regressors(lags, trend)
    assert 0 <= lags <= 4 and min_len >= k + 1 and max_len >= min_len and step >= 1 and (E == 0 or (t.min() >= 0 and t.max() < n))
    lengths = np.arange(min_len, max_len + 1, step, dtype=np.int64)
    lengths = lengths[lengths <= (int(t.max()) - L if E else 0)]
    table = np.full((E, len(lengths)), np.nan, dtype)
    min_pivot, min_fit, band = np.full(E, np.inf), np.full(E, np.inf), np.zeros(E, np.int64)
    # column numbers in the factor: 1, (tau), the lagged differences, the level; the target is row / column k
    col = {0: k, L + 1: k - 1}
    col.update({q: (2 if ct else 1) + q - 1 for q in range(1, L + 1)})
    S = {}                                               # the running moments that are sums of data
    yt = yv[t] if E else yv[:0]
    pos = {int(m): c for c, m in enumerate(lengths)}
    for m in range(1, (int(lengths[-1]) if len(lengths) else 0) + 1):
        i = t - (m - 1)
        ok = i >= L + 1                                  # the row exists (and so did every earlier one)
        ii = np.where(ok, i, L + 1)
        with np.errstate(invalid="ignore"):
            v = [yv[ii - q] for q in range(L + 2)]
            u = [v[q] - v[q + 1] for q in range(L + 1)] + [v[1] - yt]
            u = [np.where(ok, x, dtype(0)) for x in u]
            tau = (i - t).astype(dtype)
            for p in range(L + 2):
                cp = col[p]
                S[(cp, 0)] = S.get((cp, 0), 0) + u[p]
                if ct:
                    S[(cp, 1)] = S.get((cp, 1), 0) + tau * u[p]
                for q in range(p, L + 2):
                    key = (max(cp, col[q]), min(cp, col[q]))
                    S[key] = S.get(key, 0) + u[p] * u[q]
        if m not in pos:
            continue
        mm = dtype(m)
        A = [[None] * (k + 1) for _ in range(k + 1)]
        A[0][0] = np.full(E, mm)
        if ct:
            A[1][0] = np.full(E, -(mm * (mm - 1)) / 2)
            A[1][1] = np.full(E, (mm - 1) * mm * (2 * mm - 1) / 6)
        for (r, c), val in S.items():
            A[r][c] = val.copy()
        stat, degenerate, rel, in_band, ratio = _solve(A, k, m, dtype)
        table[:, pos[m]] = np.where(ok, stat, dtype(np.nan))
        live = ok & ~degenerate & ~np.isnan(stat)
        with np.errstate(invalid="ignore"):
            fit_band = live & (ratio >= BAND_LOW) & (ratio <= BAND_HIGH)
            min_fit = np.where(live & (ratio > BAND_HIGH), np.minimum(min_fit, ratio), min_fit)
        min_pivot = np.where(ok, np.minimum(min_pivot, rel), min_pivot)
        band += (ok & in_band) | fit_band
    stat = np.full(E, np.nan)
    start = np.full(E, -1, np.int64)
    runner_up = np.full(E, np.nan)
    if len(lengths) and E:
        with np.errstate(invalid="ignore"):
            filled = np.where(np.isnan(table), dtype(-np.inf), table)
            have = ~np.isnan(table).all(axis=1)
            best = filled.argmax(axis=1)                 # the first, i.e. the shortest, among equals
            rows = np.arange(E)
            lowest = have & np.isneginf(filled[rows, best])          # nothing above -inf: the first window that HAS a statistic
            best[lowest] = (~np.isnan(table)).argmax(axis=1)[lowest]
            rows = np.arange(E)
            stat[have] = table[rows, best][have].astype(np.float64)
            start[have] = (t - lengths[best] + 1)[have]
            rest = filled.copy()
            rest[rows, best] = -np.inf
            second = rest.max(axis=1)
            counts = (~np.isnan(table)).sum(axis=1)
            runner_up[counts >= 2] = second[counts >= 2].astype(np.float64)
    return {"stat": stat, "start": start, "n_skipped": int(np.isnan(stat).sum()) if E else 0, "lengths": lengths, "table": table,
            "runner_up": runner_up, "min_pivot": min_pivot, "min_fit": min_fit, "band": band, "end": t}


def lstsq_adf(y, s, t, lags, trend):
    """ADF(s, t) the plain way: numpy.linalg.lstsq on UNCENTRED regressors [y_{i-1}, dy_{i-1}, .., dy_{i-L}, 1, (i if "ct")] ->
    the t-statistic of the first coefficient, in float64."""
    y = np.asarray(y, dtype=np.float64)
    i = np.arange(s, t + 1)
    dy = lambda j: y[j] - y[j - 1]
    X = [y[i - 1]] + [dy(i - q) for q in range(1, lags + 1)] + [np.ones(len(i))] + ([i.astype(np.float64)] if trend == "ct" else [])
    X = np.column_stack(X)
    b, *_ = np.linalg.lstsq(X, dy(i), rcond=None)
    res = dy(i) - X @ b
    sigma2 = res @ res / (len(i) - X.shape[1])
    cov = sigma2 * np.linalg.inv(X.T @ X)
    return b[0] / np.sqrt(cov[0, 0])


def relative_error(y, end_idxs, min_len, max_len, step, lags, trend, ref=None):
    """The float64 restatement against the longdouble one on one input -> (largest |difference| / max(1, |stat|) over the finite
    statistics of the whole TABLE, how many were compared, end points whose start moved)."""
    ref = sadf(y, end_idxs, min_len, max_len, step, lags, trend) if ref is None else ref
    got = sadf(y, end_idxs, min_len, max_len, step, lags, trend, np.float64)
    a, b = ref["table"], got["table"]
    both = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
    err = float((np.abs(a[both] - b[both]) / np.maximum(1, np.abs(a[both]))).max()) if both.any() else 0.0
    return err, int(both.sum()), int((ref["start"] != got["start"]).sum())
