"""The augmented Dickey-Fuller statistic of backward windows and its supremum, SADF (Lopez de Prado, Advances in Financial Machine
Learning, ch. 17; Phillips, Wu and Yu), every (end point, start point) regression run on the MI355X (csrc/fmk_sadf.hip).  No CPU
fallback.  The reference has no such function; the definition is this project's (include/fmk.h):

    row i of end point t:  dy_i  on  1, (i - t if trend == "ct"), dy_{i-1}, .., dy_{i-lags}, y_{i-1} - y_t        (i >= lags + 1)
    ADF(s, t) = the t-statistic of the last coefficient over the rows i in [s, t];  SADF_t = max over the window lengths
    m = t - s + 1 in {min_len, min_len + step, ..}, m <= max_len, s >= lags + 1: the shortest window among equals.

`y` is taken as given: pass log prices for the book's test.  A degenerate window (a constant stretch, collinear columns) and a window
that holds a NaN or an infinity are never chosen; an exact fit gives +-inf; an end point without a usable window gives NaN and a
start of -1."""
from __future__ import annotations

import ctypes as C
import operator
from typing import Optional, Tuple

import numpy as np
from numpy.typing import NDArray

from .... import _ffi
from ...._ffi import DeviceArray, c_i64, ptr

MAX_LAGS = 4                         # csrc/fmk_common.h: FMK_ADF_MAX_LAGS
TRENDS = {"c": 0, "ct": 1}           # include/fmk.h: FMK_ADF_C, FMK_ADF_CT
INTEGER_MESSAGE = "sadf: min_len, max_len, step and lags must be integers."
LAGS_MESSAGE = "sadf: lags must be between 0 and 4."
TREND_MESSAGE = 'sadf: trend must be "c" or "ct".'
MAX_LEN_MESSAGE = "sadf: max_len must not be less than min_len."
STEP_MESSAGE = "sadf: step must be at least 1."
END_IDXS_MESSAGE = "sadf: end_idxs must be a one-dimensional integer array."


def regressors(lags: int, trend: str) -> int:
    """k: the level, the lagged differences, the intercept and, for "ct", the time trend."""
    return lags + 2 + TRENDS[trend]


def check_arguments(n, end_idxs, min_len, max_len, lags, trend, step):
    """What the library refuses (FMK_E_ARG), asked on the host in the library's order before anything reaches a device ->
    (min_len, max_len, lags, trend code, step) as ints.  max_len None: all history.  end_idxs: the host array of end points, or
    None when every element is one or when they are resident and the library checks them."""
    try:
        min_len, step, lags = operator.index(min_len), operator.index(step), operator.index(lags)
        max_len = max(min_len, int(n)) if max_len is None else operator.index(max_len)
    except TypeError:
        raise ValueError(INTEGER_MESSAGE) from None
    if not 0 <= lags <= MAX_LAGS:
        raise ValueError(LAGS_MESSAGE)
    if not isinstance(trend, str) or trend not in TRENDS:
        raise ValueError(TREND_MESSAGE)
    k = regressors(lags, trend)
    if min_len < k + 1:
        raise ValueError(f"sadf: min_len must be at least {k + 1} (one more than the {k} regressors).")
    if max_len < min_len:
        raise ValueError(MAX_LEN_MESSAGE)
    if step < 1:
        raise ValueError(STEP_MESSAGE)
    if end_idxs is not None and len(end_idxs):
        ev = np.asarray(end_idxs)
        if ev.ndim != 1 or ev.dtype.kind not in "iu":
            raise ValueError(END_IDXS_MESSAGE)
        bad = int(np.count_nonzero((ev < 0) | (ev >= n)))
        if bad:
            raise ValueError(f"sadf: {bad} end points outside [0, {n})")
    return min_len, max_len, lags, TRENDS[trend], step


def sadf(y, min_len: int, max_len: Optional[int] = None, lags: int = 1, trend: str = "c", step: int = 1, end_idxs=None
         ) -> Tuple[NDArray[np.float64], NDArray[np.int64]]:
    """-> (stat, start): per end point the supremum ADF statistic and the first row `s` of the window that attains it (-1 and NaN
    where no window of at least `min_len` rows exists, e.g. at the first elements, or none is usable).  max_len None: all history.
    end_idxs None: every element is an end point; otherwise any integer array of indices, duplicates and any order allowed.
    ValueError: lags outside 0..4, an unknown trend, min_len < k + 1 (k = lags + 2, + 1 for "ct"), max_len < min_len, step < 1,
    an end point outside the series."""
    x = np.ascontiguousarray(y, dtype=np.float64)
    ev = None
    if end_idxs is not None:
        ev = np.asarray(end_idxs)
        if ev.size == 0:
            ev = ev.astype(np.int64).reshape(-1)
    min_len, max_len, lags, code, step = check_arguments(len(x), ev, min_len, max_len, lags, trend, step)
    ne = len(x) if ev is None else len(ev)
    stat, start = np.empty(ne, np.float64), np.empty(ne, np.int64)
    if ne == 0:
        return stat, start
    if ev is not None:
        ev = np.ascontiguousarray(ev, dtype=np.int64)
    _ffi.default_context().call("fmk_sadf", ptr(x), c_i64(len(x)), ptr(ev), c_i64(ne), c_i64(min_len), c_i64(max_len), c_i64(step),
                                c_i64(lags), C.c_int(code), ptr(stat), ptr(start), None)
    return stat, start


def adf_rolling(y, window: int, lags: int = 1, trend: str = "c") -> NDArray[np.float64]:
    """The ADF statistic of the `window` rows that end at every element: `sadf` with min_len == max_len == window."""
    return sadf(y, window, window, lags, trend)[0]


def adf_stat(y, lags: int = 1, trend: str = "c") -> float:
    """The ADF statistic of the whole series: its len(y) - lags - 1 rows as one window that ends at the last element.  ValueError
    when that is fewer than k + 1 rows."""
    x = np.ascontiguousarray(y, dtype=np.float64)
    rows = len(x) - operator.index(lags) - 1
    min_len, max_len, lags, code, _ = check_arguments(len(x), None, max(rows, 0), max(rows, 0), lags, trend, 1)
    return float(sadf(x, min_len, max_len, lags, trend, 1, np.array([len(x) - 1], np.int64))[0][0])


def resident(ctx, y: DeviceArray, end_idx: Optional[DeviceArray], min_len, max_len, lags, trend, step):
    """fmk_sadf_dev on a DeviceArray -> (stat float64, start int64, n_skipped int64[1]) DeviceArrays.  Rules and dtypes are checked,
    in this order, before `ctx` or a pointer is looked at; without an end point the library is not called."""
    min_len, max_len, lags, code, step = check_arguments(y.n, None, min_len, max_len, lags, trend, step)
    if y.dtype != np.float64:
        raise TypeError(f"fmk_sadf_dev: the series must be float64, not {y.dtype}")
    if end_idx is not None and end_idx.dtype != np.int64:
        raise TypeError(f"fmk_sadf_dev: the end points must be int64, not {end_idx.dtype}")
    ne = y.n if end_idx is None else end_idx.n
    stat, start, skipped = DeviceArray(ctx, ne, np.float64), DeviceArray(ctx, ne, np.int64), DeviceArray(ctx, 1, np.int64)
    skipped.zero()
    if ne:
        ctx.call("fmk_sadf_dev", y.p, c_i64(y.n), None if end_idx is None else end_idx.p, c_i64(ne), c_i64(min_len), c_i64(max_len),
                 c_i64(step), c_i64(lags), C.c_int(code), stat.p, start.p, skipped.p)
    return stat, start, skipped
