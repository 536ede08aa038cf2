"""Drop-in for finmlkit/feature/core/utils.py::comp_lagged_returns, ::comp_zscore, ::comp_burst_ratio and ::pct_change, computed on
the MI355X."""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import c_f64, c_i64, ptr
from ..series_ops import OPS, PCT_PERIODS_MESSAGE as PERIODS_MESSAGE, host  # noqa: F401 -- the message is part of this module's interface


def comp_lagged_returns(timestamps: NDArray[np.int64], close: NDArray[np.float64], return_window_sec: float,
                        is_log: bool) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/utils.py:12-64 (float64 key comparison semantics included)."""
    if return_window_sec <= 0:
        raise ValueError("The return window must be greater than zero.")
    ctx = _ffi.default_context()
    ts = np.ascontiguousarray(timestamps, dtype=np.int64)
    c = np.ascontiguousarray(close, dtype=np.float64)
    out = np.empty(len(c), np.float64)
    ctx.call("fmk_comp_lagged_returns", ptr(ts), ptr(c), c_i64(len(c)), c_f64(return_window_sec),
             C.c_int(bool(is_log)), ptr(out))
    return out


def comp_zscore(x: NDArray[np.float64], window: int, ddof: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/utils.py:67-90: (x[i] - mean) / std of the window ending at i, mean and the squared deviations
    summed left to right, NaN where std == 0 and before the first full window.  `window - ddof <= 0` raises ValueError (the
    reference divides by zero or takes the root of a negative number there)."""
    return host(OPS["zscore"], (x,), window, ddof)


def comp_burst_ratio(series: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/utils.py:92-108: series[i] / np.median(the window ending at i) where that median is > 0,
    NaN elsewhere, where the window holds a NaN, and before the first full window (csrc/fmk_order.hip)."""
    return host(OPS["burst_ratio"], (series,), window)


def pct_change(x: NDArray[np.float64], periods: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/utils.py:110-124: (x[t] - base) / base with base = x[t - periods] where base > 0, NaN
    elsewhere and before `periods`."""
    return host(OPS["pct_change"], (x,), periods)
