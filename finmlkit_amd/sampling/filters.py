"""Drop-in for finmlkit/sampling/filters.py: the symmetric CUSUM event filter walks the series on the MI355X
(csrc/fmk_cusum_filter.h).  No CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.typing import NDArray

from .. import _ffi
from .._ffi import c_i64, ptr


def check_arguments(n, n_threshold):
    """The argument checks of filters.py:29-32, in the reference's order and with its messages (no device is touched)."""
    if n <= 1:
        raise ValueError("Input time series must have at least 2 elements.")
    if n_threshold != 1 and n_threshold != n:
        raise ValueError("Threshold array must either contain 1 const. element or len(raw_time_series) elements.")


def cusum_filter(raw_time_series: NDArray[np.float64], threshold: NDArray) -> NDArray[np.int64]:
    """Reference: finmlkit/sampling/filters.py:7-70 -> indices into `raw_time_series` at which an event fires, bit for bit.
    `threshold` holds one element (a constant) or len(raw_time_series) elements."""
    check_arguments(len(raw_time_series), len(threshold))
    x = np.ascontiguousarray(raw_time_series, dtype=np.float64)
    thr = np.ascontiguousarray(threshold, dtype=np.float64)
    out = np.empty(len(x) - 1, np.int64)
    m = c_i64()
    _ffi.default_context().call("fmk_cusum_filter", ptr(x), c_i64(len(x)), ptr(thr), c_i64(len(thr)), ptr(out), c_i64(len(out)),
                                C.byref(m))
    return out[:m.value].copy()


def z_score_peak_filter(y: NDArray[np.float64], window: int, threshold: float = 3) -> NDArray[np.int64]:
    """Reference: finmlkit/sampling/filters.py:73-94, which is not implemented there either."""
    raise NotImplementedError("This function is not yet implemented.")
