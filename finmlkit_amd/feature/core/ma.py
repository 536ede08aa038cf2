"""Drop-in for finmlkit/feature/core/ma.py::sma, computed on the MI355X (csrc/fmk_rolling.hip)."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import c_i64, ptr

WINDOW_MESSAGE = "window must be at least 1."


def series_call(name: str, x, arg: int, *extra, least: int = 1, message: str = WINDOW_MESSAGE) -> NDArray[np.float64]:
    """One of the one-series host-pointer entries of csrc/fmk_rolling.hip and csrc/fmk_order.hip on `x` -> float64 array of len(x).
    The check of `arg` (a window, a lag) comes first: no device is needed to refuse a call, nor to answer an empty series."""
    if int(arg) < least:
        raise ValueError(message)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(len(xx), np.float64)
    if len(xx):
        _ffi.default_context().call(name, ptr(xx), c_i64(len(xx)), c_i64(int(arg)), *extra, ptr(out))
    return out


def sma(array: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/ma.py:46-62: (1.0 / window) * (the window's sum, added left to right), NaN before the first
    full window."""
    return series_call("fmk_sma", array, window)
