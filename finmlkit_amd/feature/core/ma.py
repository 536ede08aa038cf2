"""Drop-in for finmlkit/feature/core/ma.py::sma, computed on the MI355X (csrc/fmk_rolling.hip)."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import c_i64, ptr

WINDOW_MESSAGE = "window must be at least 1."


def rolling_call(name: str, x, window: int, *extra) -> NDArray[np.float64]:
    """One of the host-pointer entries of csrc/fmk_rolling.hip on `x` -> float64 array of len(x).  The window check comes first:
    no device is needed to refuse a call, nor to answer an empty series."""
    if int(window) < 1:
        raise ValueError(WINDOW_MESSAGE)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(len(xx), np.float64)
    if len(xx):
        _ffi.default_context().call(name, ptr(xx), c_i64(len(xx)), c_i64(int(window)), *extra, ptr(out))
    return out


def sma(array: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/ma.py:46-62: (1.0 / window) * (the window's sum, added left to right), NaN before the first
    full window."""
    return rolling_call("fmk_sma", array, window)
