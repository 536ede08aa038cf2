"""Drop-in for finmlkit/feature/core/ma.py::sma (csrc/fmk_rolling.hip) and ::ewma (csrc/fmk_recur.hip), computed on the MI355X."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import c_f64, c_i64, ptr

WINDOW_MESSAGE = "window must be at least 1."
SPAN_MESSAGE = "span size is less than or equal to 1. Please provide a span size greater than 1."


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


def ewma(y: NDArray, span: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/ma.py:6-43: pandas' `ewm(span=span).mean()` with adjust=True, u = y[t] + (1 - alpha) * u and
    v = 1 + (1 - alpha) * v with alpha = 2 / (span + 1), out = u / v; NaN from the first NaN of `y` on.  `span < 1` raises
    ValueError with the reference's message.  An empty series gives an empty array (the reference raises IndexError there).
    A device-wide scan: the outputs agree with the reference to a few units in the last place (1e-9 relative is the contract),
    NaN positions and exact zeros exactly.  Outside the contract: infinite inputs, and a numerator that has decayed below 2^-969 over
    a run of zeros in `y` until the next non-zero one (the reference stalls at the smallest subnormals for 1 - alpha >= 2 / 3 and
    reaches 0.0 below, the scan's composed state underflows to 0.0)."""
    if not float(span) >= 1.0:
        raise ValueError(SPAN_MESSAGE)
    yy = np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty(len(yy), np.float64)
    if len(yy):
        _ffi.default_context().call("fmk_ewma", ptr(yy), c_i64(len(yy)), c_f64(float(span)), ptr(out))
    return out
