"""Drop-in for finmlkit/feature/core/momentum.py::roc and ::stoch_k, computed on the MI355X (csrc/fmk_order.hip).  The other
indicators of that module (rsi_wilder and the rest) are one serial chain over the whole series and out of scope."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import c_i64, ptr
from .ma import series_call

PERIOD_MESSAGE = "roc: period must not be negative."
LENGTH_MESSAGE = "stoch_k: length must be at least 1."
SHAPE_MESSAGE = "stoch_k: close, low and high must have the same length."


def roc(price: NDArray, period: int) -> NDArray:
    """Reference: finmlkit/feature/core/momentum.py:6-22: ((price[i] - price[i - period]) / price[i - period]) * 100, NaN before
    `period`; a zero divisor gives the IEEE result."""
    return series_call("fmk_roc", price, period, least=0, message=PERIOD_MESSAGE)


def stoch_k(close: NDArray[np.float64], low: NDArray[np.float64], high: NDArray[np.float64], length: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/momentum.py:68-112: (100 * (close[t] - lo)) / (hi - lo) with lo / hi the minimum of `low` /
    maximum of `high` over the `length` bars ending at t, NaN where hi <= lo, where the window holds a NaN in `low` or `high`, and
    before the first full window."""
    if int(length) < 1:
        raise ValueError(LENGTH_MESSAGE)
    c, lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (close, low, high))
    if not (c.ndim == lo.ndim == hi.ndim == 1 and len(c) == len(lo) == len(hi)):
        raise ValueError(SHAPE_MESSAGE)
    out = np.empty(len(c), np.float64)
    if len(c):
        _ffi.default_context().call("fmk_stoch_k", ptr(c), ptr(lo), ptr(hi), c_i64(len(c)), c_i64(int(length)), ptr(out))
    return out
