"""Drop-in for finmlkit/feature/core/reversion.py::vwap_distance, computed on the MI355X (csrc/fmk_runsum.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import c_i64, ptr

PERIODS_MESSAGE = "vwap_distance: n_periods must be at least 1."
SHAPE_MESSAGE = "vwap_distance: close and volume must have the same length."


def vwap_distance(close: NDArray[np.float64], volume: NDArray[np.float64], n_periods: int, is_log: bool) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/reversion.py:9-56: close / vwap - 1.0 (with `is_log`: log(close / vwap), the host's log; the
    first window is the simple form in either mode, as in the reference) with vwap = wsum / vsum from the reference's running sums
    over `n_periods` (wsum += close[i] * volume[i] - close[i-n_periods] * volume[i-n_periods]).  Where vsum > 0 is false -- a NaN
    vsum included -- the output is the one before it; NaN before n_periods - 1, until the first window with volume, and
    everywhere when the series is shorter than n_periods.  `n_periods < 1` (the reference reads uninitialised memory there) and
    unequal lengths raise ValueError.  A device-wide scan with the coefficient 1 and a hold launch after it: bit for bit the
    reference on exactly summable inputs, NaN positions and which outputs are held included; otherwise within a few units in the
    last place of the largest running sum.  Outside the contract: infinite inputs, and on inputs that are not
    exactly summable whether a window of all-zero volumes holds (the reference's vsum there is a residue, not 0)."""
    if int(n_periods) < 1:
        raise ValueError(PERIODS_MESSAGE)
    c, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (close, volume))
    if not (c.ndim == v.ndim == 1 and len(c) == len(v)):
        raise ValueError(SHAPE_MESSAGE)
    out = np.empty(len(c), np.float64)
    if len(c):
        _ffi.default_context().call("fmk_vwap_distance", ptr(c), ptr(v), c_i64(len(c)), c_i64(int(n_periods)), C.c_int(bool(is_log)),
                                    ptr(out))
    return out
