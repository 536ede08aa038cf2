"""Drop-in for finmlkit/feature/core/structural_break/cusum.py: the Chu-Stinchcombe-White CUSUM test on levels, every (t, n) pair
evaluated on the MI355X (csrc/fmk_break.hip).  No CPU fallback.  All four outputs are bit for bit what the reference's code gives with the
host's log() as its np.log (what it has when Numba compiles it; interpreted NumPy's own log differs in the last bit on a few
arguments in a thousand), NaN positions included.  Two deliberate deviations: `warmup_period < 2` raises ValueError, and so does `cusum_test_last` on fewer than 3
elements -- the reference divides by zero or reads `cum_squared_diff[-1]` there."""
from __future__ import annotations

from typing import Tuple

import numpy as np
from numpy.typing import NDArray

from .... import _ffi
from ...._ffi import c_i64, ptr

Four = Tuple[NDArray[np.float64], NDArray[np.float64], NDArray[np.float64], NDArray[np.float64]]


def check_warmup(warmup_period):
    if warmup_period < 2:
        raise ValueError("warmup_period must be at least 2.")


def _call(name, x, *args) -> Four:
    out = [np.empty(len(x), np.float64) for _ in range(4)]
    if len(x):
        _ffi.default_context().call(name, ptr(x), c_i64(len(x)), *args, *[ptr(o) for o in out])
    return tuple(out)


def cusum_test_developing(y: NDArray, warmup_period: int = 30) -> Four:
    """Reference: cusum.py:69-133.  `y`: prices (the logarithm is taken here); every output looks back to element 0; outputs below
    `warmup_period` are NaN.  Nothing is checked: log of 0 or of a negative number flows through as -inf or NaN."""
    check_warmup(warmup_period)
    x = np.ascontiguousarray(y, dtype=np.float64)
    return _call("fmk_cusum_test_developing", x, c_i64(int(warmup_period)))


def cusum_test_last(y: NDArray) -> Tuple[float, float, float, float]:
    """Reference: cusum.py:136-176: the test for the last element alone, looking back to element 0, as four floats."""
    x = np.ascontiguousarray(y, dtype=np.float64)
    if len(x) < 3:
        raise ValueError("cusum_test_last needs at least 3 elements.")
    return tuple(float(o[-1]) for o in _call("fmk_cusum_test_developing", x, c_i64(len(x) - 1)))


def cusum_test_rolling(close_prices: NDArray, window_size: int = 1000, warmup_period: int = 30) -> Four:
    """Reference: cusum.py:179-274.  Output t looks back to max(0, t - window_size); `window_size` is raised to
    `warmup_period + 2`; all-NaN when there are fewer than `warmup_period + 2` prices.  ValueError when a price is <= 0."""
    check_warmup(warmup_period)
    x = np.ascontiguousarray(close_prices, dtype=np.float64)
    if np.any(x <= 0):
        raise ValueError("All close prices must be positive.")
    return _call("fmk_cusum_test_rolling", x, c_i64(max(0, int(window_size))), c_i64(int(warmup_period)))
