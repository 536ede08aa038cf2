"""The window statistics that finmlkit/feature/transforms.py computes itself -- KurtosisTransform (:900-933), TrendSlope (:936-988),
HurstExponent (:1341-1397) and BiPowerVariation (:1551-1602) -- as functions of a float64 series, computed on the MI355X
(csrc/fmk_shape.hip).  Every window is recomputed on its own; a window that reads a NaN or an infinity gives NaN (pandas' rolling
turns +-inf into NaN and wants a full window).  The reference's values within the tolerances recorded in tests/golden/shape.json, its
NaN positions exactly.  Departure: `window < 1` raises ValueError (the reference returns all NaN or zeros)."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ..series_ops import HURST_MIN_WINDOW, HURST_WINDOW_MESSAGE, OPS, WINDOW_MESSAGE, host  # noqa: F401 -- part of this module's interface


def rolling_kurtosis(x: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """Excess kurtosis of x[t-window+1 .. t] in scipy's biased Fisher form: `m4 / (m2 * m2) - 3` of the central moments about the
    window's mean.  NaN before the first full window and where `m2 == 0` (every window at `window = 1`)."""
    return host(OPS["rolling_kurtosis"], (x,), window)


def trend_slope(x: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """The least-squares slope of `ln x` over t-window+1 .. t on the positions 0 .. window-1, as an angle in degrees:
    `atan(slope) * 180 / pi`.  NaN before the first full window, where a price of the window is not finite and > 0, and at
    `window = 1`."""
    return host(OPS["trend_slope"], (x,), window)


def hurst_exponent(x: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """The aggregated-variance Hurst exponent of x[t-window+1 .. t]: with tau_k the population standard deviation of the sums of k
    consecutive elements after the window's first, k = 1, 2, 4, 8, the least-squares slope of `ln tau_k` on `ln k`; NaN where a
    tau_k is not > 0 (every window at `window = 9`) and where an element of the window, the first included, is not finite.
    `window < 9` raises ValueError (the reference raises TypeError out of polyfit)."""
    return host(OPS["hurst_exponent"], (x,), window)


def bipower_variation(x: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """`sqrt(pi / 2) * sum(|x[j]| * |x[j-1]|, j = t-window+1 .. t)`: `window` products over the window + 1 elements x[t-window .. t],
    so the first output is at `t = window`, one later than the other three."""
    return host(OPS["bipower_variation"], (x,), window)
