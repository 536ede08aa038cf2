"""Drop-in for finmlkit/feature/core/reversion.py::vwap_distance, computed on the MI355X (csrc/fmk_runsum.hip)."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ..series_ops import OPS, VWAP_PERIODS_MESSAGE as PERIODS_MESSAGE, VWAP_SHAPE_MESSAGE as SHAPE_MESSAGE, host  # noqa: F401


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
    return host(OPS["vwap_distance"], (close, volume), n_periods, is_log)
