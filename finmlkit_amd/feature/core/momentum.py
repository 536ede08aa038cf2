"""Drop-in for finmlkit/feature/core/momentum.py::roc and ::stoch_k (csrc/fmk_order.hip) and ::rsi_wilder (a device-wide scan of
Wilder's recurrence, csrc/fmk_recur.hip), computed on the MI355X."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ..series_ops import OPS, host
from ..series_ops import (ROC_PERIOD_MESSAGE as PERIOD_MESSAGE, RSI_WINDOW_MESSAGE, STOCH_LENGTH_MESSAGE as LENGTH_MESSAGE,  # noqa: F401
                          STOCH_SHAPE_MESSAGE as SHAPE_MESSAGE)


def roc(price: NDArray, period: int) -> NDArray:
    """Reference: finmlkit/feature/core/momentum.py:6-22: ((price[i] - price[i - period]) / price[i - period]) * 100, NaN before
    `period`; a zero divisor gives the IEEE result."""
    return host(OPS["roc"], (price,), period)


def stoch_k(close: NDArray[np.float64], low: NDArray[np.float64], high: NDArray[np.float64], length: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/momentum.py:68-112: (100 * (close[t] - lo)) / (hi - lo) with lo / hi the minimum of `low` /
    maximum of `high` over the `length` bars ending at t, NaN where hi <= lo, where the window holds a NaN in `low` or `high`, and
    before the first full window."""
    return host(OPS["stoch_k"], (close, low, high), length)


def rsi_wilder(close: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/momentum.py:25-65: the gains and losses of close[1 .. window] averaged, then Wilder's
    avg = ((window - 1) * avg + x) / window; 100 - 100 / (1 + gain / loss) where loss > 0, NaN otherwise, before `window`, and
    everywhere when a difference of the first window is NaN (a later NaN difference counts as no gain and no loss).
    `window < 1` raises ValueError (the reference divides by zero there).  A device-wide scan: the outputs agree with the
    reference within 1e-7 absolute on the 0-100 scale, NaN positions exactly.  Outside the contract: infinite prices, and an
    average that has decayed below 2^-969 (969, 1 657, 9 063 bars without a gain or without a loss at windows 2, 3, 14) until both
    averages have taken a non-zero term again: there the reference stalls at the smallest subnormal for windows of 3 and more (and
    reads 50.0, 0.0 or 100.0 off it for good) and reaches 0.0 at windows 1 and 2 (NaN), while the scan's composed state underflows to
    0.0 at every window (NaN until the next loss).  tests/test_gpu_recur_runs.py pins both sides of that line."""
    return host(OPS["rsi_wilder"], (close,), window)
