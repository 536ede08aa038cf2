"""Drop-in for finmlkit/feature/core/ma.py::sma (csrc/fmk_rolling.hip) and ::ewma (csrc/fmk_recur.hip), computed on the MI355X."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ..series_ops import OPS, SPAN_MESSAGE, WINDOW_MESSAGE, host  # noqa: F401 -- the messages are part of this module's interface


def sma(array: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/ma.py:46-62: (1.0 / window) * (the window's sum, added left to right), NaN before the first
    full window."""
    return host(OPS["sma"], (array,), window)


def ewma(y: NDArray, span: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/ma.py:6-43: pandas' `ewm(span=span).mean()` with adjust=True, u = y[t] + (1 - alpha) * u and
    v = 1 + (1 - alpha) * v with alpha = 2 / (span + 1), out = u / v; NaN from the first NaN of `y` on.  `span < 1` raises
    ValueError with the reference's message.  An empty series gives an empty array (the reference raises IndexError there).
    A device-wide scan: the outputs agree with the reference to a few units in the last place (1e-9 relative is the contract),
    NaN positions and exact zeros exactly.  Outside the contract: infinite inputs, and a numerator that has decayed below 2^-969 over
    a run of zeros in `y` until the next non-zero one (the reference stalls at the smallest subnormals for 1 - alpha >= 2 / 3 and
    reaches 0.0 below, the scan's composed state underflows to 0.0)."""
    return host(OPS["ewma"], (y,), span)
