"""Drop-in for finmlkit/feature/core/correlation.py::rolling_price_volume_correlation, computed on the MI355X (csrc/fmk_corr.hip)."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ..series_ops import CORR_SHAPE_MESSAGE as SHAPE_MESSAGE, OPS, WINDOW_MESSAGE, host  # noqa: F401


def rolling_price_volume_correlation(price: NDArray[np.float64], volume: NDArray[np.float64], window: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/correlation.py:10-111: the rolling Pearson correlation of the one-step price returns
    (`(price[i] - price[i-1]) / price[i-1]`, NaN at 0, at a NaN price and over a zero price) and the volumes.  NaN before `window`
    (one output later than `sma`; everywhere when `window >= n`) and where the current return or volume is NaN.  Otherwise the
    pairs of the window without a NaN, in index order: fewer than two give NaN; the means of left-to-right sums, then
    `cov / (sqrt(qr) * sqrt(qv))` of the left-to-right sums of the deviation products where `qr > 0` and `qv > 0`, clamped to
    [-1, 1]; NaN otherwise (constant returns or volumes, an infinity in the sums).  For `4 <= t < 10` the reference's special
    case comes first: strictly rising prices with strictly rising volumes over the window give 1.0, with strictly falling volumes
    -1.0 (a NaN inside fails no comparison; `window = 1` compares nothing).  Every window is recomputed in the reference's order:
    bit for bit the reference, NaN positions included (Python's `sum` as a plain left-to-right sum, what
    it is before 3.12 and what Numba compiles).  Departures, where the reference is undefined: `window < 1` (it indexes from the
    end of the arrays) and unequal lengths (IndexError, or a short read) raise ValueError; an empty series returns an empty array
    (the reference raises IndexError)."""
    return host(OPS["price_volume_corr"], (price, volume), window)
