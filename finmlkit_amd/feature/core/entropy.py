"""Rolling approximate entropy of a float64 series, computed on the MI355X (csrc/fmk_entropy.hip): what the reference's
ApproximateEntropy transform (finmlkit/feature/transforms.py:1400-1457) computes with pandas' rolling.apply around
`antropy.app_entropy(x, order=m, metric="chebyshev", tolerance=tolerance * std(x))`.  No `antropy` is needed here: the contract is
that function's published algorithm, within the tolerance recorded in tests/golden/entropy.json, NaN positions exactly (DESIGN.md
section 7c4).  Every window is an all-pairs problem of its own, O(n * window^2)."""
from __future__ import annotations

import numpy as np
from numpy.typing import NDArray

from ..series_ops import (APEN_M_MESSAGE, APEN_MAX_M, APEN_MAX_M_MESSAGE, APEN_MAX_WINDOW, APEN_MAX_WINDOW_MESSAGE,  # noqa: F401
                          APEN_TOLERANCE_MESSAGE, APEN_WINDOW_MESSAGE, OPS, host, rule_approximate_entropy as check_arguments)


def approximate_entropy(x: NDArray[np.float64], window: int, m: int = 2, tolerance: float = 0.2) -> NDArray[np.float64]:
    """Approximate entropy of x[t-window+1 .. t]: with `r = tolerance * std(window)` (population standard deviation) and, for k in
    (m, m + 1), `C_k[i]` the number of the `N_k = window - k + 1` vectors `(x_j .. x_{j+k-1})` within Chebyshev distance r of
    vector i (inclusive, itself counted), `phi_k = mean(ln(C_k / N_k))` and the output is `phi_m - phi_{m+1}`; it can be negative.
    NaN before the first full window and in every window that reads a NaN or an infinity; exactly 0.0 where every pair matches (a
    constant window).  `tolerance = 0` is legal: only equal values match.  ValueError for `m < 1`, `m > 4`, `window < m + 1`,
    `window > 1024` and a tolerance that is negative, NaN or infinite."""
    return host(OPS["approximate_entropy"], (x,), window, m, tolerance)
