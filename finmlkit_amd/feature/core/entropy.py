"""Rolling approximate entropy of a float64 series, computed on the MI355X (csrc/fmk_entropy.hip): what the reference's
ApproximateEntropy transform (finmlkit/feature/transforms.py:1400-1457) computes with pandas' rolling.apply around
`antropy.app_entropy(x, order=m, metric="chebyshev", tolerance=tolerance * std(x))`.  No `antropy` is needed here: the contract is
that function's published algorithm, within the tolerance recorded in tests/golden/entropy.json, NaN positions exactly (DESIGN.md
section 7c4).  Every window is an all-pairs problem of its own, O(n * window^2)."""
from __future__ import annotations

import math

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import c_f64, c_i64, ptr

APEN_MAX_M = 4                       # the kernels are instantiated per m (csrc/fmk_common.h: FMK_APEN_MAX_M)
APEN_MAX_WINDOW = 1024               # one tile's span and the table of logarithms fit in LDS (FMK_APEN_MAX_WINDOW)
APEN_M_MESSAGE = "approximate_entropy: m must be at least 1."
APEN_MAX_M_MESSAGE = "approximate_entropy: m must be at most 4."
APEN_WINDOW_MESSAGE = "approximate_entropy: window must be at least m + 1."
APEN_MAX_WINDOW_MESSAGE = "approximate_entropy: window must be at most 1024."
APEN_TOLERANCE_MESSAGE = "approximate_entropy: tolerance must be finite and not negative."


def check_arguments(window: int, m: int, tolerance: float) -> None:
    """What approximate_entropy refuses, in the library's order (csrc/fmk_common.h: fmk_rule_apen); needs no device."""
    if int(m) < 1:
        raise ValueError(APEN_M_MESSAGE)
    if int(m) > APEN_MAX_M:
        raise ValueError(APEN_MAX_M_MESSAGE)
    if int(window) < int(m) + 1:
        raise ValueError(APEN_WINDOW_MESSAGE)
    if int(window) > APEN_MAX_WINDOW:
        raise ValueError(APEN_MAX_WINDOW_MESSAGE)
    if not (float(tolerance) >= 0.0 and float(tolerance) < math.inf):
        raise ValueError(APEN_TOLERANCE_MESSAGE)


def approximate_entropy(x: NDArray[np.float64], window: int, m: int = 2, tolerance: float = 0.2) -> NDArray[np.float64]:
    """Approximate entropy of x[t-window+1 .. t]: with `r = tolerance * std(window)` (population standard deviation) and, for k in
    (m, m + 1), `C_k[i]` the number of the `N_k = window - k + 1` vectors `(x_j .. x_{j+k-1})` within Chebyshev distance r of
    vector i (inclusive, itself counted), `phi_k = mean(ln(C_k / N_k))` and the output is `phi_m - phi_{m+1}`; it can be negative.
    NaN before the first full window and in every window that reads a NaN or an infinity; exactly 0.0 where every pair matches (a
    constant window).  `tolerance = 0` is legal: only equal values match.  ValueError for `m < 1`, `m > 4`, `window < m + 1`,
    `window > 1024` and a tolerance that is negative, NaN or infinite."""
    check_arguments(window, m, tolerance)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(len(xx), np.float64)
    if len(xx):
        _ffi.default_context().call("fmk_approximate_entropy", ptr(xx), c_i64(len(xx)), c_i64(int(window)), c_i64(int(m)),
                                    c_f64(float(tolerance)), ptr(out))
    return out
