"""Drop-in for the tick-level estimators of finmlkit/feature/core/volatility.py on the MI355X.

The estimators that run on the raw tick frame are on the hot path: `ewmst`,
`ewmst_mean0`, `ewms` and `realized_vol`; `rolling_variance_nb` and `variance_ratio_1_4_core` (the reference's
microstructure-noise detector) run on a resident series too (csrc/fmk_rolling.hip), and so do `true_range` and `atr`
(csrc/fmk_recur.hip), `bollinger_percent_b` and `parkinson_range` (csrc/fmk_runsum.hip).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import c_f64, c_i64, ptr
from ..series_ops import ATR_WINDOW_MESSAGE, BOLLINGER_WINDOW_MESSAGE, HLC_MESSAGE, OPS, PARKINSON_MESSAGE, host  # noqa: F401


def _ewmst(timestamps, y, half_life, sigma_floor, mean0):
    ctx = _ffi.default_context()
    ts = np.ascontiguousarray(timestamps, dtype=np.int64)
    yy = np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty(len(yy), np.float64)
    ctx.call("fmk_ewmst", ptr(ts), ptr(yy), c_i64(len(yy)), c_f64(half_life), c_f64(sigma_floor),
             C.c_int(int(mean0)), ptr(out))
    return out


def ewmst(timestamps: NDArray[np.int64], y: NDArray[np.float64], half_life: float,
          sigma_floor: float = 1e-12) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:139-219 (unbiased time-decay EWMA std)."""
    return _ewmst(timestamps, y, half_life, sigma_floor, False)


def ewmst_mean0(timestamps: NDArray[np.int64], y: NDArray[np.float64], half_life: float,
                sigma_floor: float = 1e-12) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:72-136 (zero-mean variant)."""
    return _ewmst(timestamps, y, half_life, sigma_floor, True)


def ewms(y: NDArray[np.float64], span: int) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:9-69 (fixed-alpha EW std, alpha = 2/(span+1))."""
    ctx = _ffi.default_context()
    yy = np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty(len(yy), np.float64)
    ctx.call("fmk_ewms", ptr(yy), c_i64(len(yy)), c_i64(int(span)), ptr(out))
    return out


def realized_vol(r: NDArray[np.float64], window: int, is_sample: bool) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:256-286 (rolling sqrt(nansum(r^2) / (valid - is_sample)))."""
    ctx = _ffi.default_context()
    rr = np.ascontiguousarray(r, dtype=np.float64)
    if int(window) == 0:                           # every window is empty: NaN everywhere (nothing to compute)
        return np.full(len(rr), np.nan)
    out = np.empty(len(rr), np.float64)
    ctx.call("fmk_realized_vol", ptr(rr), c_i64(len(rr)), c_i64(int(window)), C.c_int(bool(is_sample)), ptr(out))
    return out


def rolling_variance_nb(series: NDArray[np.float64], window: int, ddof: int = 1, min_periods: int = 1) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:440-478: per window the count, sum and sum of squares of the non-NaN
    elements, max(0, (sum_sq / cnt - mean^2) * (cnt / (cnt - ddof))) when cnt >= min_periods and cnt > ddof, NaN otherwise."""
    return host(OPS["rolling_variance"], (series,), window, ddof, min_periods)


def variance_ratio_1_4_core(price: NDArray[np.float64], window: int, ddof: int, ret_type: str) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:481-540: var(1-step returns) / (var(4-step returns) / 4) over `window`;
    `ret_type` "log" takes log returns (the host's log), anything else simple returns."""
    return host(OPS["variance_ratio_1_4"], (price,), window, ddof, ret_type == "log")


def true_range(high: NDArray, low: NDArray, close: NDArray) -> NDArray:
    """Reference: finmlkit/feature/core/volatility.py:222-253: max(high - low, |high - close[i-1]|, |low - close[i-1]|), NaN where
    one of the three inputs is; bar 0 is high - low.  The reference's bits."""
    return host(OPS["true_range"], (high, low, close))


def atr(high: NDArray[np.float64], low: NDArray[np.float64], close: NDArray[np.float64], window: int, ema_based: bool = False,
        normalize: bool = False) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:352-437.  SMA mode: the mean of the non-NaN true ranges of the window, the
    reference's bits (its NaN at bar 2 included).  EMA mode: the mean of the first window's non-NaN true ranges, then
    ((window - 1) * atr + tr) / window, NaN for good from the first NaN true range on; a device-wide scan that agrees with the
    reference to a few units in the last place (1e-9 relative is the contract), NaN positions and exact zeros exactly; outside the
    contract there: infinite prices, and an average that has decayed below 2^-969 over bars without a range (1 657 of them at window
    3, 9 063 at window 14) until the next bar with one: the reference stalls at the smallest subnormals for windows of 3 and more and
    reaches 0.0 at windows 1 and 2, the scan's composed state underflows to 0.0 (DESIGN.md section 7e;
    tests/test_gpu_recur_runs.py pins it).  `normalize` divides by (high + low) / 2.0.  Window 0 gives NaN everywhere, as the reference;
    a negative window raises ValueError."""
    return host(OPS["atr"], (high, low, close), window, ema_based, normalize)


def bollinger_percent_b(close: NDArray[np.float64], window: int, num_std: float) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:289-338: (close - lower) / (upper - lower) of the Bollinger bands mean -+
    num_std * sd over `window`, from the reference's running sum and sum of squares (sum += close[i] - close[i-window]); NaN before
    window - 1, where upper > lower is false, from a NaN of `close` on, everywhere when the series is shorter than the window
    and for window 1.  `window < 1` raises ValueError.  A device-wide scan with the coefficient 1: bit for bit the reference on
    exactly summable prices; otherwise the sum that enters a thread's 8 elements is added in another order, and as the variance
    cancels the outputs agree within a few 2^-52 * sumsq / ((window - 1) * var).  Outside the contract:
    infinite prices, and on prices that are not exactly summable a window whose elements are all equal (the reference's
    NaN-or-number there is rounding noise)."""
    return host(OPS["bollinger_percent_b"], (close,), window, num_std)


def parkinson_range(high: NDArray[np.float64], low: NDArray[np.float64]) -> NDArray[np.float64]:
    """Reference: finmlkit/feature/core/volatility.py:341-349: log(high / low) ** 2 / (log(2.0) * 4.0) with the host's log, the
    reference's bits: inf where low is 0, NaN where an input is NaN or the ratio negative.  Unequal lengths raise ValueError."""
    return host(OPS["parkinson_range"], (high, low))
