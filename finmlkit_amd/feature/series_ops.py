"""The single-output series features as ONE table and two drivers.

Every row of `OPS` is one pair of entries of include/fmk.h with the shape
    int fmk_X[_dev](fmk_ctx*, <1..3 float64 series>, int64_t n, <0..3 scalars>, <double|float> *out)
`host` runs the host-pointer flavour on NumPy arrays (the drop-ins of feature/core/*.py), `resident` the `_dev` flavour on
DeviceArrays (the `DeviceTrades` methods of engine.py and the transforms' device form under `Compose`).  What a feature refuses, its
messages, how its scalars are marshalled and the prototypes ctypes checks every call against are stated here and nowhere else:
a new feature needs a kernel, its two prototypes in include/fmk.h and one row (tests/test_series_ops.py holds the rows against the
header, and the rules against the library's own).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Callable, NamedTuple, Tuple

import numpy as np

from .. import _ffi
from .._ffi import DeviceArray, c_f64, c_i64, c_vp, ptr

WINDOW_MESSAGE = "window must be at least 1."
ZSCORE_MESSAGE = "comp_zscore: window - ddof must be positive."
ROC_PERIOD_MESSAGE = "roc: period must not be negative."
PCT_PERIODS_MESSAGE = "pct_change: periods must not be negative."
STOCH_LENGTH_MESSAGE = "stoch_k: length must be at least 1."
STOCH_SHAPE_MESSAGE = "stoch_k: close, low and high must have the same length."
SPAN_MESSAGE = "span size is less than or equal to 1. Please provide a span size greater than 1."
RSI_WINDOW_MESSAGE = "rsi_wilder: window must be at least 1."
HLC_MESSAGE = "The length of high, low, and close prices must be the same."
ATR_WINDOW_MESSAGE = "atr: window must not be negative."
ADX_LENGTH_MESSAGE = "adx_core: length must be at least 1."
ADX_SHAPE_MESSAGE = "adx_core: high, low and close must have the same length."
BOLLINGER_WINDOW_MESSAGE = "bollinger_percent_b: window must be at least 1."
VWAP_PERIODS_MESSAGE = "vwap_distance: n_periods must be at least 1."
VWAP_SHAPE_MESSAGE = "vwap_distance: close and volume must have the same length."
RECENT_MESSAGE = "comp_flow_acceleration: recent_periods must not be negative."
VPIN_WINDOW_MESSAGE = "vpin: window must not be negative."
VPIN_SHAPE_MESSAGE = "vpin: volume_buy and volume_sell must have the same length."
PARKINSON_MESSAGE = "parkinson_range: high and low must have the same length."
CORR_SHAPE_MESSAGE = "rolling_price_volume_correlation: price and volume must be one-dimensional and of the same length."
CORR_RESIDENT_SHAPE_MESSAGE = "rolling_price_volume_correlation: price and volume must have the same length."
HURST_MIN_WINDOW = 9
HURST_WINDOW_MESSAGE = "hurst_exponent: window must be at least 9."
APEN_MAX_M = 4                       # the kernels are instantiated per m (csrc/fmk_common.h: FMK_APEN_MAX_M)
APEN_MAX_WINDOW = 1024               # one tile's span and the table of logarithms fit in LDS (FMK_APEN_MAX_WINDOW)
APEN_M_MESSAGE = "approximate_entropy: m must be at least 1."
APEN_MAX_M_MESSAGE = "approximate_entropy: m must be at most 4."
APEN_WINDOW_MESSAGE = "approximate_entropy: window must be at least m + 1."
APEN_MAX_WINDOW_MESSAGE = "approximate_entropy: window must be at most 1024."
APEN_TOLERANCE_MESSAGE = "approximate_entropy: tolerance must be finite and not negative."


def _any(*_) -> None:
    """The rule of a feature that refuses nothing."""


def _at_least(least: int, message: str) -> Callable:
    """The rule `first scalar >= least`."""
    def rule(arg, *_) -> None:
        if int(arg) < least:
            raise ValueError(message)
    return rule


def _rule_zscore(window, ddof) -> None:
    if int(window) < 1:
        raise ValueError(WINDOW_MESSAGE)
    if int(window) - int(ddof) <= 0:
        raise ValueError(ZSCORE_MESSAGE)


def _rule_ewma(span) -> None:
    if not float(span) >= 1.0:
        raise ValueError(SPAN_MESSAGE)


def _rule_flow_acceleration(window, recent_periods) -> None:
    if int(recent_periods) < 0:
        raise ValueError(RECENT_MESSAGE)


def _rule_hurst(window) -> None:
    if int(window) < 1:
        raise ValueError(WINDOW_MESSAGE)
    if int(window) < HURST_MIN_WINDOW:
        raise ValueError(HURST_WINDOW_MESSAGE)


def rule_approximate_entropy(window: int, m: int, tolerance: float) -> None:
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


class SeriesOp(NamedTuple):
    entry: str                        # the host-pointer entry of include/fmk.h; the device flavour is entry + "_dev"
    inputs: int                       # float64 input series: 1, 2 or 3
    params: Tuple = ()                # the ctypes of the scalars in ABI order; a C.c_int is a flag
    rule: Callable = _any             # over the scalars: ValueError for what the library answers with FMK_E_ARG
    unequal: str = ""                 # `host`'s message for inputs that are not one-dimensional and of one length
    unequal_resident: str = ""        # `resident`'s message for series of unequal length, where it is another one
    out: type = np.float64            # the output's dtype


_WINDOW = _at_least(1, WINDOW_MESSAGE)
OPS = {
    # rolling-window moments (csrc/fmk_rolling.hip)
    "sma": SeriesOp("fmk_sma", 1, (c_i64,), _WINDOW),
    "zscore": SeriesOp("fmk_zscore", 1, (c_i64, c_i64), _rule_zscore),
    "rolling_variance": SeriesOp("fmk_rolling_variance", 1, (c_i64, c_i64, c_i64), _WINDOW),
    "variance_ratio_1_4": SeriesOp("fmk_variance_ratio_1_4", 1, (c_i64, c_i64, C.c_int), _WINDOW),
    # windowed order statistics (csrc/fmk_order.hip)
    "burst_ratio": SeriesOp("fmk_burst_ratio", 1, (c_i64,), _WINDOW),
    "roc": SeriesOp("fmk_roc", 1, (c_i64,), _at_least(0, ROC_PERIOD_MESSAGE)),
    "pct_change": SeriesOp("fmk_pct_change", 1, (c_i64,), _at_least(0, PCT_PERIODS_MESSAGE)),
    "stoch_k": SeriesOp("fmk_stoch_k", 3, (c_i64,), _at_least(1, STOCH_LENGTH_MESSAGE), STOCH_SHAPE_MESSAGE),
    # recursive indicators (csrc/fmk_recur.hip)
    "ewma": SeriesOp("fmk_ewma", 1, (c_f64,), _rule_ewma),
    "rsi_wilder": SeriesOp("fmk_rsi_wilder", 1, (c_i64,), _at_least(1, RSI_WINDOW_MESSAGE)),
    "true_range": SeriesOp("fmk_true_range", 3, (), _any, HLC_MESSAGE),
    "atr": SeriesOp("fmk_atr", 3, (c_i64, C.c_int, C.c_int), _at_least(0, ATR_WINDOW_MESSAGE), HLC_MESSAGE),
    "adx": SeriesOp("fmk_adx", 3, (c_i64,), _at_least(1, ADX_LENGTH_MESSAGE), ADX_SHAPE_MESSAGE),
    # running-sum indicators (csrc/fmk_runsum.hip)
    "bollinger_percent_b": SeriesOp("fmk_bollinger_percent_b", 1, (c_i64, c_f64), _at_least(1, BOLLINGER_WINDOW_MESSAGE)),
    "vwap_distance": SeriesOp("fmk_vwap_distance", 2, (c_i64, C.c_int), _at_least(1, VWAP_PERIODS_MESSAGE), VWAP_SHAPE_MESSAGE),
    "flow_acceleration": SeriesOp("fmk_flow_acceleration", 1, (c_i64, c_i64), _rule_flow_acceleration),
    "vpin": SeriesOp("fmk_vpin", 2, (c_i64,), _at_least(0, VPIN_WINDOW_MESSAGE), VPIN_SHAPE_MESSAGE, out=np.float32),
    "parkinson_range": SeriesOp("fmk_parkinson_range", 2, (), _any, PARKINSON_MESSAGE),
    # rolling price-volume correlation (csrc/fmk_corr.hip)
    "price_volume_corr": SeriesOp("fmk_price_volume_corr", 2, (c_i64,), _WINDOW, CORR_SHAPE_MESSAGE, CORR_RESIDENT_SHAPE_MESSAGE),
    # window statistics (csrc/fmk_shape.hip)
    "rolling_kurtosis": SeriesOp("fmk_rolling_kurtosis", 1, (c_i64,), _WINDOW),
    "trend_slope": SeriesOp("fmk_trend_slope", 1, (c_i64,), _WINDOW),
    "hurst_exponent": SeriesOp("fmk_hurst_exponent", 1, (c_i64,), _rule_hurst),
    "bipower_variation": SeriesOp("fmk_bipower_variation", 1, (c_i64,), _WINDOW),
    # approximate entropy (csrc/fmk_entropy.hip)
    "approximate_entropy": SeriesOp("fmk_approximate_entropy", 1, (c_i64, c_i64, c_f64), rule_approximate_entropy),
}

_PYTHON = {c_i64: int, c_f64: float, C.c_int: bool}          # what a caller's number becomes before ctypes marshals it


def prototype(op: SeriesOp) -> list:
    """The argtypes of both entries of a row: context, the series, n, the scalars, the output."""
    return [c_vp] * (1 + op.inputs) + [c_i64, *op.params, c_vp]


@functools.lru_cache(maxsize=None)
def entries(op: SeriesOp):
    """(host-pointer entry, device entry) of the loaded library, with restype and argtypes set from the row."""
    fns = tuple(getattr(_ffi.lib(), name) for name in (op.entry, op.entry + "_dev"))
    for fn in fns:
        fn.restype, fn.argtypes = C.c_int, prototype(op)
    return fns


def _scalars(op: SeriesOp, params) -> list:
    """Apply the row's rule to the caller's scalars, then turn them into what the row's ctypes take."""
    op.rule(*params)
    return [_PYTHON[t](v) for t, v in zip(op.params, params)]


def host(op: SeriesOp, arrays, *params) -> np.ndarray:
    """The host-pointer entry of `op` on NumPy-convertible `arrays` -> array of len(arrays[0]).  The rule comes first: no device is
    needed to refuse a call, nor to answer an empty series."""
    values = _scalars(op, params)
    xs = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    if len(xs) > 1 and not (all(x.ndim == 1 for x in xs) and all(len(x) == len(xs[0]) for x in xs)):
        raise ValueError(op.unequal)
    n = len(xs[0])
    out = np.empty(n, op.out)
    if n:
        ctx = _ffi.default_context()
        _ffi.check(entries(op)[0](ctx.handle, *[ptr(x) for x in xs], n, *values, ptr(out)), ctx.handle)
    return out


def resident(ctx, op: SeriesOp, series, *params) -> DeviceArray:
    """The `_dev` entry of `op` on DeviceArrays -> DeviceArray.  Rule, dtype and lengths are checked, in this order, before `ctx` or
    a pointer is looked at; an empty series is answered by an empty array that owns no memory."""
    values = _scalars(op, params)
    for y in series:
        if y.dtype != np.float64:
            raise TypeError(f"{op.entry}_dev: the series must be float64, not {y.dtype}")
    n = series[0].n
    if any(y.n != n for y in series):
        raise ValueError(op.unequal_resident or op.unequal)
    if not n:
        return DeviceArray(ctx, 0, op.out, dptr=0)
    out = DeviceArray(ctx, n, op.out)
    _ffi.check(entries(op)[1](ctx.handle, *[y.p for y in series], n, *values, out.p), ctx.handle)
    return out
