"""The bar clock, run lengths and the opening range, computed on the MI355X (csrc/fmk_clock.hip): NumPy drop-ins for what the
reference's BarDuration, BarDurationEWMA, BarRate, DirRunLen and ORBBreak transforms compute (finmlkit/feature/transforms.py
:1511-1548, :1460-1508, :1210-1270, :1605-1664, :1122-1207; there pandas' diff, ewm, a time-window rolling sum, a sequential loop and
a Python loop per day).  `ts` is int64 nanoseconds and non-decreasing; what unsorted stamps give is undefined, as for
`comp_lagged_returns`.

These entries take int64 stamps and give int8 or two uint8 series, so they are no rows of `series_ops.OPS`; `CLOCK_OPS` below is
their table, `host` and `resident` its two drivers (the `DeviceTrades` methods and the transforms' device form use `resident`).
Dtypes, lengths and arguments are checked before a device is looked at, and an empty series is answered without one."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple, Tuple

import numpy as np
import pandas as pd
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import DeviceArray, c_f64, c_i64, c_vp, ptr
from ..series_ops import SPAN_MESSAGE

BAR_RATE_WINDOW_MESSAGE = "bar_rate: the window must be at least one nanosecond."
STAMPS_MESSAGE = "the timestamps must be a one-dimensional int64 array of nanoseconds."
ORB_SHAPE_MESSAGE = "orb_break: ts, high, low and close must be one-dimensional and of the same length."
ORB_RESIDENT_SHAPE_MESSAGE = "orb_break: ts, high, low and close must have the same length."


class ClockOp(NamedTuple):
    entry: str                        # the host-pointer entry of include/fmk.h; the device flavour is entry + "_dev"
    inputs: Tuple                     # the dtypes of the input series
    params: Tuple                     # the ctypes of the scalars in ABI order
    outs: Tuple                       # the dtypes of the output series


I64, F64 = np.dtype(np.int64), np.dtype(np.float64)
CLOCK_OPS = {
    "bar_duration": ClockOp("fmk_bar_duration", (I64,), (c_i64,), (F64,)),
    "bar_duration_ewma": ClockOp("fmk_bar_duration_ewma", (I64,), (c_f64,), (F64,)),
    "bar_rate": ClockOp("fmk_bar_rate", (I64,), (c_f64, c_i64), (F64,)),
    "dir_run_len": ClockOp("fmk_dir_run_len", (F64,), (), (np.dtype(np.int8),)),
    "orb_break": ClockOp("fmk_orb_break", (I64, F64, F64, F64), (), (np.dtype(np.uint8), np.dtype(np.uint8))),
}


def prototype(op: ClockOp) -> list:
    """The argtypes of both entries of a row: context, the series, n, the scalars, the outputs."""
    return [c_vp] * (1 + len(op.inputs)) + [c_i64, *op.params] + [c_vp] * len(op.outs)


@functools.lru_cache(maxsize=None)
def entries(op: ClockOp):
    """(host-pointer entry, device entry) of the loaded library, with restype and argtypes set from the row."""
    fns = tuple(getattr(_ffi.lib(), name) for name in (op.entry, op.entry + "_dev"))
    for fn in fns:
        fn.restype, fn.argtypes = C.c_int, prototype(op)
    return fns


def geometry() -> dict:
    """The tile sizes of the kernels (fmk_clock_geometry): needs no device."""
    out = (c_i64 * 4)()
    fn = _ffi.lib().fmk_clock_geometry
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(c_i64)]
    _ffi.check(fn(out))
    return dict(zip(("scan_tile", "scan_trip_tiles", "rate_tile", "rate_stage"), (int(v) for v in out)))


# ------------------------------------------------------------------------------------------------ argument rules (no device)
def rule_span(span) -> float:
    if not float(span) >= 1.0:
        raise ValueError(SPAN_MESSAGE)
    return float(span)


def window_ns(window_sec) -> int:
    """pd.Timedelta(seconds=window_sec).value, the window pandas' rolling uses; ValueError for what is below one nanosecond (the
    reference divides by zero there), not a number, or beyond a Timedelta."""
    try:
        w = pd.Timedelta(seconds=float(window_sec)).value
    except (OverflowError, ValueError, TypeError):
        raise ValueError(BAR_RATE_WINDOW_MESSAGE) from None
    if not isinstance(w, (int, np.integer)) or int(w) < 1:
        raise ValueError(BAR_RATE_WINDOW_MESSAGE)
    return int(w)


def _stamps(ts) -> np.ndarray:
    ts = np.asarray(ts)
    if ts.dtype != I64:
        raise TypeError(STAMPS_MESSAGE)
    if ts.ndim != 1:
        raise ValueError(STAMPS_MESSAGE)
    return np.ascontiguousarray(ts)


# ------------------------------------------------------------------------------------------------ the two drivers
def host(op: ClockOp, arrays, *values):
    """The host-pointer entry of `op` on prepared, C-contiguous arrays of one length -> a tuple of output arrays."""
    n = len(arrays[0])
    outs = tuple(np.empty(n, dt) for dt in op.outs)
    if n:
        ctx = _ffi.default_context()
        _ffi.check(entries(op)[0](ctx.handle, *[ptr(a) for a in arrays], n, *values, *[ptr(o) for o in outs]), ctx.handle)
    return outs


def resident(ctx, op: ClockOp, series, *values, unequal: str = ""):
    """The `_dev` entry of `op` on DeviceArrays -> a tuple of DeviceArrays.  Dtypes and lengths are checked before `ctx` or a pointer
    is looked at; an empty series is answered by empty arrays that own no memory."""
    for y, dt in zip(series, op.inputs):
        if y.dtype != dt:
            raise TypeError(f"{op.entry}_dev: the series must be {dt}, not {y.dtype}")
    n = series[0].n
    if any(y.n != n for y in series):
        raise ValueError(unequal)
    if not n:
        return tuple(DeviceArray(ctx, 0, dt, dptr=0) for dt in op.outs)
    outs = tuple(DeviceArray(ctx, n, dt) for dt in op.outs)
    _ffi.check(entries(op)[1](ctx.handle, *[y.p for y in series], n, *values, *[o.p for o in outs]), ctx.handle)
    return outs


# ------------------------------------------------------------------------------------------------ the five drop-ins
def bar_duration(ts: NDArray[np.int64], periods: int = 1) -> NDArray[np.float64]:
    """out[i] = (ts[i] - ts[i - periods]) / 1e9 where 0 <= i - periods < n, NaN elsewhere: pandas' `diff(periods)` of the stamps as
    `total_seconds()`, the reference's BarDuration bit for bit.  Any integer `periods`, zero and negative included."""
    return host(CLOCK_OPS["bar_duration"], (_stamps(ts),), int(periods))[0]


def bar_duration_ewma(ts: NDArray[np.int64], span=20) -> NDArray[np.float64]:
    """NaN at element 0, then `ewma`'s recursion over the bar durations, seeded at element 1: the reference's BarDurationEWMA
    (pandas' `ewm(span, adjust=True).mean()` of the durations) within 1e-9 relative, its NaN exactly.  `span < 1` raises ValueError
    with `ewma`'s message."""
    return host(CLOCK_OPS["bar_duration_ewma"], (_stamps(ts),), rule_span(span))[0]


def bar_rate(ts: NDArray[np.int64], window_sec: float) -> NDArray[np.float64]:
    """Bars per hour over the closed window [ts[i] - window, ts[i]]: (rows j <= i with ts[j] >= ts[i] - window) / window_sec * 3600,
    the reference's BarRate bit for bit (rows after i with the same stamp do not count).  The comparison is on int64 nanoseconds
    with window = pd.Timedelta(seconds=window_sec).value; a window below one nanosecond raises ValueError."""
    w = window_ns(window_sec)
    return host(CLOCK_OPS["bar_rate"], (_stamps(ts),), float(window_sec), w)[0]


def dir_run_len(x: NDArray[np.float64]) -> NDArray[np.int8]:
    """The length of the run of equal non-zero signs that row i ends (0 at row 0 and where x is +-0.0, 1 at a NaN), the reference's
    DirRunLen.numba_core; the low 8 bits as int8, as its compiled store (a run of 128 reads -128).  One element gives [0]."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("dir_run_len: x must be one-dimensional.")
    return host(CLOCK_OPS["dir_run_len"], (x,))[0]


def orb_break(ts: NDArray[np.int64], high, low, close) -> Tuple[NDArray[np.bool_], NDArray[np.bool_]]:
    """(orb_long, orb_short) of the reference's ORBBreak: inside a UTC day whose first row is stamped in the day's first minute, from
    the day's fifth row on, close > max(high of the first four rows) and close < min(low of the first four rows), NaN skipped.
    Strictly increasing stamps (the reference marks every row of a duplicated stamp)."""
    ts = _stamps(ts)
    cols = [np.ascontiguousarray(a, dtype=np.float64) for a in (high, low, close)]
    if not all(c.ndim == 1 and len(c) == len(ts) for c in cols):
        raise ValueError(ORB_SHAPE_MESSAGE)
    lg, sh = host(CLOCK_OPS["orb_break"], (ts, *cols))
    return lg.view(np.bool_), sh.view(np.bool_)
