"""Trend-scanning labels (Lopez de Prado, Machine Learning for Asset Managers, ch. 5) under the name the reference reserves:
finmlkit/label/trend_scanning.py is an empty placeholder there, so the definition is this project's.  Every
look-forward span of every event is fitted on the MI355X (csrc/fmk_trend.hip)."""
from __future__ import annotations

import ctypes as C
import operator
import warnings
from typing import Tuple

import numpy as np
from numpy.typing import NDArray

from .. import _ffi
from .._ffi import c_i64, ptr


def check_arguments(n_close, event_idxs, min_len, max_len, step):
    """What the library refuses (FMK_E_ARG), asked on the host before anything reaches a device -> (min_len, max_len, step) as
    ints.  event_idxs: the host array of event indices, or None when they are resident and the library checks them."""
    try:
        min_len, max_len, step = operator.index(min_len), operator.index(max_len), operator.index(step)
    except TypeError:
        raise ValueError("trend_scanning: min_len, max_len and step must be integers.") from None
    if min_len < 3:
        raise ValueError("trend_scanning: min_len must be at least 3.")
    if max_len < min_len:
        raise ValueError("trend_scanning: max_len must not be less than min_len.")
    if step < 1:
        raise ValueError("trend_scanning: step must be at least 1.")
    if event_idxs is not None and len(event_idxs):
        ev = np.asarray(event_idxs)
        if ev.ndim != 1 or ev.dtype.kind not in "iu":
            raise ValueError("trend_scanning: event_idxs must be a one-dimensional integer array.")
        bad = int(np.count_nonzero((ev < 0) | (ev >= n_close)))
        if bad:
            raise ValueError(f"trend_scanning: {bad} event indices outside [0, {n_close})")
    return min_len, max_len, step


def trend_scanning(close: NDArray[np.float64], event_idxs: NDArray[np.int64], min_len: int = 5, max_len: int = 20, step: int = 1
                   ) -> Tuple[NDArray[np.int8], NDArray[np.float64], NDArray[np.int64], NDArray[np.float64]]:
    """-> (labels, t_values, touch_idxs, rets).  From each event t0 a line is fitted to close[t0 .. t0+L-1] for every span
    L = min_len, min_len + step, ... <= max_len; the span whose slope has the largest |t-value| is kept (the smallest L among
    equals): label = the sign of that t-value, touch index = t0 + L - 1, ret = close[touch] / close[t0] - 1.  A constant span has
    t = 0, an exact fit +-inf, a span that holds a NaN is never chosen.  An event whose longest span runs past the end of the
    series, or all of whose spans hold a NaN, has label 0, NaN t-value and return and its own index as touch index; one
    RuntimeWarning says how many there were.  ValueError: min_len < 3, max_len < min_len, step < 1, an event outside the series."""
    px = np.ascontiguousarray(close, dtype=np.float64)
    ev = np.asarray(event_idxs)
    if ev.size == 0:
        ev = ev.astype(np.int64)
    min_len, max_len, step = check_arguments(len(px), ev, min_len, max_len, step)
    ev = np.ascontiguousarray(ev, dtype=np.int64)
    ne = len(ev)
    labels, t_values = np.empty(ne, np.int8), np.empty(ne, np.float64)
    touch, rets = np.empty(ne, np.int64), np.empty(ne, np.float64)
    if ne == 0:
        return labels, t_values, touch, rets
    skipped = c_i64()
    _ffi.default_context().call("fmk_trend_scanning", ptr(px), c_i64(len(px)), ptr(ev), c_i64(ne), c_i64(min_len), c_i64(max_len),
                                c_i64(step), ptr(labels), ptr(t_values), ptr(touch), ptr(rets), C.byref(skipped))
    if skipped.value:
        warnings.warn(f"trend_scanning: {skipped.value} of {ne} events have no span that fits the series and is free of NaN and were "
                      "skipped (label 0, NaN t-value and return, touch index = event index)", RuntimeWarning, stacklevel=2)
    return labels, t_values, touch, rets
