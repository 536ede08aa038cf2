"""Drop-in for finmlkit/label/tbm.py::triple_barrier: the path of every event is walked on the MI355X (csrc/fmk_label.hip)."""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional, Tuple

import numpy as np
from numpy.typing import NDArray

from .. import _ffi
from .._ffi import c_f64, c_i64, ptr


def check_arguments(n_ts, n_close, n_events, n_targets, n_side, vertical_barrier, min_ret):
    """The argument checks of tbm.py:45-59, in the reference's order and with its messages."""
    if vertical_barrier <= 0:
        raise ValueError("The vertical barrier must be greater than zero.")
    if min_ret < 0:
        raise ValueError("The minimum return must be non-negative.")
    if n_ts != n_close:
        raise ValueError("The lengths of timestamps and close must match.")
    if n_events != n_targets:
        raise ValueError("The lengths of event_idxs and targets must match.")
    if n_events == 0:
        raise ValueError("The event_idxs array must not be empty.")
    if n_side is not None and n_events != n_side:
        raise ValueError("The length of event_idxs must match the length of side.")


def triple_barrier(timestamps: NDArray[np.int64], close: NDArray[np.float64], event_idxs: NDArray[np.int64],
                   targets: NDArray[np.float64], horizontal_barriers: Tuple[float, float], vertical_barrier: float,
                   min_close_time_sec: float, side: Optional[NDArray[np.int8]], min_ret: float
                   ) -> Tuple[NDArray[np.int8], NDArray[np.int64], NDArray[np.float64], NDArray[np.float64]]:
    """Reference: finmlkit/label/tbm.py:11-158 -> (labels, touch_idxs, rets, max_rb_ratios), bit for bit on every event the
    reference evaluates.  An event whose window holds no later tick (the reference skips it and leaves its touch index
    uninitialised) has label 0, NaN return and ratio and its own event index as touch index; one RuntimeWarning says how many there
    were.  Event indices outside the tape raise ValueError."""
    check_arguments(len(timestamps), len(close), len(event_idxs), len(targets), None if side is None else len(side),
                    vertical_barrier, min_ret)
    ts = np.ascontiguousarray(timestamps, dtype=np.int64)
    px = np.ascontiguousarray(close, dtype=np.float64)
    ev = np.ascontiguousarray(event_idxs, dtype=np.int64)
    tg = np.ascontiguousarray(targets, dtype=np.float64)
    sd = None if side is None else np.ascontiguousarray(side, dtype=np.int8)
    bottom, top = horizontal_barriers
    ne = len(ev)
    labels, touch = np.empty(ne, np.int8), np.empty(ne, np.int64)
    rets, ratios = np.empty(ne, np.float64), np.empty(ne, np.float64)
    skipped = c_i64()
    _ffi.default_context().call("fmk_triple_barrier", ptr(ts), ptr(px), c_i64(len(px)), ptr(ev), ptr(tg), ptr(sd), c_i64(ne),
                                c_f64(bottom), c_f64(top), c_f64(vertical_barrier), c_f64(min_close_time_sec), c_f64(min_ret),
                                ptr(labels), ptr(touch), ptr(rets), ptr(ratios), C.byref(skipped))
    if skipped.value:
        warnings.warn(f"triple_barrier: {skipped.value} of {ne} events have no later tick inside their vertical barrier and were "
                      "skipped (label 0, NaN return, touch index = event index)", RuntimeWarning, stacklevel=2)
    return labels, touch, rets, ratios
