"""Drop-ins for finmlkit/label/weights.py.  The two loops over the tick tape -- concurrency / average uniqueness and return
attribution -- run on the MI355X (csrc/fmk_label.hip); time decay and class balance are O(events) and stay NumPy on the host."""
from __future__ import annotations

from typing import Tuple

import numpy as np
from numpy.typing import NDArray

from .. import _ffi
from .._ffi import c_i64, ptr


def average_uniqueness(timestamps: NDArray[np.int64], event_idxs: NDArray[np.int64], touch_idxs: NDArray[np.int64]
                       ) -> Tuple[NDArray[np.float64], NDArray[np.int16]]:
    """Reference: finmlkit/label/weights.py:7-49 -> (weights, concurrency).  Events outside 0 <= event <= touch < len(timestamps)
    raise ValueError (the reference slices silently into something else there)."""
    if len(event_idxs) != len(touch_idxs):
        raise ValueError("Timestamps and lookahead indices must have the same length.")
    n, ne = len(timestamps), len(event_idxs)
    concurrency = np.zeros(n, np.int16)
    weights = np.zeros(ne, np.float64)
    if ne == 0:
        return weights, concurrency
    ev = np.ascontiguousarray(event_idxs, dtype=np.int64)
    tc = np.ascontiguousarray(touch_idxs, dtype=np.int64)
    ctx = _ffi.default_context()
    ctx.call("fmk_label_concurrency", ptr(ev), ptr(tc), c_i64(ne), c_i64(n), ptr(concurrency))
    ctx.call("fmk_label_weights", None, ptr(concurrency), c_i64(n), ptr(ev), ptr(tc), c_i64(ne), ptr(weights), None)
    return weights, concurrency


def normalize_attribution(weights: NDArray[np.float64]) -> NDArray[np.float64]:
    """weights.py:96-101: rescaled to sum to the number of events."""
    total = np.sum(weights)
    if total <= 0.:
        raise ValueError("Sum of weights is zero or negative, cannot normalize.")
    weights *= len(weights) / total
    return weights


def return_attribution(event_idxs: NDArray[np.int64], touch_idxs: NDArray[np.int64], close: NDArray[np.float64],
                       concurrency: NDArray[np.int16], normalize: bool) -> NDArray[np.float64]:
    """Reference: finmlkit/label/weights.py:52-103."""
    ne, n = len(event_idxs), len(close)
    weights = np.zeros(ne, np.float64)
    if ne:
        ev = np.ascontiguousarray(event_idxs, dtype=np.int64)
        tc = np.ascontiguousarray(touch_idxs, dtype=np.int64)
        px = np.ascontiguousarray(close, dtype=np.float64)
        cc = np.ascontiguousarray(concurrency, dtype=np.int16)
        if len(cc) != n:
            raise ValueError("close and concurrency must have the same length.")
        _ffi.default_context().call("fmk_label_weights", ptr(px), ptr(cc), c_i64(n), ptr(ev), ptr(tc), c_i64(ne), None,
                                    ptr(weights))
    return normalize_attribution(weights) if normalize else weights


def time_decay(avg_uniqueness: NDArray[np.float64], last_weight: float) -> NDArray[np.float64]:
    """Reference: finmlkit/label/weights.py:106-142: linear decay along the cumulated uniqueness, newest weight 1."""
    if not -1.0 <= last_weight <= 1.0:
        raise ValueError("last_weight must lie in [-1, 1]")
    cum = np.cumsum(avg_uniqueness)
    total = cum[-1]
    if total == 0.0:
        raise ValueError("The sum of all average uniqueness weights must be grater than 0.")
    slope = (1. - last_weight) / total if last_weight >= 0.0 else 1. / ((last_weight + 1.) * total)
    out = (1. - slope * total) + slope * cum
    return np.maximum(out, 0.0) if last_weight < 0.0 else out


def class_balance_weights(labels: NDArray[np.int8], base_w: NDArray[np.float64]
                          ) -> Tuple[NDArray[np.int8], NDArray[np.float64], NDArray[np.float64], NDArray[np.float64]]:
    """Reference: finmlkit/label/weights.py:146-188 -> (classes, class weights, weighted class sizes, final sample weights).
    The class sizes are added in sample order, like the reference's loop."""
    classes = np.unique(labels)
    k = len(classes)
    where = np.searchsorted(classes, labels)
    size = np.zeros(k, np.float64)
    np.add.at(size, where, base_w)                     # unbuffered: sample order
    total = np.sum(size)
    cw = np.zeros(k, np.float64)
    for c in range(k):
        cw[c] = total / (k * size[c]) if size[c] > 0. else 0.0
    final = np.zeros(len(labels), np.float64)
    final[:] = np.asarray(base_w, dtype=np.float64) * cw[where] if len(labels) else 0.0
    return classes, cw, size, final
