"""Bet sizing of Advances in Financial Machine Learning, chapter 10, on label spans: from a predicted probability to a signal, the
average of the signals of the bets still open per tick of the tape (snippets 10.1 / 10.2), its discretisation (10.3), the budget
approach of section 10.2 and the sigmoid family of snippet 10.4.  The reference has no such functions: the definition is this
project's.  Signals are counted in units of 2^-30 and summed as integers, so a path is a function of its
events and nothing else, bit for bit.  The paths are made on the MI355X (csrc/fmk_bet.hip): a difference array over the tape and one
device-wide scan, the loop of `label_concurrency`; the closed forms are O(events) NumPy on the host, like `time_decay`."""
from __future__ import annotations

import ctypes as C
import math
import operator
from typing import Optional

import numpy as np
from numpy.typing import NDArray

from .. import _ffi
from .._ffi import c_f64, c_i64, ptr
from .bootstrap import UNIT, _spans

MAX_CONCURRENCY = 32767


# ---------------------------------------------------------------------------------------- argument rules (no device)
def check_step(what: str, step) -> float:
    try:
        step = float(step)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: step must be a number.") from None
    if not (step == 0.0 or 0.0 < step <= 1.0):
        raise ValueError(f"{what}: step must be 0 (no discretisation) or in (0, 1].")
    return step


def _signal(what, signal, n_events):
    m = np.asarray(signal)
    if m.ndim != 1 or (m.size and m.dtype.kind not in "fiu"):
        raise ValueError(f"{what}: signal must be a one-dimensional array of real numbers.")
    if len(m) != n_events:
        raise ValueError(f"{what}: signal must have the length of event_idxs.")
    m = np.ascontiguousarray(m, dtype=np.float64)
    bad = int(np.count_nonzero(~((m >= -1.0) & (m <= 1.0))))
    if bad:
        raise ValueError(f"{what}: {bad} signals are NaN or outside [-1, 1]")
    return m


def _side(what, side, n_events):
    s = np.asarray(side)
    if s.ndim != 1 or (s.size and s.dtype.kind not in "iu"):
        raise ValueError(f"{what}: side must be a one-dimensional integer array.")
    if len(s) != n_events:
        raise ValueError(f"{what}: side must have the length of event_idxs.")
    return np.ascontiguousarray(np.sign(s), dtype=np.int8)


def _at(what, at_idxs, n):
    at = np.asarray(at_idxs)
    if at.ndim != 1 or (at.size and at.dtype.kind not in "iu"):
        raise ValueError(f"{what}: at_idxs must be a one-dimensional integer array.")
    at = np.ascontiguousarray(at, dtype=np.int64)
    bad = int(np.count_nonzero((at < 0) | (at >= n)))
    if bad:
        raise ValueError(f"{what}: {bad} indices outside [0, {n})")
    return at


def _axis(what, ev, tc, n):
    ev, tc, n = _spans(what, ev, tc, n)
    if n < 1:
        raise ValueError(f"{what}: n must be between 1 and 2^32.")
    return ev, tc, n


def geometry() -> dict:
    """The kernels' geometry (fmk_bet_geometry): needs no device.  tile: the ticks of one workgroup; row: the ticks of one workgroup
    scan (a thread owns four consecutive ticks of it); agg_unit: the tiles of one trip of the aggregate scan."""
    out = (C.c_int64 * 3)()
    _ffi.check(_ffi.lib().fmk_bet_geometry(out))
    return dict(zip(("tile", "row", "agg_unit"), (int(v) for v in out)))


# ---------------------------------------------------------------------------------------- the paths (device)
def bet_size_path(event_idxs: NDArray[np.int64], touch_idxs: NDArray[np.int64], signal: NDArray[np.float64], n: Optional[int] = None,
                  step: float = 0.0, return_count: bool = False):
    """-> value, float64 of n ticks: the average of the signals of the events open at each tick, event i being open on
    event_idxs[i] <= t < touch_idxs[i] (the bet is closed at the touch; an event with touch == event is never open), +0.0 where
    none is; discretised when step > 0 (`discretise`).  With return_count also the int16 number of open events per tick.
    n: the length of the tape (default max(touch_idxs) + 1).  signal: float64 in [-1, 1], taken in units of 2^-30.
    ValueError: no events, lengths or dtypes that do not fit, an event outside 0 <= event_idx <= touch_idx < n, a signal that is NaN
    or outside [-1, 1], a step that is neither 0 nor in (0, 1], n > 2^32, more than 32767 events open on one tick."""
    ev, tc, n = _axis("bet_size_path", event_idxs, touch_idxs, n)
    m = _signal("bet_size_path", signal, len(ev))
    step = check_step("bet_size_path", step)
    value = np.empty(n, np.float64)
    count = np.empty(n, np.int16) if return_count else None
    _ffi.default_context().call("fmk_bet_size_path", ptr(ev), ptr(tc), ptr(m), c_i64(len(ev)), c_i64(n), c_f64(step), ptr(value),
                                ptr(count))
    return (value, count) if return_count else value


def bet_size_at(event_idxs: NDArray[np.int64], touch_idxs: NDArray[np.int64], signal: NDArray[np.float64],
                at_idxs: Optional[NDArray[np.int64]] = None, n: Optional[int] = None, step: float = 0.0) -> NDArray[np.float64]:
    """The path of `bet_size_path` at chosen ticks (the path itself stays on the device).  at_idxs None: each event's own tick -- the
    bet in force once that signal has arrived.  ValueError as `bet_size_path`, and for an index outside [0, n)."""
    ev, tc, n = _axis("bet_size_at", event_idxs, touch_idxs, n)
    m = _signal("bet_size_at", signal, len(ev))
    step = check_step("bet_size_at", step)
    at = ev if at_idxs is None else _at("bet_size_at", at_idxs, n)
    out = np.empty(len(at), np.float64)
    _ffi.default_context().call("fmk_bet_size_at", ptr(ev), ptr(tc), ptr(m), c_i64(len(ev)), c_i64(n), c_f64(step), ptr(at),
                                c_i64(len(at)), ptr(out))
    return out


def avg_active_signals(event_idxs: NDArray[np.int64], touch_idxs: NDArray[np.int64], signal: NDArray[np.float64],
                       n: Optional[int] = None, step: float = 0.0):
    """Snippet 10.2's series -> (points, values): the sorted distinct ticks at which a bet opens or closes, and the average of the
    active signals there."""
    ev, tc, n = _axis("avg_active_signals", event_idxs, touch_idxs, n)
    points = np.union1d(ev, tc)
    return points, bet_size_at(ev, tc, signal, points, n, step)


def bet_size_budget(event_idxs: NDArray[np.int64], touch_idxs: NDArray[np.int64], side: NDArray[np.int8], n: Optional[int] = None):
    """The budget approach of section 10.2 -> (m, max_long, max_short): with cl[t] / cs[t] the open events of side > 0 / side < 0
    (side 0 counts nowhere) and Ml, Ms their maxima over the tape, m[t] = cl[t] / Ml - cs[t] / Ms, a term being 0 where its maximum
    is.  ValueError as `bet_size_path`; the bound of 32767 holds for each side."""
    ev, tc, n = _axis("bet_size_budget", event_idxs, touch_idxs, n)
    sd = _side("bet_size_budget", side, len(ev))
    m, max2 = np.empty(n, np.float64), np.zeros(2, np.int64)
    _ffi.default_context().call("fmk_bet_size_budget", ptr(ev), ptr(tc), ptr(sd), c_i64(len(ev)), c_i64(n), ptr(m), ptr(max2))
    return m, int(max2[0]), int(max2[1])


# ---------------------------------------------------------------------------------------- host closed forms
def discretise(values, step: float) -> NDArray[np.float64]:
    """Snippet 10.3: min(1, max(-1, rint(v / step) * step)) in float64, one operation at a time (rint: ties to even); step 0: the
    values as they are.  What the kernels apply to a path."""
    step = check_step("discretise", step)
    v = np.array(values, dtype=np.float64)
    if step == 0.0:
        return v
    return np.minimum(1.0, np.maximum(-1.0, np.rint(v / step) * step))


def signal_from_probability(prob, pred=None, side=None, n_classes: int = 2) -> NDArray[np.float64]:
    """Snippet 10.1's signal: z = (p - 1/K) / sqrt(p (1 - p)), m = pred * erf(z / sqrt(2)) = pred * (2 Phi(z) - 1), times side for
    meta labels.  p = 0 gives -pred and p = 1 gives +pred (z = -inf, +inf).  pred (default 1) and side: values in [-1, 1].
    ValueError: p outside [0, 1] or NaN, n_classes < 2, pred / side outside [-1, 1] or NaN, lengths that differ."""
    try:
        k = operator.index(n_classes)
    except TypeError:
        raise ValueError("signal_from_probability: n_classes must be an integer.") from None
    if k < 2:
        raise ValueError("signal_from_probability: n_classes must be at least 2.")
    p = np.array(prob, dtype=np.float64, ndmin=1)
    if p.ndim != 1:
        raise ValueError("signal_from_probability: prob must be one-dimensional.")
    if np.count_nonzero(~((p >= 0.0) & (p <= 1.0))):
        raise ValueError("signal_from_probability: a probability is NaN or outside [0, 1].")
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (p - 1.0 / k) / np.sqrt(p * (1.0 - p))
    root2 = math.sqrt(2.0)
    m = np.array([math.erf(v / root2) for v in z], dtype=np.float64)
    for name, factor in (("pred", pred), ("side", side)):
        if factor is None:
            continue
        f = np.array(factor, dtype=np.float64, ndmin=1)
        if f.shape != p.shape:
            raise ValueError(f"signal_from_probability: {name} must have the length of prob.")
        if np.count_nonzero(~((f >= -1.0) & (f <= 1.0))):
            raise ValueError(f"signal_from_probability: a value of {name} is NaN or outside [-1, 1].")
        m = m * f
    return m


def _positive(what, name, w):
    w = np.asarray(w, dtype=np.float64)
    if np.count_nonzero(~(w > 0.0)):
        raise ValueError(f"{what}: {name} must be positive.")
    return w


def _inside(what, m, zero_ok):
    m = np.asarray(m, dtype=np.float64)
    if np.count_nonzero(~((m > -1.0) & (m < 1.0))) or (not zero_ok and np.count_nonzero(m == 0.0)):
        raise ValueError(f"{what}: m must lie inside (-1, 1)" + ("." if zero_ok else " and must not be 0."))
    return m


def bet_size_sigmoid(w, x):
    """Snippet 10.4's betSize: x / sqrt(w + x^2), x = forecast - price.  ValueError: w <= 0."""
    w, x = _positive("bet_size_sigmoid", "w", w), np.asarray(x, dtype=np.float64)
    r = x / np.sqrt(w + x * x)
    return float(r) if r.ndim == 0 else r


def calibrate_w(x, m):
    """Snippet 10.4's getW: the w at which a divergence x gives the bet size m, x^2 (m^-2 - 1).  ValueError: m outside (-1, 1) or 0."""
    x, m = np.asarray(x, dtype=np.float64), _inside("calibrate_w", m, False)
    r = x * x * (m ** -2.0 - 1.0)
    return float(r) if r.ndim == 0 else r


def target_position(w, f, price, max_pos):
    """Snippet 10.4's getTPos: trunc(bet_size_sigmoid(w, f - price) * max_pos) as int64.  ValueError: w <= 0, max_pos < 1."""
    if np.count_nonzero(~(np.asarray(max_pos, dtype=np.float64) >= 1.0)):
        raise ValueError("target_position: max_pos must be at least 1.")
    r = np.trunc(np.asarray(bet_size_sigmoid(w, np.asarray(f, dtype=np.float64) - np.asarray(price, dtype=np.float64))) * max_pos)
    r = r.astype(np.int64)
    return int(r) if r.ndim == 0 else r


def inv_price(f, w, m):
    """Snippet 10.4's invPrice: the price at which the bet size is m, f - m sqrt(w / (1 - m^2)).  ValueError: w <= 0, m outside
    (-1, 1)."""
    w, m = _positive("inv_price", "w", w), _inside("inv_price", m, True)
    r = np.asarray(f, dtype=np.float64) - m * np.sqrt(w / (1.0 - m * m))
    return float(r) if r.ndim == 0 else r


def limit_price(t_pos: int, pos: int, f: float, w: float, max_pos: int) -> float:
    """Snippet 10.4's limitPrice: the mean of inv_price over the units between the position and the target, summed in the book's
    order (j from |pos + sgn| to |t_pos|); NaN when t_pos == pos.  ValueError: w <= 0, max_pos < 1, a unit at or beyond max_pos."""
    try:
        t_pos, pos, max_pos = operator.index(t_pos), operator.index(pos), operator.index(max_pos)
    except TypeError:
        raise ValueError("limit_price: t_pos, pos and max_pos must be integers.") from None
    if max_pos < 1:
        raise ValueError("limit_price: max_pos must be at least 1.")
    _positive("limit_price", "w", w)
    if t_pos == pos:
        return float("nan")
    sgn = 1 if t_pos >= pos else -1
    total = 0.0
    for j in range(abs(pos + sgn), abs(t_pos + 1)):
        total += inv_price(f, w, j / float(max_pos))
    return total / (t_pos - pos)


__all__ = ["bet_size_path", "bet_size_at", "avg_active_signals", "bet_size_budget", "discretise", "geometry",
           "signal_from_probability", "bet_size_sigmoid", "calibrate_w", "target_position", "inv_price", "limit_price",
           "check_step", "MAX_CONCURRENCY", "UNIT"]
