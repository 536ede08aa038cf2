"""Drop-in for finmlkit/feature/core/trend.py::adx_core, computed on the MI355X (csrc/fmk_recur.hip)."""
from __future__ import annotations

from ..series_ops import ADX_LENGTH_MESSAGE as LENGTH_MESSAGE, ADX_SHAPE_MESSAGE as SHAPE_MESSAGE, OPS, host  # noqa: F401


def adx_core(high, low, close, length):
    """Reference: finmlkit/feature/core/trend.py:8-96: Wilder's sums of true range, +DM and -DM from bar `length`, the directional
    indices and dx from them, adx[2 * length - 1] = mean(dx[length : 2 * length]) and (adx * (length - 1) + dx) / length after
    it; 0.0 before and everywhere when the series is shorter than 2 * length.  A NaN price makes the sums NaN and dx 0.0 from
    there on, as in the reference.  `length < 1` raises ValueError (the reference divides by zero there).  Two device-wide scans:
    the outputs agree with the reference within 1e-7 absolute on the 0-100 scale, the zeros exactly.  Outside the contract: infinite prices, and
    sums that have decayed below 2^-969 over bars without a range (1 657 of them at length 3, 9 063 at length 14): the reference's sums
    stall at the smallest subnormals for lengths of 3 and more (0.0 at lengths 1 and 2) and dx is a quotient of those, the scan's
    composed sums underflow to 0.0 and dx is 0.0; this ends once each sum has taken a non-zero term and the last average has
    forgotten those dx (100 * (1 - 1 / length)^t after t bars).  DESIGN.md section 7e; tests/test_gpu_recur_runs.py pins it."""
    return host(OPS["adx"], (high, low, close), length)
