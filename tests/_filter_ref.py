"""Plain Python restatement of the symmetric CUSUM event filter (finmlkit/sampling/filters.py:7-70) in the reference's evaluation
order: the quotient rounded to float64, math.log of it (libm: the project's `log` contract), Python's own max / min for the clamps.
What GPU results are compared with, bit for bit, on inputs that have no fixture.  Reads nothing outside the repository."""
import math

import numpy as np


def log_returns(x):
    """ret[i] = log(x[i] / x[i-1]) as IEEE arithmetic gives it: a zero divisor gives +-inf or NaN, log of 0 is -inf, of a negative
    number NaN.  ret[0] is NaN and never read."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        q = (x[1:] / x[:-1]).tolist()
    out = [math.nan]
    for v in q:
        if v > 0.0:
            out.append(math.log(v) if v != math.inf else math.inf)
        elif v == 0.0:
            out.append(-math.inf)
        else:                                        # negative or NaN
            out.append(math.nan)
    return out


def hashed_threshold(n, c, per_element, shift=0.0):
    """The threshold array of a seeded fixture case, in exact integer arithmetic so that every machine regenerates the same bits:
    the constant c, or c * (1 + h(i) / 1024) - shift * c with a multiplicative hash h of the index (shift > 1 makes some negative)."""
    if not per_element:
        return np.array([c], np.float64)
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(1024)
    return c * (1.0 + h.astype(np.float64) / 1024.0) - shift * c


def cusum_filter(raw_time_series, threshold, negative_first=True, return_state=False):
    """-> int64 event indices.  `negative_first=False` swaps the order in which the two sides are tested (for the test that shows an
    input separates the two orders); `return_state`: also the final (s_pos, s_neg)."""
    n = len(raw_time_series)
    if n <= 1:
        raise ValueError("Input time series must have at least 2 elements.")
    if len(threshold) != 1 and len(threshold) != n:
        raise ValueError("Threshold array must either contain 1 const. element or len(raw_time_series) elements.")
    thr = np.asarray(threshold, np.float64).tolist()
    if len(thr) == 1:
        thr = thr * n
    ret = log_returns(raw_time_series)
    events = []
    s_pos = s_neg = 0.0
    for i in range(1, n):
        r, t = ret[i], thr[i]
        s_pos = max(0.0, s_pos + r)                  # Python's max / min: a NaN second argument loses, -0.0 loses to 0.0
        s_neg = min(0.0, s_neg + r)
        if negative_first:
            if s_neg < -t:
                s_neg = 0.0
                events.append(i)
            elif s_pos > t:
                s_pos = 0.0
                events.append(i)
        else:
            if s_pos > t:
                s_pos = 0.0
                events.append(i)
            elif s_neg < -t:
                s_neg = 0.0
                events.append(i)
    ev = np.asarray(events, np.int64)
    return (ev, (s_pos, s_neg)) if return_state else ev
