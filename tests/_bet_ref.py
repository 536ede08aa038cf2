"""Bet sizing restated independently of the library: written from the definition's text, not from
csrc/fmk_bet_rule.h.  Two forms of the path and of the budget position -- a direct one (per tick a loop over the events, Python
integers, fractions.Fraction for the quotient) for small cases and a cumulative one (difference array, cumsum) for larger ones --
and the book's snippets 10.1 - 10.4 (Lopez de Prado, Advances in Financial Machine Learning, chapter 10) restated by hand in plain
NumPy / Python floats."""
from __future__ import annotations

import math
from fractions import Fraction
from statistics import NormalDist

import numpy as np

UNIT = 1 << 30
MAX_CONC = 32767


class Refused(Exception):
    """what the library answers with FMK_E_ARG / ValueError: kind in {"spans", "signals", "concurrency"} and the count it reports."""

    def __init__(self, kind, count):
        super().__init__(f"{kind} {count}")
        self.kind, self.count = kind, count


def quantise(m: float) -> int:
    """rint(m * 2^30) with ties to even, in exact rational arithmetic (Python's round of a Fraction rounds half to even)."""
    return int(round(Fraction(float(m)) * UNIT))


def _check(ev, tc, n, signal=None):
    bad = sum(1 for s, t in zip(ev, tc) if s < 0 or t < s or t >= n)
    if bad:
        raise Refused("spans", bad)
    if signal is not None:
        bad = sum(1 for (s, t), m in zip(zip(ev, tc), signal) if not (-1.0 <= m <= 1.0))
        if bad:
            raise Refused("signals", bad)


def discretise(v: float, step: float) -> float:
    """snippet 10.3 on one value with Python's round (half to even on the float64 quotient)."""
    if step == 0.0:
        return v
    return min(1.0, max(-1.0, round(v / step) * step))


def discretise_np(values, step):
    """the definition's form: rint for the rounding, so a negative value that rounds to zero keeps its sign (-0.0), which
    Python's integer-valued round does not; the two are equal as numbers."""
    v = np.asarray(values, np.float64)
    return v.copy() if step == 0.0 else np.minimum(1.0, np.maximum(-1.0, np.rint(v / step) * step))


def path_direct(ev, tc, signal, n, step=0.0):
    """-> (values, counts) as Python lists; per tick a loop over the events."""
    ev, tc, signal = [int(x) for x in ev], [int(x) for x in tc], [float(x) for x in signal]
    _check(ev, tc, n, signal)
    q = [quantise(m) for m in signal]
    values, counts = [], []
    for t in range(n):
        open_ = [i for i in range(len(ev)) if ev[i] <= t < tc[i]]
        c, S = len(open_), sum(q[i] for i in open_)
        counts.append(c)
        v = math.ldexp(float(Fraction(S, c)), -30) if c else 0.0       # float(Fraction) rounds correctly; the scaling is exact
        values.append(discretise(v, step))
    if max(counts) > MAX_CONC:
        raise Refused("concurrency", max(counts))
    return values, counts


def path_cumulative(ev, tc, signal, n, step=0.0):
    """-> (values float64, counts int64): difference arrays and cumsum.  |S| < 2^45 and c <= 32767 convert exactly, and NumPy's
    float64 division is correctly rounded."""
    ev, tc, signal = np.asarray(ev, np.int64), np.asarray(tc, np.int64), np.asarray(signal, np.float64)
    bad = int(np.count_nonzero((ev < 0) | (tc < ev) | (tc >= n)))
    if bad:
        raise Refused("spans", bad)
    bad = int(np.count_nonzero(~((signal >= -1.0) & (signal <= 1.0))))
    if bad:
        raise Refused("signals", bad)
    q = np.rint(signal * float(UNIT)).astype(np.int64)                   # the product is exact; rint: ties to even
    live = tc > ev
    ds, dc = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    np.add.at(ds, ev[live], q[live])
    np.add.at(ds, tc[live], -q[live])
    np.add.at(dc, ev[live], 1)
    np.add.at(dc, tc[live], -1)
    S, c = np.cumsum(ds)[:n], np.cumsum(dc)[:n]
    if int(c.max()) > MAX_CONC:
        raise Refused("concurrency", int(c.max()))
    v = np.zeros(n, np.float64)
    on = c > 0
    v[on] = (S[on].astype(np.float64) / c[on].astype(np.float64)) * 2.0 ** -30
    return discretise_np(v, step), c


def budget_direct(ev, tc, side, n):
    """-> (m list, Ml, Ms)."""
    ev, tc, side = [int(x) for x in ev], [int(x) for x in tc], [int(x) for x in side]
    _check(ev, tc, n)
    cl = [sum(1 for i in range(len(ev)) if side[i] > 0 and ev[i] <= t < tc[i]) for t in range(n)]
    cs = [sum(1 for i in range(len(ev)) if side[i] < 0 and ev[i] <= t < tc[i]) for t in range(n)]
    ml, ms = max(cl), max(cs)
    if max(ml, ms) > MAX_CONC:
        raise Refused("concurrency", max(ml, ms))
    m = [(float(Fraction(cl[t], ml)) if ml else 0.0) - (float(Fraction(cs[t], ms)) if ms else 0.0) for t in range(n)]
    return m, ml, ms


def budget_cumulative(ev, tc, side, n):
    ev, tc, side = np.asarray(ev, np.int64), np.asarray(tc, np.int64), np.asarray(side, np.int64)
    bad = int(np.count_nonzero((ev < 0) | (tc < ev) | (tc >= n)))
    if bad:
        raise Refused("spans", bad)
    out = []
    for pick in (side > 0, side < 0):
        live = pick & (tc > ev)
        d = np.zeros(n + 1, np.int64)
        np.add.at(d, ev[live], 1)
        np.add.at(d, tc[live], -1)
        out.append(np.cumsum(d)[:n])
    cl, cs = out
    ml, ms = int(cl.max()), int(cs.max())
    if max(ml, ms) > MAX_CONC:
        raise Refused("concurrency", max(ml, ms))
    a = cl.astype(np.float64) / float(ml) if ml else np.zeros(n)
    b = cs.astype(np.float64) / float(ms) if ms else np.zeros(n)
    return a - b, ml, ms


# ---------------------------------------------------------------------------------------- the book, by hand
def book_avg_active_signals(ev, tc, signal):
    """snippet 10.2: at every point where a bet opens or closes, the float mean of the signals with start <= point < end, 0 when
    none is active -> (points, means)."""
    ev, tc, signal = np.asarray(ev), np.asarray(tc), np.asarray(signal, np.float64)
    points = sorted(set(ev.tolist()) | set(tc.tolist()))
    means = []
    for loc in points:
        active = (ev <= loc) & (loc < tc)
        means.append(float(np.mean(signal[active])) if active.any() else 0.0)
    return np.asarray(points, np.int64), np.asarray(means)


def book_discrete_signal(signal0, step):
    """snippet 10.3: (signal0 / stepSize).round() * stepSize, capped at 1 and floored at -1."""
    s = np.round(np.asarray(signal0, np.float64) / step) * step
    s[s > 1] = 1
    s[s < -1] = -1
    return s


def book_get_signal(prob, pred, n_classes):
    """snippet 10.1: signal0 = (prob - 1/numClasses) / (prob (1 - prob))^.5;  signal0 = pred * (2 norm.cdf(signal0) - 1)."""
    nd = NormalDist()
    out = []
    for p, x in zip(prob, pred):
        z = (p - 1.0 / n_classes) / (p * (1.0 - p)) ** .5
        out.append(x * (2.0 * nd.cdf(z) - 1.0))
    return np.asarray(out)


def book_bet_size(w, x):
    return x / math.sqrt(w + x * x)                                       # x (w + x^2)^-.5


def book_get_t_pos(w, f, m_p, max_pos):
    return int(book_bet_size(w, f - m_p) * max_pos)


def book_inv_price(f, w, m):
    return f - m * math.sqrt(w / (1 - m * m))                            # f - m (w / (1 - m^2))^.5


def book_limit_price(t_pos, pos, f, w, max_pos):
    sgn = 1 if t_pos >= pos else -1
    lp = 0
    for j in range(abs(pos + sgn), abs(t_pos + 1)):
        lp += book_inv_price(f, w, j / float(max_pos))
    lp /= t_pos - pos
    return lp


def book_get_w(x, m):
    return x ** 2 * (m ** -2 - 1)


# ---------------------------------------------------------------------------------------- case makers shared by the test files
UNIT_SIGNALS = [1.0, -1.0, 0.0, -0.0, 2.0 ** -31, -(2.0 ** -31), 3 * 2.0 ** -31, -3 * 2.0 ** -31, 2.0 ** -30, -(2.0 ** -30),
                1 - 2.0 ** -30, -(1 - 2.0 ** -30)]
STEPS = [1.0, 0.5, 0.1, 0.05, 1.0 / 3.0]


def random_case(rng, n, n_events, max_len=None):
    """spans inside [0, n) with some skipped labels (tc == ev) and repeats, signals mixed from the unit cases and random doubles."""
    max_len = max(1, n if max_len is None else max_len)
    ev = rng.integers(0, n, n_events)
    tc = np.minimum(ev + rng.integers(0, max_len + 1, n_events), n - 1)
    sig = rng.uniform(-1.0, 1.0, n_events)
    pick = rng.random(n_events) < 0.3
    sig[pick] = rng.choice(UNIT_SIGNALS, int(pick.sum()))
    if n_events > 3:
        ev[-1], tc[-1], sig[-1] = ev[0], tc[0], sig[0]                   # a repeated event
    return ev.astype(np.int64), tc.astype(np.int64), sig
