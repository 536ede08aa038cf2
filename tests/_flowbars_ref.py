"""The loops that DEFINE imbalance and run bars with a fixed threshold (DESIGN.md section 6 "Imbalance and run bars"), in plain Python
on lists of floats, the tapes the tests share, and the exactness certificate restated on the host with NumPy.

The run rule's max(up, dn) >= thr is written as two comparisons, `up >= thr or dn >= thr`: a NaN total never closes a bar, the
other side still does (and the close clears both).  The kernels keep to this form."""
import functools
import math

import numpy as np

KINDS = ("tick", "volume", "dollar")


def sizes(kind, prices, amounts):
    """float64 size of every tick: 1, the amount, or price * amount as ONE float64 product."""
    a = np.asarray(amounts).astype(np.float64)
    if kind == "tick":
        return np.ones(len(a))
    if kind == "volume":
        return a
    assert kind == "dollar"
    return np.asarray(prices, dtype=np.float64) * a


def imbalance(b, q, thr):
    n = len(b)
    out = [0]
    if n == 0:
        return out
    theta = b[0] * q[0]
    for i in range(1, n):
        theta += b[i] * q[i]
        if math.fabs(theta) >= thr:
            out.append(i)
            theta = 0.0
    return out


def run(b, q, thr):
    n = len(b)
    out = [0]
    if n == 0:
        return out
    up = q[0] if b[0] > 0 else 0.0
    dn = q[0] if b[0] < 0 else 0.0
    for i in range(1, n):
        if b[i] > 0:
            up += q[i]
        elif b[i] < 0:
            dn += q[i]
        if up >= thr or dn >= thr:
            out.append(i)
            up = dn = 0.0
    return out


RULES = {"imbalance": imbalance, "run": run}


def closes(rule, kind, prices, amounts, sides, thr):
    """int64 close indices of the loop for `rule` on NumPy columns."""
    q = sizes(kind, prices, amounts)
    return np.array(RULES[rule]([int(s) for s in np.asarray(sides)], q.tolist(), float(thr)), np.int64)


# ---------------------------------------------------------------------------------------------- the certificate, on the host
def low_bit_exp(x):
    """Binary exponent of the lowest set bit of every nonzero finite float64 (None when all are zero): the tape's quantum."""
    x = np.asarray(x, np.float64)
    x = x[x != 0.0]
    if len(x) == 0:
        return None
    bits = x.view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    m = bits & np.uint64((1 << 52) - 1)
    m = np.where(e > 0, m | np.uint64(1 << 52), m)
    low = (m & (~m + np.uint64(1))).astype(np.float64)              # the lowest set bit as a number: a power of two, exact
    tz = np.log2(low).astype(np.int64)
    return int((np.where(e > 0, e - 1075, -1074) + tz).min())


def certifies(rule, kind, prices, amounts, sides, thr):
    """What the tables rung's certificate decides for this tape: every increment is a multiple of q = 2^e, and
    sum |x| + ceil(thr / q) q < 2^53 q.  Increments: side * size (imbalance), the size of every tick with a side (run)."""
    q = sizes(kind, prices, amounts)
    s = np.asarray(sides).astype(np.float64)
    x = s * q if rule == "imbalance" else np.where(s != 0, q, 0.0)
    e = low_bit_exp(x)
    if e is None:
        e = 0
    total = math.fsum(np.abs(x).tolist())
    c = max(math.ceil(math.ldexp(thr, -e)), 1)
    return total + math.ldexp(c, e) < math.ldexp(1.0, 53 + e)


# ---------------------------------------------------------------------------------------------- the tapes
@functools.lru_cache(maxsize=None)
def recipe(n, lots="dyadic"):
    """(prices, float32 amounts, int8 sides) of the issue's recipe: sides +-1, lots k / 64 (dyadic) or k / 1000 (milli)."""
    rng = np.random.default_rng(7)
    sides = rng.choice([-1, 1], n).astype(np.int8)
    if lots == "dyadic":
        am = (rng.integers(1, 65, n) / 64).astype(np.float32)
    elif lots == "milli":
        am = (rng.integers(1, 1000, n) / 1000).astype(np.float32)
    else:
        assert lots == "unit"
        am = np.ones(n, np.float32)
    px = 100.0 + rng.integers(-40, 41, n).cumsum() / 4.0            # dyadic prices: multiples of 1/4
    px = np.abs(px) + 0.25
    for a in (px, am, sides):
        a.setflags(write=False)
    return px, am, sides


def with_quiet_stretch(cols, at, length):
    """The tape with `length` ticks of side 0 inserted in front of tick `at` (prices and amounts repeat the tick before)."""
    px, am, sd = cols
    return (np.concatenate([px[:at], np.full(length, px[at - 1]), px[at:]]),
            np.concatenate([am[:at], np.full(length, am[at - 1], am.dtype), am[at:]]),
            np.concatenate([sd[:at], np.zeros(length, np.int8), sd[at:]]))


def shifted(idx, at, length):
    """Close indices of a tape after `length` ticks that change no state were inserted in front of tick `at`."""
    idx = np.asarray(idx, np.int64)
    return np.where(idx >= at, idx + length, idx)
