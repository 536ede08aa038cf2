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


def one_sided(n, sign, lot=1.0):
    """Every side is `sign`, every lot is `lot`, prices are 1.0: with thr = K lot every link is exactly K ticks long."""
    return np.ones(n), np.full(n, lot, np.float32), np.full(n, sign, np.int8)


def closes_one_sided(n, K):
    """The closes of one_sided(n, +-1, lot) at thr = K lot, both rules, in closed form: tick 0 is counted but cannot close, so the
    first bar closes at K - 1 and every later one K ticks on (K = 1: tick 1 sees 2 lots and closes, then every tick does)."""
    if K == 1:
        return np.arange(n, dtype=np.int64)
    return np.concatenate([np.zeros(1, np.int64), np.arange(K - 1, n, K, dtype=np.int64)])


@functools.lru_cache(maxsize=None)
def biased(n, seed, p_up, p_zero, p_zero_lot):
    """(prices, float32 amounts, int8 sides): a share p_zero of the sides is 0, the others are +1 with probability p_up and -1
    otherwise; lots k / 64 with a share p_zero_lot of exact zeros; prices in quarters.  Every product is a multiple of 2^-8 and
    the tape's total stays far below 2^45, so the tape certifies as recipe() does."""
    rng = np.random.default_rng(seed)
    up = (1.0 - p_zero) * p_up
    sides = rng.choice([1, 0, -1], n, p=[up, p_zero, 1.0 - p_zero - up]).astype(np.int8)
    am = (rng.integers(1, 65, n) / 64).astype(np.float32)
    am[rng.random(n) < p_zero_lot] = 0.0
    px = np.abs(100.0 + rng.integers(-40, 41, n).cumsum() / 4.0) + 0.25
    for a in (px, am, sides):
        a.setflags(write=False)
    return px, am, sides


# recipe() has lots of k / 64.  Thresholds just below and just above 8, with the multiples of 1 / 64 they must act as, and two at
# and below one lot (every tick closes): (8 - 2^-10 like 8), (8 + 2^-10 like 8 + 1/64), 1/64, 1/128
ROUNDING_THR = (8.0 - 2.0 ** -10, 8.0, 8.0 + 2.0 ** -10, 8.0 + 1.0 / 64, 1.0 / 64, 1.0 / 128)
# (rule, thr, longest bar in ticks) on recipe(2^20 + 1), volume kind: links across many blocks whose summaries are not flat
LONG_BARS = (("imbalance", 64.0, 37513), ("imbalance", 256.0, 479378), ("run", 4096.0, 16173), ("run", 40000.0, 157525))

CERT_EDGE_THR = 2.0 ** 19
CERT_EDGE_AT = (3, 100, 600, 601, 1100, 1200, 1300, 1400, 1499)
CERT_EDGE_CLOSES = (0, 100, 600, 601, 1100, 1200, 1300, 1400)
CERT_EDGE_X = (2.0 ** 19 - 2.0 ** -29, 2.0 ** 19 - 2.0 ** -30)      # the last inside the certificate, the first outside it


def certificate_edge(X):
    """(prices, float64 amounts, int8 sides), 1500 ticks, for the volume kind at thr = 2^19.  Nine ticks have a side (+1 at odd
    positions, -1 at even ones) and the amounts 2^-30, seven times 2^20, X; all else is zero.  The quantum is 2^-30 and
    sum |x| + T = 2^-30 + 7 2^20 + X + 2^19: 2^23 - 2^-30 for X = 2^19 - 2^-29 (certifies: below 2^53 2^-30), exactly 2^23 for
    X = 2^19 - 2^-30 (does not).  Every sum on the way is exact in float64 in any order."""
    n = 1500
    am, sd = np.zeros(n), np.zeros(n, np.int8)
    for p, a in zip(CERT_EDGE_AT, [2.0 ** -30] + [2.0 ** 20] * 7 + [X]):
        am[p] = a
        sd[p] = 1 if p % 2 else -1
    return np.ones(n), am, sd


# ---------------------------------------------------------------------------------------------- the tapes written out by hand
NAN = float("nan")
# group -> (sides, sizes, thr, {rule: closes written out by hand}); tests/test_flowbars_host.py asserts the closes on the loops,
# tests/test_gpu_flowbars_edges.py runs every tape with both rules on the device
HAND_TAPES = {
    "tie": (
        # theta: 1, 2, 3 (== thr: close), 1, 0, -1, -2, -3 (== -thr: close), 1
        ([1, 1, 1, 1, -1, -1, -1, -1, 1], [1.0] * 9, 3.0, {"imbalance": [0, 2, 7]}),
        # up: 1, 2, 3 (close); then dn: 1, 2, 3 (close)
        ([1, 1, 1, -1, -1, -1, 1], [1.0] * 7, 3.0, {"run": [0, 2, 5]}),
        ([1, 1, 1], [1.0, 1.0, 0.999], 3.0, {"imbalance": [0]}),
    ),
    "side_zero": (
        ([1, 0, 0, 1, 0, 1], [1.0, 50.0, 50.0, 1.0, 50.0, 1.0], 3.0, {"imbalance": [0, 5], "run": [0, 5]}),
    ),
    "tick_zero": (
        # |x[0]| >= thr: no close at 0; tick 1 sees theta = 5 + 1 and closes
        ([1, 1, 1, 1], [5.0, 1.0, 1.0, 1.0], 3.0, {"imbalance": [0, 1]}),
        ([1, -1, 1, 1], [5.0, 1.0, 1.0, 1.0], 3.0, {"imbalance": [0, 1]}),           # theta = 4 at tick 1
        ([1, -1, -1, -1], [3.0, 1.0, 1.0, 1.0], 3.0, {"imbalance": [0]}),            # 2, 1, 0: tick 0 was counted
        ([-1, 1, 1], [5.0, 1.0, 1.0], 3.0, {"run": [0, 1]}),                         # dn = 5 from tick 0 closes at tick 1
        ([1], [5.0], 3.0, {"imbalance": [0], "run": [0]}),
        ([], [], 3.0, {"imbalance": [0], "run": [0]}),
    ),
    "sell_side": (
        # buys and sells alternate: neither total is a "run" of consecutive ticks, the sell total reaches 3 first; the imbalance
        # of the same tape never gets there
        ([1, -1, -1, 1, -1, 1], [0.5, 1.0, 1.0, 0.5, 1.0, 0.5], 3.0, {"run": [0, 4], "imbalance": [0]}),
    ),
    "nan_amount": (
        # imbalance: closes at 2, then theta is NaN for good.  run: up is NaN from tick 3 on and never closes; dn reaches 3 at
        # tick 6 and the close clears both; then up: 1, 2, 3
        ([1, 1, 1, 1, -1, -1, -1, 1, 1, 1], [1.0, 1.0, 1.0, NAN, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 3.0,
         {"imbalance": [0, 2], "run": [0, 2, 6, 9]}),
        # a side of 0 with a NaN size: 0 * NaN is NaN for the imbalance sum, and nothing for the run totals
        ([1, 0, 1, 1, 1], [1.0, NAN, 1.0, 1.0, 1.0], 3.0, {"imbalance": [0], "run": [0, 3]}),
    ),
}


def hand_tape_columns(sides, sizes, pad=0):
    """A hand-written tape as (prices, float32 amounts, int8 sides) for the volume kind, with `pad` ticks of side 0 (amount 1)
    appended: they change no state (a state that tick 0 alone left at the threshold closes at the first of them)."""
    am = np.concatenate([np.asarray(sizes, np.float32), np.ones(pad, np.float32)])
    sd = np.concatenate([np.asarray(sides, np.int8), np.zeros(pad, np.int8)])
    return np.ones(len(am)), am, sd
