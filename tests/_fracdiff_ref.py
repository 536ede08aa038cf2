"""The oracle of the fractional differentiation and the causal FIR filter, restated independently of
finmlkit_amd/feature/core/fracdiff.py and of the kernel.

    w[0] = 1.0;  w[k] = ((-w[k-1]) * (d - (k - 1))) / k,  up to and without the first |w[k]| < threshold
    y[t] = NaN for t < W - 1;  y[t] = acc after  acc = +0.0;  for k = W-1 .. 0: acc = fma(w[k], x~[t-k], acc)

The fused step is DEFINED as `float(Fraction(w) * Fraction(x) + Fraction(acc))` (Python rounds a Fraction to float correctly); a NaN
or an infinity among the operands gives NaN.  That form costs about 8 microseconds per tap, so `fir_ref` takes the host libm's `fma`
through ctypes by default; tests/test_fracdiff_host.py shows the two agree bit for bit first (the sign of an exact zero aside, which
a Fraction cannot carry: no case here reaches one)."""
import ctypes
import ctypes.util
import math
from fractions import Fraction

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double]


def fma_libm(a, b, c):
    return _libm.fma(a, b, c)


def fma_fraction(a, b, c):
    """The definition: one correctly rounded a * b + c."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return math.nan
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def weights_ref(d, threshold=1e-5, limit=1 << 20):
    """The weight recurrence in Python floats."""
    w = [1.0]
    while len(w) < limit:
        k = len(w)
        nxt = ((-w[k - 1]) * (d - (k - 1))) / k
        if abs(nxt) < threshold:
            break
        w.append(nxt)
    return w


def fir_ref(x, w, fma=fma_libm):
    """The fold, output by output.  -> float64 array of len(x)."""
    xs = [float(v) if math.isfinite(v) else math.nan for v in np.asarray(x, dtype=np.float64)]
    ws = [float(v) for v in w]
    width, n = len(ws), len(xs)
    out = np.full(n, np.nan)
    taps = list(range(width - 1, -1, -1))
    for t in range(width - 1, n):
        acc = 0.0
        for k in taps:
            acc = fma(ws[k], xs[t - k], acc)
        out[t] = acc
    return out


def products(n, width):
    """Tap-products the oracle forms for a series of n elements."""
    return max(0, n - width + 1) * width


def bits_equal(got, want):
    """NaN positions exactly, every other output bit for bit."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64)))


# ---------------------------------------------------------------------------------------------- seeded inputs
def log_price_walk(n, seed):
    """ln of a price that starts at 100 and moves by seeded steps of about ten basis points."""
    rng = np.random.default_rng(seed)
    return np.log(100.0) + np.cumsum(rng.standard_normal(n) * 1e-3)


def mantissa_returns(n, seed):
    """Seeded returns of either sign within +-2^-9 that use all 53 bits of the mantissa: no product or sum of a window is exact."""
    rng = np.random.default_rng(seed)
    k = rng.integers(1 << 52, 1 << 53, n).astype(np.float64) * 2.0 ** -62
    return np.where(rng.integers(0, 2, n) == 1, k, -k)


def random_weights(width, seed):
    """Seeded finite weights of mixed sign, magnitudes 1e-8 .. 1e3."""
    rng = np.random.default_rng(seed)
    return np.where(rng.integers(0, 2, width) == 1, 1.0, -1.0) * 10.0 ** rng.uniform(-8.0, 3.0, width)


def fma_triples(seed, count=2500):
    """4 * count seeded (a, b, c): full-mantissa operands over a wide range of exponents; c cancelling the rounded product, so that
    the result is the product's rounding error; subnormal results; exact ties (1 + an odd multiple of 2^-53)."""
    rng = np.random.default_rng(seed)

    def mant(m):
        s = np.where(rng.integers(0, 2, m) == 1, 1.0, -1.0)
        return s * rng.integers(1 << 52, 1 << 53, m).astype(np.float64) * 2.0 ** -52

    a = mant(count) * 2.0 ** rng.integers(-40, 40, count)
    b = mant(count) * 2.0 ** rng.integers(-40, 40, count)
    c = mant(count) * 2.0 ** rng.integers(-80, 80, count)
    out = list(zip(a, b, c))
    out += [(p, q, -(p * q)) for p, q in zip(a, b)]
    sa, sb = mant(count) * 2.0 ** -520, mant(count) * 2.0 ** rng.integers(-545, -505, count)
    sc = mant(count) * 2.0 ** rng.integers(-1074, -1030, count)                      # subnormal or nearly so
    out += list(zip(sa, sb, sc))
    p = (2 * rng.integers(0, 1 << 24, count) + 1).astype(np.float64)
    q = (2 * rng.integers(0, 1 << 24, count) + 1).astype(np.float64)
    sign = np.where(rng.integers(0, 2, count) == 1, 1.0, -1.0)
    out += list(zip(sign * p * 2.0 ** -30, q * 2.0 ** -23, sign))                    # +-(1 + p q 2^-53), p q odd and < 2^50
    return [(float(u), float(v), float(z)) for u, v, z in out]
