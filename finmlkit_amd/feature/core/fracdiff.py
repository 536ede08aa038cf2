"""Fractional differentiation with a fixed-width window ("FFD": Lopez de Prado, Advances in Financial Machine Learning, ch. 5) and the
causal FIR filter it runs on (csrc/fmk_fir.hip).  The reference has no such function; the definition is this project's (DESIGN.md
section 7k):

    w[0] = 1.0;  w[k] = ((-w[k-1]) * (d - (k - 1))) / k  in float64, up to and without the first |w[k]| < threshold
    y[t] = NaN for t < W - 1;  y[t] = acc after  acc = +0.0;  for k = W-1 .. 0: acc = fma(w[k], x~[t-k], acc)

with x~ = x where x is finite and NaN elsewhere: one correctly rounded fused multiply-add per tap, oldest tap first.  The weights are
computed here, on the host, once per call, and handed to the kernel: there is no second implementation of the recurrence."""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import DeviceArray, c_i64, c_vp, ptr
from .structural_break import adf

FIR_MAX_WIDTH = 8192                 # csrc/fmk_common.h: FMK_FIR_MAX_WIDTH
D_MESSAGE = "frac_diff: d must be finite and not negative."
THRESHOLD_MESSAGE = "frac_diff: threshold must be greater than 0 and less than 1."
WIDTH_MESSAGE = "frac_diff: more than 8192 weights reach the threshold; raise the threshold."
FIR_EMPTY_MESSAGE = "fir: at least one weight is needed."
FIR_MAX_WIDTH_MESSAGE = "fir: at most 8192 weights."
FIR_FINITE_MESSAGE = "fir: the weights must be finite."
FIR_ALIAS_MESSAGE = "fir: the output must not be the input."


def frac_diff_weights(d: float, threshold: float = 1e-5) -> NDArray[np.float64]:
    """The FFD weights of order `d`: w[k] multiplies x[t-k].  Pure Python floats (IEEE float64), no device and no library."""
    d, threshold = float(d), float(threshold)
    if not (math.isfinite(d) and d >= 0.0):
        raise ValueError(D_MESSAGE)
    if not 0.0 < threshold < 1.0:
        raise ValueError(THRESHOLD_MESSAGE)
    w = [1.0]
    while True:
        k = len(w)
        nxt = ((-w[-1]) * (d - (k - 1))) / k
        if abs(nxt) < threshold:
            return np.array(w, dtype=np.float64)
        if k == FIR_MAX_WIDTH:
            raise ValueError(WIDTH_MESSAGE)
        w.append(nxt)


def rule_fir(weights) -> NDArray[np.float64]:
    """What fir refuses about its weights, in the library's order (csrc/fmk_common.h: fmk_rule_fir) -> the weights as the library
    takes them; needs no device."""
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.size < 1:
        raise ValueError(FIR_EMPTY_MESSAGE)
    if w.size > FIR_MAX_WIDTH:
        raise ValueError(FIR_MAX_WIDTH_MESSAGE)
    if not np.isfinite(w).all():
        raise ValueError(FIR_FINITE_MESSAGE)
    return w


PROTOTYPE = [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]       # context, series, n, weights (host), width, output


@functools.lru_cache(maxsize=None)
def entries():
    """(fmk_fir, fmk_fir_dev) of the loaded library with restype and argtypes set."""
    fns = tuple(getattr(_ffi.lib(), name) for name in ("fmk_fir", "fmk_fir_dev"))
    for fn in fns:
        fn.restype, fn.argtypes = C.c_int, PROTOTYPE
    return fns


def geometry():
    """(outputs per workgroup, taps per staging pass) of the kernel (fmk_fir_geometry); needs no device."""
    out = (C.c_int64 * 2)()
    _ffi.check(_ffi.lib().fmk_fir_geometry(out))
    return int(out[0]), int(out[1])


def fir(x, weights) -> NDArray[np.float64]:
    """The causal filter y[t] = sum_k weights[k] * x[t-k] as the fold above; NaN before the first full window and wherever the window
    holds a NaN or an infinity.  The rule comes first; an empty series is answered without a device."""
    w = rule_fir(weights)
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(len(x), np.float64)
    if len(x):
        ctx = _ffi.default_context()
        _ffi.check(entries()[0](ctx.handle, ptr(x), len(x), ptr(w), w.size, ptr(out)), ctx.handle)
    return out


def frac_diff_ffd(x, d: float, threshold: float = 1e-5) -> NDArray[np.float64]:
    """`fir(x, frac_diff_weights(d, threshold))`: x differentiated to the order d over a fixed-width window."""
    return fir(x, frac_diff_weights(d, threshold))


def resident(ctx, y: DeviceArray, weights) -> DeviceArray:
    """fmk_fir_dev on a DeviceArray -> DeviceArray; `weights` stay on the host.  Rule and dtype are checked, in this order, before
    `ctx` or a pointer is looked at; an empty series is answered by an empty array that owns no memory."""
    w = rule_fir(weights)
    if y.dtype != np.float64:
        raise TypeError(f"fmk_fir_dev: the series must be float64, not {y.dtype}")
    if not y.n:
        return DeviceArray(ctx, 0, np.float64, dptr=0)
    out = DeviceArray(ctx, y.n, np.float64)
    _ffi.check(entries()[1](ctx.handle, y.p, y.n, ptr(w), w.size, out.p), ctx.handle)
    return out


ADF_CRIT_95 = -2.8623                # the 95 % critical value of the ADF test with a constant that the book's Table 5.1 quotes


def ffd_adf_stats(x, ds, threshold: float = 1e-5, lags: int = 1) -> NDArray[np.float64]:
    """The ADF statistic (constant, `lags` lagged differences) of frac_diff_ffd(x, d, threshold) for every d of `ds`, taken over the
    series from its first full window on (the leading NaN are left out; a NaN later on makes the statistic NaN, and so does a tail
    too short for one degree of freedom).  `x` goes up once; per d one fmk_fir_dev and one fmk_sadf_dev with a single end point run
    on the device and eight bytes come back."""
    ds = [float(d) for d in ds]
    weights = [frac_diff_weights(d, threshold) for d in ds]
    x = np.ascontiguousarray(x, dtype=np.float64)
    lags = adf.check_arguments(len(x), None, adf.MAX_LAGS + 3, None, lags, "c", 1)[2]      # (refuses lags outside 0..4)
    k = adf.regressors(lags, "c")
    stats = np.full(len(ds), np.nan)
    tails = [len(x) - (w.size - 1) for w in weights]                       # elements from the first full window on
    if not any(tail - lags - 1 >= k + 1 for tail in tails):
        return stats
    ctx = _ffi.default_context()
    d_x = DeviceArray.from_host(ctx, x)
    d_last = DeviceArray.from_host(ctx, np.array([max(tail - 1, 0) for tail in tails], np.int64))
    for i, (w, tail) in enumerate(zip(weights, tails)):
        rows = tail - lags - 1
        if rows < k + 1:
            continue
        y = resident(ctx, d_x, w).view(w.size - 1)
        stats[i] = adf.resident(ctx, y, d_last.view(i, 1), rows, rows, lags, "c", 1)[0].to_host()[0]
    return stats


def min_ffd_d(x, ds=np.linspace(0, 1, 11), threshold: float = 1e-5, lags: int = 1, crit: float = ADF_CRIT_95):
    """-> (d, stats): the first `d` of `ds` whose FFD series passes the ADF test, i.e. has a statistic below `crit`, or None when
    none has, and the statistic of every d (ffd_adf_stats; NaN never passes).  This is the book's search for the smallest order
    that makes a series stationary (ch. 5, Table 5.1).  `crit` defaults to -2.8623, the 95 % critical value that table quotes for a
    test with a constant; it depends on the sample size and on the deterministic terms (MacKinnon's tables), so pass your own for
    another level or a short series: this library computes no p-values."""
    ds = np.asarray(ds, dtype=np.float64).reshape(-1)
    stats = ffd_adf_stats(x, ds, threshold, lags)
    below = np.flatnonzero(stats < crit)
    return (float(ds[below[0]]) if below.size else None), stats
