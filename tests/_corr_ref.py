"""Plain restatement of the reference's rolling_price_volume_correlation (finmlkit/feature/core/correlation.py:10-111) in its own
evaluation order, in two forms: a sequential loop (`form="scalar"`: one window after the other, Python floats) and a NumPy form in
the kernel's order (`form="vector"`: vectorised over the outputs, looped over the position in the window, a pair with a NaN skipped
by `np.where(valid, s + v, s)`; what large GPU cases are compared with).  Every window is summed on its own, left to right from
0.0, one rounded addition per element -- Python's `sum` before 3.12 and what Numba compiles; from 3.12 on `sum` of floats is
compensated, so the restatement spells the loop out.  Reads nothing outside the repository.

    ret[0] = NaN; ret[i] = (price[i] - price[i-1]) / price[i-1] where neither is NaN and price[i-1] != 0, NaN otherwise
    out[t] = NaN for t < window and where ret[t] or volume[t] is NaN
    4 <= t < 10: up / incv / decv = no price[j+1] <= price[j] / no volume[j+1] <= volume[j] / no volume[j+1] >= volume[j] over
                 j = t - window + 1 .. t - 1; up and incv -> 1.0, else up and decv -> -1.0
    otherwise the pairs of j = t - window + 1 .. t without a NaN: fewer than 2 -> NaN; mr, mv = sr / cnt, sv / cnt; cov, qr, qv the
                 sums of dr * dv, dr * dr, dv * dv; qr > 0 and qv > 0 -> cov / (sqrt(qr) * sqrt(qv)) clamped to [-1, 1], else NaN"""
import hashlib
import math

import numpy as np

from tests._break_ref import grid_walk  # noqa: F401 -- part of this module's interface

WINDOW_MESSAGE = "window must be at least 1."
SHAPE_MESSAGE = "rolling_price_volume_correlation: price and volume must be one-dimensional and of the same length."
SPECIAL_LO, SPECIAL_HI = 4, 10       # the reference's special case holds for SPECIAL_LO <= t < SPECIAL_HI
NAN = math.nan


def dyadic_volumes(n, seed):
    """n seeded volumes on a 1/64 grid below 256 (integer arithmetic: every machine regenerates the same bits)."""
    return np.random.default_rng(seed).integers(1, 1 << 14, n) / 64.0


def mantissa_volumes(n, seed):
    """n seeded volumes below 1024 that use all 53 bits of the mantissa (integer arithmetic, exact conversion)."""
    return np.random.default_rng(seed).integers(1 << 52, 1 << 53, n).astype(np.float64) * 2.0 ** -43


GENERATORS = {"grid_walk": grid_walk, "dyadic_volumes": dyadic_volumes, "mantissa_volumes": mantissa_volumes}


def generate(source):
    """(price, volume) of a case's `source`: {"price": [generator, args], "volume": [generator, args]}."""
    return tuple(GENERATORS[source[k][0]](*source[k][1]) for k in ("price", "volume"))


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def _inputs(price, volume, window):
    if int(window) < 1:
        raise ValueError(WINDOW_MESSAGE)
    p, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (price, volume))
    if not (p.ndim == v.ndim == 1 and len(p) == len(v)):
        raise ValueError(SHAPE_MESSAGE)
    return p, v


def returns(price):
    """ret of the whole series (the vector form's and the tests')."""
    p = np.asarray(price, np.float64)
    r = np.full(len(p), np.nan)
    if len(p) > 1:
        with np.errstate(all="ignore"):
            c, b = p[1:], p[:-1]
            ok = ~np.isnan(c) & ~np.isnan(b) & (b != 0)
            r[1:] = np.where(ok, (c - np.where(ok, b, 1.0)) / np.where(ok, b, 1.0), np.nan)
    return r


def _special(ps, vs, window, t):
    """The special case at output t (its current position holds no NaN): 1.0, -1.0 or None."""
    up = incv = decv = True
    for j in range(t - window + 1, t):
        if ps[j + 1] <= ps[j]:
            up = False
        if vs[j + 1] >= vs[j]:
            decv = False
        if vs[j + 1] <= vs[j]:
            incv = False
    if up and incv:
        return 1.0
    if up and decv:
        return -1.0
    return None


def _scalar(p, v, window):
    n = len(p)
    out = np.full(n, np.nan)
    ps, vs = p.tolist(), v.tolist()
    ret = [NAN] * n
    for i in range(1, n):
        c, b = ps[i], ps[i - 1]
        if c == c and b == b and b != 0:
            ret[i] = (c - b) / b
    for t in range(window, n):
        if ret[t] != ret[t] or vs[t] != vs[t]:
            continue
        if SPECIAL_LO <= t < SPECIAL_HI:
            sp = _special(ps, vs, window, t)
            if sp is not None:
                out[t] = sp
                continue
        rs, ws = [], []
        for j in range(t - window + 1, t + 1):
            if ret[j] == ret[j] and vs[j] == vs[j]:
                rs.append(ret[j])
                ws.append(vs[j])
        cnt = len(rs)
        if cnt < 2:
            continue
        sr = sv = 0.0
        for k in range(cnt):
            sr = sr + rs[k]
            sv = sv + ws[k]
        mr, mv = sr / cnt, sv / cnt
        cov = qr = qv = 0.0
        for k in range(cnt):
            dr, dv = rs[k] - mr, ws[k] - mv
            cov = cov + dr * dv
            qr = qr + dr * dr
            qv = qv + dv * dv
        if qr > 0 and qv > 0:
            with np.errstate(all="ignore"):
                c = float(np.float64(cov) / np.float64(math.sqrt(qr) * math.sqrt(qv)))
            out[t] = 1.0 if c > 1.0 else (-1.0 if c < -1.0 else c)
    return out


def _vector(p, v, window):
    n = len(p)
    out = np.full(n, np.nan)
    m = n - window                                               # outputs window .. n - 1; output k reads pairs k + 1 .. k + window
    if m <= 0:
        return out
    ret = returns(p)
    ok_all = ~np.isnan(ret) & ~np.isnan(v)
    with np.errstate(all="ignore"):
        sr, sv, cnt = np.zeros(m), np.zeros(m), np.zeros(m, np.int64)
        for q in range(window):
            r, w, valid = ret[q + 1:q + 1 + m], v[q + 1:q + 1 + m], ok_all[q + 1:q + 1 + m]
            sr = np.where(valid, sr + r, sr)
            sv = np.where(valid, sv + w, sv)
            cnt += valid
        fc = cnt.astype(np.float64)
        mr, mv = sr / fc, sv / fc
        cov, qr, qv = np.zeros(m), np.zeros(m), np.zeros(m)
        for q in range(window):
            r, w, valid = ret[q + 1:q + 1 + m], v[q + 1:q + 1 + m], ok_all[q + 1:q + 1 + m]
            dr, dv = r - mr, w - mv
            cov = np.where(valid, cov + dr * dv, cov)
            qr = np.where(valid, qr + dr * dr, qr)
            qv = np.where(valid, qv + dv * dv, qv)
        c = cov / (np.sqrt(qr) * np.sqrt(qv))
        c = np.where(c > 1.0, 1.0, np.where(c < -1.0, -1.0, c))
        good = ok_all[window:] & (cnt >= 2) & (qr > 0) & (qv > 0)
        out[window:] = np.where(good, c, np.nan)
    ps, vs = p.tolist(), v.tolist()
    for t in range(max(window, SPECIAL_LO), min(SPECIAL_HI, n)):  # at most six outputs
        if ok_all[t]:
            sp = _special(ps, vs, window, t)
            if sp is not None:
                out[t] = sp
    return out


def rolling_price_volume_correlation(price, volume, window, form="vector"):
    p, v = _inputs(price, volume, window)
    return _scalar(p, v, int(window)) if form == "scalar" else _vector(p, v, int(window))
