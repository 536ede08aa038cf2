"""The optimal-trading-rule mesh restated in Python, independent of csrc/fmk_otr_rule.h: Python integers for
the counter words, math.log / math.sqrt on Python floats for the polar pair (the host's logarithm, which the device's is by the
project's standing contract), NumPy element-wise float64 operations for a step of all paths, the book's literal rule for a node's
exit (the first index where cp > pt or cp < -sl, else the last) and plain += loops in the definition's block order for the sums."""
import functools
import math

import numpy as np

M64 = (1 << 64) - 1
ATTEMPTS = 64


def word(seed, index):
    """splitmix64 at the counter index + 1 (the bootstrap's word)."""
    z = (seed + (index + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def index(p, k, a, w):
    return ((((p << 12) | k) << 6 | a) << 1) | w


def uniform(wd):
    return float(wd >> 11) * 2.0 ** -52 - 1.0


def pair(seed, p, k):
    """-> (z0, z1, attempts made); attempts = ATTEMPTS + 1 when none was accepted."""
    for a in range(ATTEMPTS):
        u, v = uniform(word(seed, index(p, k, a, 0))), uniform(word(seed, index(p, k, a, 1)))
        uu, vv = u * u, v * v
        s = uu + vv
        if s < 1.0 and s != 0.0:
            f = math.sqrt((-2.0 * math.log(s)) / s)
            return u * f, v * f, a + 1
    return 0.0, 0.0, ATTEMPTS + 1


@functools.lru_cache(maxsize=None)
def _normals(seed, n_paths, max_hp):
    z = np.empty((n_paths, max_hp), np.float64)
    att = np.empty((n_paths, (max_hp + 1) // 2), np.int64)
    for p in range(n_paths):
        for k in range((max_hp + 1) // 2):
            z0, z1, a = pair(seed, p, k)
            z[p, 2 * k] = z0
            if 2 * k + 1 < max_hp:
                z[p, 2 * k + 1] = z1
            att[p, k] = a
    z.setflags(write=False)
    att.setflags(write=False)
    return z, att


def normals(seed, n_paths, max_hp):
    """The generator's variates, (n_paths, max_hp) float64, read-only and shared among the callers."""
    return _normals(seed & M64, n_paths, max_hp)[0]


def attempts(seed, n_paths, max_hp):
    return _normals(seed & M64, n_paths, max_hp)[1]


def paths(forecast, phi, sigma, z):
    """-> P of shape (n_paths, max_hp): P[:, h-1] = P_h, every operation a NumPy float64 operation of its own."""
    forecast, phi, sigma = np.float64(forecast), np.float64(phi), np.float64(sigma)
    c0 = (np.float64(1.0) - phi) * forecast
    out = np.empty(z.shape, np.float64)
    P = np.zeros(z.shape[0], np.float64)
    for h in range(z.shape[1]):
        drift = phi * P
        mean = c0 + drift
        shock = sigma * z[:, h]
        P = mean + shock
        out[:, h] = P
    return out


def node_exits(P, pt, sl):
    """The book's rule for one node on every path -> (x, step 1 .. max_hp, kind 0 profit / 1 stop / 2 time)."""
    hit_p, hit_s = P > pt, P < -sl
    hit = hit_p | hit_s
    any_hit = hit.any(axis=1)
    first = np.where(any_hit, hit.argmax(axis=1), P.shape[1] - 1)
    rows = np.arange(P.shape[0])
    kind = np.where(any_hit & hit_p[rows, first], 0, np.where(any_hit & hit_s[rows, first], 1, 2))
    return P[rows, first], first + 1, kind


def block_sums(x, B):
    """S1, S2 of one node: block partials in path order, then the partials in block order -- plain Python floats."""
    S1 = S2 = 0.0
    for b0 in range(0, len(x), B):
        s1 = s2 = 0.0
        for v in x[b0:b0 + B].tolist():
            s1 += v
            s2 += v * v
        S1 += s1
        S2 += s2
    return S1, S2


def stats(S1, S2, n):
    mean = S1 / n
    var = S2 / n - mean * mean
    if var < 0.0:
        var = 0.0
    std = math.sqrt(var)
    if std == 0.0:                         # IEEE division (std is +0.0): 0/0 NaN, x/0 +-inf
        sharpe = math.nan if (mean == 0.0 or mean != mean) else math.copysign(math.inf, mean)
    else:
        sharpe = mean / std
    return mean, std, sharpe


def mesh(forecast, phi, sigma, pt, sl, max_hp, n_paths, seed, B, z=None):
    """The seven outputs, each (n_cfg, n_pt, n_sl), for parameter sets given as equal-length sequences."""
    forecast, phi, sigma = (np.atleast_1d(np.asarray(v, np.float64)) for v in (forecast, phi, sigma))
    pt, sl = np.asarray(pt, np.float64), np.asarray(sl, np.float64)
    z = normals(seed, n_paths, max_hp) if z is None else np.asarray(z, np.float64)
    shape = (len(forecast), len(pt), len(sl))
    out = {k: np.empty(shape, np.float64) for k in ("mean", "std", "sharpe")}
    out.update({k: np.empty(shape, np.int64) for k in ("n_profit", "n_stop", "n_time", "hold")})
    for c in range(shape[0]):
        P = paths(forecast[c], phi[c], sigma[c], z)
        for i in range(shape[1]):
            for j in range(shape[2]):
                x, step, kind = node_exits(P, pt[i], sl[j])
                S1, S2 = block_sums(x, B)
                out["mean"][c, i, j], out["std"][c, i, j], out["sharpe"][c, i, j] = stats(S1, S2, float(n_paths))
                out["n_profit"][c, i, j] = int((kind == 0).sum())
                out["n_stop"][c, i, j] = int((kind == 1).sum())
                out["n_time"][c, i, j] = int((kind == 2).sum())
                out["hold"][c, i, j] = int(step.sum())
    return out


def simulate(forecast, phi, sigma, n, seed, start=0.0):
    """One O-U series of n prices from the generator's variates of path 0 (for ou_fit)."""
    z = normals(seed, 1, n - 1)[0]
    p = np.empty(n, np.float64)
    p[0] = start
    for t in range(1, n):
        p[t] = (1.0 - phi) * forecast + phi * p[t - 1] + sigma * z[t - 1]
    return p
