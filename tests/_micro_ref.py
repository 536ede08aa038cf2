"""The per-bar microstructure features in NumPy and Python: the definition the HIP kernel is tested against.

Bar b holds the ticks s = ci[b] + 1 .. e = ci[b + 1].  The per-tick terms are float64, formed exactly as defined (math.log of the
rounded quotient and math.sqrt element by element: the library's log contract is the host libm's bits); `reference` sums the float64
terms in np.longdouble and evaluates the rules there, `restatement` sums them left to right in float64 and evaluates the rules in
float64 -- it exists to measure what another float64 summation order costs.  Nothing here reads outside the repository."""
import math

import numpy as np

COLS = ("kyle_lambda", "kyle_t", "amihud_lambda", "amihud_t", "hasbrouck_lambda", "hasbrouck_t", "serial_cov", "roll_spread")
REGS = ("kyle", "amihud", "hasbrouck")
EPS = 2.0 ** -53
EXACT_FIT = 2.0 ** -26
NAN = float("nan")


def _log(q):
    if q != q or q < 0.0:
        return NAN
    if q == 0.0:
        return -math.inf
    return math.log(q)


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN


def tick_terms(p, v, sd):
    """Tape-wide float64 terms, index t holding the term of tick t against tick t - 1 (index 0 unused); a bar uses s + 1 .. e of
    them and the products d_t d_{t-1} of s + 2 .. e only, so nothing crosses a bar's first tick."""
    p = np.asarray(p, np.float64)
    v = np.asarray(v).astype(np.float64)
    sd = np.asarray(sd).astype(np.float64)
    n = len(p)
    d, r, q = np.zeros(n), np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        d[1:] = p[1:] - p[:-1]
        quot = np.zeros(n)
        quot[1:] = p[1:] / p[:-1]
        r[1:] = [_log(x) for x in quot[1:].tolist()]
        xk = sd * v
        xa = p * v
        xh = sd * np.array([_sqrt(x) for x in xa.tolist()])
        q[2:] = d[2:] * d[1:-1]
        t = {"d": d, "r": r, "xk": xk, "xa": xa, "xh": xh, "q": q}
        ar = np.abs(r)
        t["prod"] = {"kyle": (xk * xk, xk * d, d * d), "amihud": (xa * xa, xa * ar, r * r), "hasbrouck": (xh * xh, xh * r, r * r)}
    return t


def _rules(m, sxx, sxy, syy, one, sqrt, inf):
    """-> (rule, lambda, t, u) in the arithmetic of the arguments"""
    if m < 2 or not (np.isfinite(sxx) and np.isfinite(sxy) and np.isfinite(syy)) or sxx == 0:
        return 1, NAN, NAN, NAN
    if syy == 0:
        return 2, 0.0, 0.0, NAN
    lam = sxy / sxx
    den = sxx * syy
    u = one - sxy * sxy / den
    if u <= EXACT_FIT:
        return 3, lam, (inf if not np.signbit(sxy) else -inf), u
    return 4, lam, sxy / sqrt(den) * sqrt((m - 1) / u), u


def _evaluate(p, v, sd, ci, longdouble):
    t = tick_terms(p, v, sd)
    ci = np.asarray(ci, np.int64)
    nb = max(len(ci) - 1, 0)
    ft = np.longdouble if longdouble else np.float64
    out = {k: np.full(nb, NAN, ft) for k in COLS}
    aux = {"m": np.zeros(nb, np.int64), "qabs": np.zeros(nb, np.longdouble)}
    for g in REGS:
        aux[g] = {k: np.full(nb, NAN, np.longdouble) for k in ("Sxx", "Sxy", "Syy", "u")}
        aux[g]["rule"] = np.zeros(nb, np.int64)
    if longdouble:
        total = lambda a: a.astype(np.longdouble).sum() if len(a) else np.longdouble(0)
        one, sqrt, inf = np.longdouble(1), np.sqrt, np.longdouble(np.inf)
    else:
        total = lambda a: np.cumsum(a)[-1] if len(a) else np.float64(0)        # cumsum adds left to right; np.float64 scalars: IEEE, no raise
        one, sqrt, inf = np.float64(1), np.sqrt, np.float64(np.inf)
    with np.errstate(all="ignore"):
        for b in range(nb):
            s, e = int(ci[b]) + 1, int(ci[b + 1])
            m = e - s
            aux["m"][b] = m
            for g in REGS:
                xx, xy, yy = (total(a[s + 1:e + 1]) for a in t["prod"][g])
                rule, lam, tv, u = _rules(m, xx, xy, yy, one, sqrt, inf)
                out[g + "_lambda"][b], out[g + "_t"][b] = lam, tv
                a = aux[g]
                a["Sxx"][b], a["Sxy"][b], a["Syy"][b], a["u"][b], a["rule"][b] = xx, xy, yy, u, rule
            if m >= 2:
                qs = t["q"][s + 2:e + 1]
                gamma = total(qs) / (m - 1)
                aux["qabs"][b] = np.abs(qs).astype(np.longdouble).sum()
                out["serial_cov"][b] = gamma
                out["roll_spread"][b] = 2 * sqrt(-gamma) if gamma < 0 else (0.0 if gamma >= 0 else NAN)
    out["aux"] = aux
    return out


def reference(p, v, sd, ci):
    """longdouble sums of the float64 terms, rules in longdouble -> {column: longdouble[nb], "aux": moments, rules, u, m, sum |q|}"""
    return _evaluate(p, v, sd, ci, True)


def restatement(p, v, sd, ci):
    """float64 left-to-right sums, rules in float64 -> {column: float64[nb], ...}"""
    return _evaluate(p, v, sd, ci, False)


def roll_of(gamma):
    """roll_spread as the stated float64 function of a serial_cov column"""
    return np.array([2.0 * math.sqrt(-g) if g < 0 else (0.0 if g >= 0 else NAN) for g in np.asarray(gamma, np.float64).tolist()])


def lambda_bound(ref, g):
    a, m = ref["aux"][g], ref["aux"]["m"]
    with np.errstate(all="ignore"):
        return 4 * m.astype(np.longdouble) * EPS * np.sqrt(a["Syy"] / a["Sxx"])


def gamma_bound(ref):
    m = ref["aux"]["m"].astype(np.longdouble)
    with np.errstate(all="ignore"):
        return 2 * m * EPS * ref["aux"]["qabs"] / (m - 1)


def t_errors(got, ref, bars=None):
    """relative errors of the finite nonzero t-values of rule 4 (of the bars of the mask `bars`), all three regressions in one array"""
    errs = []
    for g in REGS:
        w = ref[g + "_t"]
        sel = (ref["aux"][g]["rule"] == 4) & np.isfinite(w) & (w != 0)
        sel = sel if bars is None else sel & np.asarray(bars, bool)
        x = np.asarray(got[g + "_t"])[sel].astype(np.longdouble)
        errs.append(np.abs(x - w[sel]) / np.abs(w[sel]))
    return np.concatenate(errs) if errs else np.zeros(0, np.longdouble)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def assert_equal(got, ref, t_tol, what="", t_bars=None):
    """`got` (eight float64 arrays, a dict or a tuple in COLS order) equals the reference in the sense of DESIGN.md §7m: NaN
    positions, +-inf and the exact 0.0 of rule 2 bit for bit; roll_spread bit for bit the function of the returned serial_cov;
    serial_cov and lambda inside their derived bounds; finite t-values within t_tol relative (t_bars: a mask of the bars whose
    t-values the measured tolerance speaks for -- hand-built bars with a sum that cancels are not among them)."""
    if not isinstance(got, dict):
        got = dict(zip(COLS, got))
    nb = len(ref["aux"]["m"])
    for k in COLS:
        assert np.asarray(got[k]).dtype == np.float64 and len(got[k]) == nb, (what, k)
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k].astype(np.float64))), (what, k, "NaN positions")
    for g in REGS:
        rule = ref["aux"][g]["rule"]
        lam, tv = np.asarray(got[g + "_lambda"]), np.asarray(got[g + "_t"])
        z = rule == 2
        assert not lam[z].any() and not tv[z].any() and not np.signbit(lam[z]).any() and not np.signbit(tv[z]).any(), (what, g, "rule 2")
        x = rule == 3
        assert np.array_equal(tv[x], ref[g + "_t"][x].astype(np.float64)), (what, g, "exact fits")
        assert not np.isinf(tv[rule == 4]).any(), (what, g, "an infinite t-value outside rule 3")
        f = rule >= 3
        err = np.abs(lam[f].astype(np.longdouble) - ref[g + "_lambda"][f])
        bound = lambda_bound(ref, g)[f]
        assert np.all(err <= bound), (what, g, "lambda", float(np.max(err / bound)))
    te = t_errors(got, ref, t_bars)
    assert len(te) == 0 or float(te.max()) <= t_tol, (what, "t-values", float(te.max()), t_tol)
    gam = np.asarray(got["serial_cov"])
    f = ~np.isnan(gam)
    err = np.abs(gam[f].astype(np.longdouble) - ref["serial_cov"][f])
    assert np.all(err <= gamma_bound(ref)[f]), (what, "serial_cov")
    assert same_bits(got["roll_spread"], roll_of(gam)), (what, "roll_spread is not the function of the returned serial_cov")
