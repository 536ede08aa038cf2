#!/usr/bin/env python3
"""Writes tests/golden/shape_degenerate.npz + shape_degenerate.json: rolling kurtosis and the Hurst exponent on the inputs where a
window has no statistic, or where the statistic is badly conditioned -- held prices and held returns, whole-series constants, one odd
element in a constant series, series of period 2, 4, 8 and 3 (single lags of Hurst without a variance), prices offset by 1e5, 1e7
and 1e9, and one held-price case at the window whose span takes more than one slab.  Build container only: imports the reference
through oracle/shim, like tools/gen_shape_golden.py; no GPU, nothing of the product.

The truth is EXACT: every window is computed in rational arithmetic (fractions.Fraction / Python integers) on the float64 inputs.
Kurtosis w * sum(y^4) / sum(y^2)^2 - 3 with y = w x - sum(x) is rational throughout; of Hurst the four variances are rational and only
the logarithms and their linear combination are in float64.  A full finite window is of class `none` (exact m2 == 0, or some exact
tau_k == 0) or of class `value`.  The generator STOPS, it does not skip, when on any case
  * the exact class differs from the class that the rule of DESIGN.md section 7c3 gives on the float64 words (kurtosis: the w elements
    all compare equal; Hurst: for some lag the w - k tree sums all compare equal), or the restatement's NaN positions are not the head
    plus the `none` windows;
  * the reference is NaN on a `value` window;
  * the error of either form of tests/_shape_ref.py against the exact value exceeds 16 times the reference's own error on that case
    plus the statistic's tolerance of tests/golden/shape.json.
Per case it records the reference's output, the exact values, the class mask, both worst errors and how many `none` windows the
reference leaves finite (information only).  Per statistic and input family it records the tolerance: _shape_ref.tolerance_from of the
worst error of the vector form against the exact value (16 times, rounded up to a power of ten) -- never anything measured on a kernel.
At the long window the exact arithmetic gives the class mask only; the values there are compared with the restatement.
    python tools/gen_shape_degenerate_golden.py <reference checkout>
"""
import json
import math
import os
import sys
import warnings
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_shape_degenerate_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import finmlkit.feature.transforms as RT  # noqa: E402

from tests import _shape_ref as H  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
TRANSFORMS = {"kurtosis": RT.KurtosisTransform, "hurst": RT.HurstExponent}
WINDOWS = {"kurtosis": (2, 3, 5, 12, 32, 64, 100), "hurst": (9, 10, 12, 17, 24, 64, 100)}
TILE = {"kurtosis": 1024, "hurst": 512}                             # outputs per workgroup (csrc/fmk_shape.hip)
LONG_WINDOW = {"kurtosis": 4100, "hurst": 1100}                     # tests/test_gpu_shape.py: a tile's span takes more than one slab
BASE_TOLERANCE = {fn: t["tolerance"] for fn, t in json.load(open(os.path.join(GOLD, "shape.json")))["tolerances"].items()}
C_HURST = (-1.5, -0.5, 0.5, 1.5)


def reference(fn, x, window):
    t = TRANSFORMS[fn](window)
    frame = pd.DataFrame({t.requires[0]: x}, index=pd.date_range("2024-01-01", periods=len(x), freq="1min"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(t(frame, backend="pd").values, np.float64)


# ---------------------------------------------------------------------------------------------------- exact arithmetic
def integers(x):
    """The float64 values as integers over one common power-of-two denominator (which cancels out of both statistics)."""
    fr = [Fraction(float(v)) for v in x]
    den = max(f.denominator for f in fr)
    return [f.numerator * (den // f.denominator) for f in fr]


def exact_kurtosis(X, w, t):
    """None for a window without a kurtosis, else the correctly rounded exact value."""
    win = X[t - w + 1:t + 1]
    s = sum(win)
    y2 = [(w * v - s) ** 2 for v in win]
    a = sum(y2)
    if a == 0:
        return None
    return float(Fraction(w * sum(v * v for v in y2), a * a) - 3)


def exact_hurst(X, w, t):
    win = X[t - w + 2:t + 1]                                        # the w - 1 elements that enter a sum
    p = [0]
    for v in win:
        p.append(p[-1] + v)
    h = 0.0
    for c, k in zip(C_HURST, H.LAGS):
        d = [p[j + k] - p[j] for j in range(w - k)]
        n = w - k
        num = n * sum(v * v for v in d) - sum(d) ** 2               # n^2 times the population variance
        if num == 0:
            return None
        h += c * 0.5 * (math.log(num) - math.log(n * n))           # the common denominator cancels: the weights sum to 0
    return h / (5.0 * math.log(2.0))


def exact_none_only(fn, x, X, w):
    """The class mask without the values (the long window): run lengths of equal exact sums."""
    n = len(x)
    none = np.zeros(n, bool)
    p = [0]
    for v in X:
        p.append(p[-1] + v)
    for k in ((1,) if fn == "kurtosis" else H.LAGS):
        d = [None] * k + [p[i + 1] - p[i + 1 - k] for i in range(k, n)] if fn == "hurst" else list(X)
        run = [1] * n
        for i in range(1, n):
            if d[i] is not None and d[i] == d[i - 1]:
                run[i] = run[i - 1] + 1
        need = w if fn == "kurtosis" else w - k
        for t in range(w - 1, n):
            if run[t] >= need:
                none[t] = True
    return none


def rule_none(fn, x, w, t):
    """The class that the product's rule gives on the float64 words."""
    xs = x[t - w + 1:t + 1].tolist()
    if fn == "kurtosis":
        return all(v == xs[-1] for v in xs)
    for k in H.LAGS:
        d = [H._tree(xs[j + 1:j + k + 1]) for j in range(w - k)]
        if all(v == d[-1] for v in d):
            return True
    return False


# ---------------------------------------------------------------------------------------------------- the cases
def case(fn, family, window, source, long=False):
    return dict(fn=fn, family=family, window=window, source=source, long=long)


def edge_runs(fn, w):
    """A run of w + 50 across the first tile edge (output w - 1 + TILE) and one of w + 22 under lanes 63 / 64 of the first wave."""
    edge = w - 1 + TILE[fn]
    return [[edge - w - 25, w + 50], [54, w + 22]]


def value_seed(fn, w, seed, base):
    """The first of seed, seed + 100, ... whose offset series has a statistic in every window: at window 10 lag 8 has two sums, which
    are exactly equal wherever x[t] == x[t-8] while their float64 trees differ -- such an input is changed, as the rule is about the
    words the kernel holds."""
    if fn == "hurst" and w == H.HURST_MIN_WINDOW:
        return seed
    while True:
        X = integers(H.grid_normal(w + 150, seed, base, 100))
        if all((exact_kurtosis if fn == "kurtosis" else exact_hurst)(X, w, t) is not None for t in range(w - 1, len(X))):
            return seed
        seed += 100


def all_cases():
    out = {}
    for fn in ("kurtosis", "hurst"):
        for j, w in enumerate(WINDOWS[fn]):
            n = w - 1 + TILE[fn] + 60
            out[f"held_price.{fn}_w{w}"] = case(fn, "held_price", w, ["held_series", [n, 1700 + j, 100.0, 100, edge_runs(fn, w)]])
            out[f"held_return.{fn}_w{w}"] = case(fn, "held_return", w, ["held_series", [n, 1720 + j, 0.0, 100000, edge_runs(fn, w)]])
            for tag, base, seed in (("1e5", 1e5, 1740), ("1e7", 1e7, 1760)):
                out[f"offset.{fn}_{tag}_w{w}"] = case(fn, "offset_" + tag, w, ["grid_normal", [w + 150, value_seed(fn, w, seed + j, base), base, 100]])
        for tag, v in (("0.1", 0.1), ("99.55", 99.55), ("1e-4", 1e-4), ("-0.3", -0.3), ("1e300", 1e300), ("5e-324", 5e-324),
                       ("1e-160", 1e-160)):
            for w in ((5, 12) if fn == "kurtosis" else (10, 24)):
                out[f"constant.{fn}_{tag}_w{w}"] = case(fn, "constant", w, ["constant", [40, v]])
        for w in ((5, 32) if fn == "kurtosis" else (10, 24)):
            out[f"one_odd.{fn}_w{w}"] = case(fn, "one_odd", w, ["one_odd", [3 * w + 5, 99.55, w + 2, 100.07]])
        w = LONG_WINDOW[fn]
        n = w + TILE[fn] + 1
        out[f"long.{fn}_w{w}"] = case(fn, "long", w, ["held_series", [n, 1790, 100.0, 100, [[n - 15 - (w + 20), w + 20]]]], long=True)
    out["offset.kurtosis_1e9_w3"] = case("kurtosis", "offset_1e9", 3, ["levels", [400, 1780, 1e9, 100, 3]])
    for w in (12, 24, 100):
        out[f"period.hurst_p2_w{w}"] = case("hurst", "period", w, ["periodic", [w + 60, [99.55, 100.07]]])
    for w in (12, 24):
        out[f"period.hurst_p4_w{w}"] = case("hurst", "period", w, ["periodic", [w + 60, [99.5, 100.25, 99.75, 100.125]]])
        out[f"period.hurst_p8_w{w}"] = case("hurst", "period", w, ["periodic", [w + 60, [99.5, 100.25, 99.75, 100.125, 99.0, 101.5, 100.0,
                                                                                         98.75]]])
        out[f"period.hurst_p3_w{w}"] = case("hurst", "period", w, ["periodic", [w + 60, [99.55, 100.07, 99.81]]])
    return out


EXTREME = ("1e300", "5e-324", "1e-160")                             # kept only where the reference gives NaN too


def main():
    arrays, manifest, dropped = {}, {}, {}
    worst = {}
    for name, c in all_cases().items():
        fn, w = c["fn"], c["window"]
        x = np.asarray(H.generate(c["source"]), np.float64)
        n = len(x)
        first = w - 1
        ref = reference(fn, x.copy(), w)
        own = {form: H.call(fn, x.copy(), w, form) for form in ("vector", "scalar")}
        X = integers(x)
        exact = np.full(n, np.nan)
        if c["long"]:
            none = exact_none_only(fn, x, X, w)                     # the rule's class is read off the restatement below
        else:
            none = np.zeros(n, bool)
            for t in range(first, n):
                v = (exact_kurtosis if fn == "kurtosis" else exact_hurst)(X, w, t)
                none[t] = v is None
                if v is not None:
                    exact[t] = v
                if rule_none(fn, x, w, t) != none[t]:
                    raise SystemExit(f"{name}: window ending at {t} is exactly {'none' if none[t] else 'value'}, the rule says otherwise")
        value = np.zeros(n, bool)
        value[first:] = ~none[first:]
        want_nan = ~value
        for form, o in own.items():
            if not np.array_equal(np.isnan(o), want_nan):
                bad = np.nonzero(np.isnan(o) != want_nan)[0]
                raise SystemExit(f"{name}: the {form} form's NaN positions are not the head plus the none windows ({len(bad)}: {bad[:5]})")
        finite_on_none = int(np.isfinite(ref[none]).sum())
        if any(name.startswith(f"constant.{fn}_{tag}_") for tag in EXTREME):
            if finite_on_none:
                why = f"the reference is finite on {finite_on_none} of {int(none.sum())} windows"
                dropped[name] = {"fn": fn, "window": w, "source": c["source"], "reason": why, "reference_last": float(ref[-1])}
                print(name, "DROPPED:", why)
                continue
        if np.isnan(ref[value]).any():
            raise SystemExit(f"{name}: the reference is NaN on {int(np.isnan(ref[value]).sum())} value windows")
        entry = {"fn": fn, "family": c["family"], "window": w, "n": n, "source": c["source"], "input_sha256": H.sha256(x),
                 "none": int(none.sum()), "value": int(value.sum()), "reference_finite_on_none": finite_on_none}
        if c["long"]:
            entry["exact_values"] = False
        else:
            err = {k: (float(np.abs(o[value] - exact[value]).max()) if value.any() else 0.0)
                   for k, o in (("reference", ref), ("vector", own["vector"]), ("scalar", own["scalar"]))}
            for form in ("vector", "scalar"):
                if err[form] > 16.0 * err["reference"] + BASE_TOLERANCE[fn]:
                    raise SystemExit(f"{name}: the {form} form is {err[form]} from the exact value, the reference {err['reference']}")
            entry.update(err_reference=err["reference"], err_vector=err["vector"], err_scalar=err["scalar"])
            wf = worst.setdefault(fn, {}).setdefault(c["family"], {"reference": 0.0, "vector": 0.0, "scalar": 0.0})
            for k in wf:
                wf[k] = max(wf[k], err[k])
            arrays[name + ".exact"] = exact
        arrays[name + ".ref"] = ref
        arrays[name + ".none"] = np.packbits(none)
        manifest[name] = entry
        print(name, {k: v for k, v in entry.items() if k not in ("input_sha256", "source")})
    tolerances = {fn: {fam: {"err_reference": e["reference"], "err_vector": e["vector"], "err_scalar": e["scalar"],
                             "tolerance": H.tolerance_from(e["vector"])} for fam, e in fams.items()} for fn, fams in worst.items()}
    print(json.dumps(tolerances, indent=1))
    np.savez_compressed(os.path.join(GOLD, "shape_degenerate.npz"), **arrays)
    with open(os.path.join(GOLD, "shape_degenerate.json"), "w") as fh:
        json.dump({"tolerances": tolerances, "cases": manifest, "dropped": dropped}, fh, indent=1, sort_keys=True)
    size = sum(os.path.getsize(os.path.join(GOLD, "shape_degenerate" + e)) for e in (".npz", ".json"))
    limit = sum(os.path.getsize(os.path.join(GOLD, "shape" + e)) for e in (".npz", ".json"))
    print(len(manifest), "cases,", len(dropped), "dropped,", size, "bytes of", limit)
    if size > limit:
        raise SystemExit("the fixture is larger than shape.npz + shape.json")


if __name__ == "__main__":
    main()
