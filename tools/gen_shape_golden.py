#!/usr/bin/env python3
"""Writes tests/golden/shape.npz + shape.json: outputs of the REFERENCE's KurtosisTransform, TrendSlope, HurstExponent and
BiPowerVariation (finmlkit/feature/transforms.py:900-933, :936-988, :1341-1397, :1551-1602) on seeded series that the tests
regenerate (tests/_shape_ref.py: grid walks for the prices, returns on a dyadic grid with a few 30-fold jumps, and returns that use
the whole mantissa), on series with NaN, infinities and refused prices at the edges of a window, on constant windows of zeros and
dyadic values, on the edge lengths, and the refused arguments.  Build container only: imports the reference through oracle/shim,
like tools/gen_recur_golden.py; no GPU, nothing of the product.

The truth is the UNTOUCHED reference.  A case is refused unless the reference and both forms of tests/_shape_ref.py agree on every NaN
position.  The values are compared within a tolerance that is measured here, never from a kernel's output: per statistic the largest
deviation of the vector form (the kernel's order) from the reference over all cases -- absolute for kurtosis, hurst and slope (in
degrees), relative for bipower -- times 16, rounded up to a power of ten.  shape.json records both under "tolerances", and per case
the deviations of both forms.  The inputs of seeded cases are recorded as digests only.
    python tools/gen_shape_golden.py <reference checkout>
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_shape_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import finmlkit.feature.transforms as RT  # noqa: E402

from tests import _shape_ref as H  # noqa: E402

TRANSFORMS = {"kurtosis": RT.KurtosisTransform, "slope": RT.TrendSlope, "hurst": RT.HurstExponent, "bipower": RT.BiPowerVariation}
NAMES = {"kurtosis": "ret1_kurt_{w}", "slope": "close_trend_slope_{w}", "hurst": "ret1_hurst{w}", "bipower": "ret1_bv_{w}"}
WINDOWS = {"kurtosis": (2, 3, 4, 32, 64, 65, 257), "slope": (2, 3, 24, 64, 65, 300), "hurst": (9, 10, 11, 24, 64, 65, 300),
           "bipower": (1, 2, 3, 12, 64, 65, 300)}
N_WALK = 1000
INF = np.inf


def reference(fn, x, window):
    """The reference's transform on the default column, its pandas backend (the other one falls back to it)."""
    t = TRANSFORMS[fn](window)
    frame = pd.DataFrame({t.requires[0]: x}, index=pd.date_range("2024-01-01", periods=len(x), freq="1min"))
    s = t(frame, backend="pd")
    if s.name != NAMES[fn].format(w=window):
        raise SystemExit(f"{fn}: the reference names its output {s.name}")
    return np.asarray(s.values, np.float64)


def case(fn, window, x=None, source=None):
    return dict(fn=fn, window=window, x=np.asarray(H.generate(source) if source else x, np.float64), source=source)


def series_for(fn, n, seed):
    return ["grid_walk", [n, seed]] if fn == "slope" else ["dyadic_returns", [n, seed]]


def walk_cases():
    out = {}
    for k, fn in enumerate(H.FUNCTIONS):
        for j, w in enumerate(WINDOWS[fn]):
            out[f"walk.{fn}_w{w}"] = case(fn, w, source=series_for(fn, N_WALK, 1300 + 10 * k + j))
    for j, (fn, w) in enumerate((("kurtosis", 32), ("hurst", 10), ("hurst", 24), ("bipower", 12), ("bipower", 64), ("bipower", 300))):
        out[f"mantissa.{fn}_w{w}"] = case(fn, w, source=["mantissa_returns", [N_WALK, 1380 + j]])    # nothing sums exactly
    out["walk.kurtosis_w1"] = case("kurtosis", 1, source=series_for("kurtosis", 60, 1390))      # m2 == 0: NaN everywhere
    out["walk.slope_w1"] = case("slope", 1, source=series_for("slope", 60, 1391))
    out["held.slope_w5"] = case("slope", 5, source=["grid_walk", [400, 1392, 35, 0.8]])          # runs of equal prices
    return out


def edge_cases():
    """A value the window refuses in its first and in its last position (and for hurst in the first, which enters no difference)."""
    out = {}
    bad = {"kurtosis": (np.nan, INF, -INF), "hurst": (np.nan, INF, -INF), "bipower": (np.nan, INF, -INF),
           "slope": (np.nan, INF, -INF, 0.0, -0.0, -1.5)}
    for k, fn in enumerate(H.FUNCTIONS):
        for w in (12, 33):
            x = np.array(H.generate(series_for(fn, 80 * len(bad[fn]) + 100, 1400 + k)))
            for j, v in enumerate(bad[fn]):
                x[60 + 80 * j] = v
            out[f"edge.{fn}_w{w}"] = case(fn, w, x=x)
        x = np.array(H.generate(series_for(fn, 200, 1410 + k)))
        x[[0, 70, 71, 199]] = (np.nan, INF, 0.0 if fn != "slope" else 101.25, np.nan)
        out[f"edge.{fn}_ends_w10"] = case(fn, 10, x=x)
    x = np.array(H.dyadic_returns(120, 1420))
    x[40], x[41], x[80], x[81] = INF, 0.0, 0.0, -INF                    # inf times zero, and zero times inf
    out["edge.bipower_inf_zero_w4"] = case("bipower", 4, x=x)
    return out


def const_cases():
    out = {}
    for tag, v in (("zeros", 0.0), ("half", 0.5), ("three", 3.0)):
        for fn, w in (("kurtosis", 5), ("hurst", 10), ("bipower", 5)):
            out[f"const.{fn}_{tag}_w{w}"] = case(fn, w, x=np.full(40, v))
    for tag, v in (("100", 100.0), ("half", 0.5)):
        out[f"const.slope_{tag}_w5"] = case("slope", 5, x=np.full(40, v))
    x = np.array(H.dyadic_returns(90, 1430))
    x[30:60] = 0.5                                                      # a constant stretch inside a walk
    for fn, w in (("kurtosis", 7), ("hurst", 12), ("bipower", 7)):
        out[f"const.{fn}_stretch_w{w}"] = case(fn, w, x=x)
    return out


def length_cases():
    out = {}
    for k, fn in enumerate(H.FUNCTIONS):
        for w in (1, 9, 12):
            if fn == "hurst" and w < H.HURST_MIN_WINDOW:
                continue
            for n in sorted({1, 2, w - 1, w, w + 1, w + 2} - {0}):
                out[f"length.{fn}_n{n}_w{w}"] = case(fn, w, x=H.generate(series_for(fn, max(n, 2), 1440 + k))[:n])
    return out


def refused_cases():
    out = {}
    for k, fn in enumerate(H.FUNCTIONS):
        for w in (0, -1):
            out[f"refused.{fn}_w{w}"] = case(fn, w, x=H.generate(series_for(fn, 40, 1450 + k)))
    for w in (1, 8):
        out[f"refused.hurst_w{w}"] = case("hurst", w, x=H.dyadic_returns(40, 1454))
    return out


def run(f, *a):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return ("ok", np.asarray(f(*a), np.float64))
    except Exception as e:                                             # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))


def main():
    out, manifest = {}, {}
    cases = {}
    for group in (walk_cases, edge_cases, const_cases, length_cases, refused_cases):
        cases.update(group())
    worst = {fn: {"vector": 0.0, "scalar": 0.0} for fn in H.FUNCTIONS}
    for name, c in cases.items():
        fn, w, x = c["fn"], c["window"], c["x"]
        entry = {"fn": fn, "window": w, "n": int(len(x))}
        if c["source"]:
            entry["source"] = c["source"]
            entry["input_sha256"] = H.sha256(x)
        else:
            out[name + ".x"] = x
        ref = run(reference, fn, x.copy(), w)
        own = {form: run(H.call, fn, x.copy(), w, form) for form in ("vector", "scalar")}
        if name.startswith("refused."):
            if not all(o[0] == "raises" and o[1] == "ValueError" for o in own.values()):
                raise SystemExit(f"{name}: the restatement does not refuse this call")
            entry.update(raises="ValueError", message=own["vector"][2],
                         reference=f"raises {ref[1]}" if ref[0] == "raises" else
                         f"returns ({int(np.isnan(ref[1]).sum())} NaN, {int((ref[1] == 0).sum())} zeros of {len(ref[1])})")
            manifest[name] = entry
            continue
        if ref[0] != "ok":
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        for form, o in own.items():
            dev = H.deviation(fn, o[1], ref[1]) if o[0] == "ok" else None
            if dev is None:
                raise SystemExit(f"{name}: the reference and the {form} form disagree on a NaN position -- case refused")
            entry[f"dev_{form}"] = dev
            worst[fn][form] = max(worst[fn][form], dev)
        out[name + ".out"] = ref[1]
        entry.update(finite=int(np.isfinite(ref[1]).sum()), nan=int(np.isnan(ref[1]).sum()), zeros=int((ref[1] == 0).sum()))
        manifest[name] = entry
    tolerances = {fn: {"measure": "relative" if H.RELATIVE[fn] else "absolute", "ref_dev": worst[fn]["vector"],
                       "ref_dev_scalar": worst[fn]["scalar"], "tolerance": H.tolerance_from(worst[fn]["vector"])}
                  for fn in H.FUNCTIONS}
    for k in sorted(manifest):
        print(k, {a: b for a, b in manifest[k].items() if not a.endswith("_sha256")})
    print(tolerances)
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "shape.npz"), **out)
    with open(os.path.join(gold, "shape.json"), "w") as fh:
        json.dump({"tolerances": tolerances, "cases": manifest}, fh, indent=1, sort_keys=True)
    print(len(manifest), "cases,", os.path.getsize(os.path.join(gold, "shape.npz")), "bytes")


if __name__ == "__main__":
    main()
