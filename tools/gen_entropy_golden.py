#!/usr/bin/env python3
"""Writes tests/golden/entropy.npz + entropy.json: outputs of the REFERENCE's ApproximateEntropy (finmlkit/feature/transforms.py:
1400-1457, its pandas backend) on seeded series that the tests regenerate (tests/_shape_ref.py: returns on a dyadic grid, which tie
at distance 0, and returns that use the whole mantissa), on constant and two-valued series, on series with NaN and infinities in a
window's first and last position, on the edge lengths, and the refused arguments.  Build container only: imports the reference
through oracle/shim, like tools/gen_shape_golden.py; no GPU, nothing of the product.

The reference calls `antropy.app_entropy`, and `antropy` is not installed where this runs, nor is its source part of the reference
checkout.  This tool therefore places a stand-in module of that name in sys.modules before the import: `app_entropy` as the package
publishes it -- for k in (order, order + 1) the embedded vectors, sklearn's KDTree(metric="chebyshev").query_radius(.., count_only=
True) for the counts, mean(log(count / N)), phi_order - phi_{order+1}.  THE STAND-IN FOLLOWS antropy's PUBLISHED ALGORITHM AND
COULD NOT BE COMPARED WITH THE PACKAGE ITSELF HERE.  Everything around it -- the rolling apply, the tolerance times np.std, the
NaN handling, the name -- is the untouched reference.

A case is refused unless the reference path and both forms of tests/_entropy_ref.py agree on every NaN position, the scalar form's
integer counts reproduce the KD-tree's in every window, and `knife_edge` is empty (no pair of a window within 2^-40 r of r).  The
tolerance is measured here, never from a kernel's output: the largest absolute deviation of the vector form (the kernel's order)
from the reference path over all cases, times 16, rounded up to a power of ten.  entropy.json records it under "tolerances" with
the deviations of both forms per case, and the knife-edge record.  The inputs of seeded cases are recorded as digests only.
    python tools/gen_entropy_golden.py <reference checkout>
"""
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_entropy_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
from numpy.lib.stride_tricks import sliding_window_view  # noqa: E402
from sklearn.neighbors import KDTree  # noqa: E402


def stand_in():
    """`antropy` as far as the reference uses it; COUNTS keeps the KD-tree's counts of every call."""
    mod = types.ModuleType("antropy")
    mod.COUNTS = []

    def app_entropy(x, order=2, tolerance=None, metric="chebyshev"):
        x = np.asarray(x, np.float64)
        r = 0.2 * np.std(x, ddof=0) if tolerance is None else tolerance
        phi, counts = [], []
        for k in (order, order + 1):
            emb = np.ascontiguousarray(sliding_window_view(x, k))
            c = KDTree(emb, metric=metric).query_radius(emb, r, count_only=True).astype(np.float64)
            counts.append(c)
            phi.append(np.mean(np.log(c / emb.shape[0])))
        mod.COUNTS.append(counts)
        return np.subtract.reduce(phi)

    mod.app_entropy = app_entropy
    return mod


ANTROPY = sys.modules["antropy"] = stand_in()

import finmlkit.feature.transforms as RT  # noqa: E402

from tests import _entropy_ref as E  # noqa: E402

N_WALK = 1000
INF = np.inf
EVERY_PAIR = 1e6                     # a tolerance under which every pair of a window matches


def reference(x, window, m, tolerance):
    """The reference's transform on the default column, its pandas backend (the other one falls back to it) -> (values, the
    KD-tree's counts of every window it computed)."""
    t = RT.ApproximateEntropy(window, m, tolerance)
    frame = pd.DataFrame({t.requires[0]: x}, index=pd.date_range("2024-01-01", periods=len(x), freq="1min"))
    del ANTROPY.COUNTS[:]
    s = t(frame, backend="pd")
    if s.name != f"ret1_apen{window}":
        raise SystemExit(f"the reference names its output {s.name}")
    return np.asarray(s.values, np.float64), list(ANTROPY.COUNTS)


def case(window, m=2, tolerance=0.2, x=None, source=None):
    return dict(window=window, m=m, tolerance=tolerance, x=np.asarray(E.generate(source) if source else x, np.float64), source=source)


def walk_cases():
    out = {}
    for j, w in enumerate((3, 4, 24, 63, 64, 65, 300)):
        out[f"walk.m2_w{w}"] = case(w, source=["dyadic_returns", [N_WALK, 1600 + j]])
    out[f"walk.m2_w{E.MAX_WINDOW}"] = case(E.MAX_WINDOW, source=["dyadic_returns", [E.MAX_WINDOW + 3, 1608]])
    for j, w in enumerate((24, 64, 65, 300)):
        out[f"mantissa.m2_w{w}"] = case(w, source=["mantissa_returns", [N_WALK, 1610 + j]])
    out[f"mantissa.m{E.MAX_M}_w{E.MAX_WINDOW}"] = case(E.MAX_WINDOW, E.MAX_M, source=["mantissa_returns", [E.MAX_WINDOW + 3, 1615]])
    for k, m in enumerate((1, 3, E.MAX_M)):
        for j, w in enumerate((m + 1, m + 2, 24, 64, 65)):
            out[f"walk.m{m}_w{w}"] = case(w, m, source=["dyadic_returns", [400, 1620 + 10 * k + j]])
    for j, (tag, tol) in enumerate((("0", 0.0), ("1", 1.0), ("every_pair", EVERY_PAIR))):
        for i, w in enumerate((24, 65)):
            out[f"tolerance.{tag}_w{w}"] = case(w, 2, tol, source=["dyadic_returns", [400, 1660 + 2 * j + i]])
            out[f"tolerance.{tag}_mantissa_w{w}"] = case(w, 2, tol, source=["mantissa_returns", [400, 1670 + 2 * j + i]])
    return out


def const_cases():
    out = {}
    for tag, v in (("zeros", 0.0), ("half", 0.5)):
        for w in (5, 70):
            out[f"const.{tag}_w{w}"] = case(w, x=np.full(w + 40, v))
    x = np.array(E.dyadic_returns(200, 1680))
    x[60:140] = 0.5                                                     # a constant stretch inside a walk
    out["const.stretch_w24"] = case(24, x=x)
    rng = np.random.default_rng(1681)
    two = np.where(rng.integers(0, 2, 400) == 1, 2.0 ** -10, -(2.0 ** -10))
    for w in (12, 70):
        out[f"two_valued.w{w}"] = case(w, x=two)
        out[f"two_valued.tolerance1_w{w}"] = case(w, 2, 1.0, x=two)
        out[f"two_valued.tolerance0_w{w}"] = case(w, 2, 0.0, x=two)      # ties at distance 0 only
    return out


def edge_cases():
    """NaN, +inf and -inf: each is the last element of one window and the first of another."""
    out = {}
    for w in (12, 70):
        x = np.array(E.dyadic_returns(3 * 160 + 100, 1690 + w))
        for j, v in enumerate((np.nan, INF, -INF)):
            x[100 + 160 * j] = v
        out[f"edge.w{w}"] = case(w, x=x)
    x = np.array(E.dyadic_returns(200, 1695))
    x[[0, 90, 199]] = (np.nan, INF, -INF)
    out["edge.ends_w10"] = case(10, x=x)
    return out


def length_cases():
    out = {}
    for w in (3, 12, 70):
        for n in sorted({1, 2, w - 1, w, w + 1, w + 2}):
            out[f"length.n{n}_w{w}"] = case(w, x=E.dyadic_returns(max(n, 2), 1700 + w)[:n])
    out["length.empty_w12"] = case(12, x=np.empty(0))
    return out


def refused_cases():
    x = E.dyadic_returns(40, 1710)
    args = {"m0": (12, 0, 0.2), "m_negative": (12, -1, 0.2), "m_above_max": (12, E.MAX_M + 1, 0.2), "window_m": (2, 2, 0.2),
            "window_0": (0, 1, 0.2), "window_negative": (-3, 2, 0.2), "window_above_max": (E.MAX_WINDOW + 1, 2, 0.2),
            "tolerance_negative": (12, 2, -0.5), "tolerance_nan": (12, 2, np.nan), "tolerance_inf": (12, 2, INF)}
    return {f"refused.{k}": case(w, m, tol, x=x) for k, (w, m, tol) in args.items()}


def run(f, *a):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return ("ok", f(*a))
    except Exception as e:                                             # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))


def counts_agree(x, w, m, tolerance, kd):
    """The scalar form's brute-force counts against the KD-tree's, window by window (the windows the reference computed are the
    finite ones, in order)."""
    k = 0
    for t in range(w - 1, len(x)):
        win = x[t - w + 1:t + 1]
        if not np.isfinite(win).all():
            continue
        cm, cm1 = E.window_counts(win, m, tolerance * np.std(win))
        if k >= len(kd) or not (np.array_equal(cm, kd[k][0]) and np.array_equal(cm1, kd[k][1])):
            return False
        k += 1
    return k == len(kd)


def main():
    out, manifest = {}, {}
    cases = {}
    for group in (walk_cases, const_cases, edge_cases, length_cases, refused_cases):
        cases.update(group())
    worst = {"vector": 0.0, "scalar": 0.0}
    smallest_margin, edge_windows = float("inf"), 0
    for name, c in cases.items():
        w, m, tol, x = c["window"], c["m"], c["tolerance"], c["x"]
        entry = {"window": w, "m": m, "tolerance": tol if np.isfinite(tol) else repr(float(tol)), "n": int(len(x))}
        if c["source"]:
            entry["source"] = c["source"]
            entry["input_sha256"] = E.sha256(x)
        else:
            out[name + ".x"] = x
        own = {form: run(E.approximate_entropy, x.copy(), w, m, tol, form) for form in ("vector", "scalar")}
        if name.startswith("refused."):
            if not all(o[0] == "raises" and o[1] == "ValueError" and o[2] in E.MESSAGES for o in own.values()):
                raise SystemExit(f"{name}: the restatement does not refuse this call")
            ref = run(reference, x.copy(), w, m, tol)
            entry.update(raises="ValueError", message=own["vector"][2],
                         reference=f"raises {ref[1]}" if ref[0] == "raises" else f"returns ({int(np.isnan(ref[1][0]).sum())} NaN of {len(x)})")
            manifest[name] = entry
            continue
        ref = run(reference, x.copy(), w, m, tol)
        if ref[0] != "ok":
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        want, kd = ref[1]
        for form, o in own.items():
            dev = E.deviation(o[1], want) if o[0] == "ok" else None
            if dev is None:
                raise SystemExit(f"{name}: the reference and the {form} form disagree on a NaN position -- case refused ({o[1:]})")
            entry[f"dev_{form}"] = dev
            worst[form] = max(worst[form], dev)
        if not counts_agree(x, w, m, tol, kd):
            raise SystemExit(f"{name}: brute-force counts differ from the KD-tree's -- case refused")
        edges = int(E.knife_edge(x, w, m, tol).sum())
        if edges:
            raise SystemExit(f"{name}: {edges} knife-edge windows -- case refused, choose another seed")
        edge_windows += edges
        entry["margin"] = E.margin(x, w, m, tol)
        smallest_margin = min(smallest_margin, entry["margin"])
        out[name + ".out"] = want
        entry.update(finite=int(np.isfinite(want).sum()), nan=int(np.isnan(want).sum()), zeros=int((want == 0).sum()),
                     windows_counted=len(kd))
        manifest[name] = entry
    tolerances = {"measure": "absolute", "ref_dev": worst["vector"], "ref_dev_scalar": worst["scalar"],
                  "tolerance": E.tolerance_from(worst["vector"])}
    knife = {"guard": E.KNIFE, "windows": edge_windows, "smallest_margin": smallest_margin}
    for k in sorted(manifest):
        print(k, {a: b for a, b in manifest[k].items() if not a.endswith("_sha256")})
    print(tolerances, knife)
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "entropy.npz"), **out)
    with open(os.path.join(gold, "entropy.json"), "w") as fh:
        json.dump({"tolerances": tolerances, "knife_edge": knife, "cases": manifest}, fh, indent=1, sort_keys=True)
    print(len(manifest), "cases,", os.path.getsize(os.path.join(gold, "entropy.npz")), "bytes")


if __name__ == "__main__":
    main()
