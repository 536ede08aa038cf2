#!/usr/bin/env python3
"""Writes tests/golden/cusum_filter.npz + cusum_filter.json: outputs of the REFERENCE's cusum_filter (sampling/filters.py) on
synthetic tapes that the tests regenerate from their seed (oracle.synth), on a few hand-made series, and on the six calls of the
reference's own tests/sampling/test_cusum_filter.py (three of them raise: type and message are recorded).  Build container only:
imports the reference in pure-Python mode through oracle/shim, like tools/gen_label_golden.py; no GPU, nothing of the product.

A case is refused unless the reference and tests/_filter_ref.py agree exactly.
    python tools/gen_filter_golden.py [reference checkout]
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

import finmlkit.sampling.filters as RF  # noqa: E402

from oracle import oracle as orc  # noqa: E402
from tests import _filter_ref as H  # noqa: E402

# tapes regenerated from their seed: name -> (seed, ticks, c, per element, shift): the thresholds are H.hashed_threshold's
TAPES = {
    "dense_const":   (201, 60_000, 1e-5, False, 0.0),
    "zero_const":    (202, 20_000, 0.0, False, 0.0),
    "wide_const":    (203, 60_000, 1e-4, False, 0.0),
    "dense_per":     (204, 60_000, 1e-5, True, 0.0),
    "negative_per":  (205, 10_000, 4e-6, True, 1.5),          # about a quarter of the thresholds are negative
}


def hand_made():
    """Small series whose inputs are stored: odd values in x and in the thresholds."""
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng(7)
    walk = 100.0 * np.exp(np.cumsum(0.01 * rng.standard_normal(3000)))
    odd = walk[:400].copy()
    odd[[17, 18, 90, 200, 201, 350]] = [nan, nan, 0.0, -3.0, -4.0, 0.0]
    thr_odd = np.full(400, 0.02)
    thr_odd[[30, 31, 32, 120, 121, 260, 300]] = [nan, -1.0, inf, nan, -0.5, inf, -inf]
    return {
        "walk_const":     (walk, np.array([0.03])),
        "walk_per":       (walk, 0.01 + 0.04 * rng.random(3000)),
        "odd_x":          (odd, np.array([0.02])),
        "odd_thr":        (walk[:400], thr_odd),
        "odd_both":       (odd, thr_odd),
        "nan_const":      (walk[:400], np.array([nan])),
        "inf_const":      (walk[:400], np.array([inf])),
        "negative_const": (walk[:400], np.array([-0.01])),
        "powers_of_two":  (2.0 ** np.arange(40), np.array([np.log(2.0)])),
        "priority":       (np.exp(np.cumsum([0.0, 5.0, -3.0, 0.0, -1.0])), np.array([10.0, 10.0, 1.0, 10.0, 2.0])),
    }


def reference_test_calls():
    """The six calls of tests/sampling/test_cusum_filter.py, inputs as that file builds them."""
    np.random.seed(42)
    large = np.cumsum(np.random.randn(10000)) + 1000
    return {
        "no_events":        (np.array([100, 100, 100, 100, 100], dtype=np.float64), np.array([0.5])),
        "single_price":     (np.array([100], dtype=np.float64), np.array([0.01])),
        "empty_series":     (np.array([], dtype=np.float64), np.array([0.01])),
        "invalid_threshold_length": (np.array([100, 101, 102], dtype=np.float64), np.array([0.01, 0.02])),
        "large_series":     (large, np.array([0.5])),
        "all_events":       (np.array([100, 100.01, 100.02, 100.03, 100.04, 100.05], dtype=np.float64), np.array([1e-5])),
    }


def run(name, x, thr):
    """-> ("ok", indices) or ("raises", type name, message); refuses the case when the helper says otherwise."""
    def call(fn):
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                return ("ok", np.asarray(fn(x, thr), np.int64))
        except Exception as e:                                    # noqa: BLE001 -- recorded as data
            return ("raises", type(e).__name__, str(e))
    ref, own = call(RF.cusum_filter), call(H.cusum_filter)
    same = ref[0] == own[0] and (np.array_equal(ref[1], own[1]) if ref[0] == "ok" else ref[1:] == own[1:])
    if not same:
        raise SystemExit(f"{name}: reference and helper disagree -- case refused")
    return ref


def main():
    out, manifest = {}, {}
    for name, (seed, n, c, per, shift) in TAPES.items():
        _, px, _, _ = orc.synth(seed, 0, n)
        res = run(name, px, H.hashed_threshold(n, c, per, shift))
        out[f"tape.{name}.events"] = res[1]
        manifest["tape." + name] = {"seed": seed, "n": n, "c": c, "per_element": per, "shift": shift, "events": int(len(res[1]))}
    for group, cases in (("hand", hand_made()), ("refcall", reference_test_calls())):
        for name, (x, thr) in cases.items():
            res = run(name, x, thr)
            key = f"{group}.{name}"
            out[key + ".x"], out[key + ".thr"] = np.asarray(x, np.float64), np.asarray(thr, np.float64)
            if res[0] == "ok":
                out[key + ".events"] = res[1]
                manifest[key] = {"n": int(len(x)), "n_thr": int(len(thr)), "events": int(len(res[1]))}
            else:
                manifest[key] = {"n": int(len(x)), "n_thr": int(len(thr)), "raises": res[1], "message": res[2]}
    for k in sorted(manifest):
        print(k, manifest[k])
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "cusum_filter.npz"), **out)
    with open(os.path.join(gold, "cusum_filter.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
