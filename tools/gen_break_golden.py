#!/usr/bin/env python3
"""Writes tests/golden/cusum_test.npz + cusum_test.json: outputs of the REFERENCE's Chu-Stinchcombe-White CUSUM test
(feature/core/structural_break/cusum.py) and of its CUSUMTest transform on seeded walks that the tests regenerate
(tests/_break_ref.py: grid_walk, integer arithmetic), on the six calls of the reference's own
tests/structural_breaks/test_cusum.py, on series with NaN, +inf, zero and negative prices, and the raising cases (type and message).  Build container only: imports the reference in
pure-Python mode through oracle/shim, like tools/gen_filter_golden.py; no GPU, nothing of the product.

A case is refused unless the reference and both forms of tests/_break_ref.py agree exactly, NaN positions included.
    python tools/gen_break_golden.py [reference checkout]
"""
import json
import math
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
import pandas as pd  # noqa: E402

import finmlkit.feature.core.structural_break.cusum as RC  # noqa: E402
from finmlkit.feature.transforms import CUSUMTest as RefCUSUMTest  # noqa: E402

from tests import _break_ref as H  # noqa: E402

NAMES = ("up", "down", "crit_up", "crit_down")


class HostLogNumpy:
    """numpy with `log` taken from libm.  The reference's functions are Numba kernels: compiled, their np.log is the host's log(),
    which is the project's contract (csrc/fmk_log.h).  Interpreted, np.log on an array is NumPy's own SIMD routine, which differs
    from libm in the last bit on a few arguments in a thousand and from one NumPy build to the next.  The recorded outputs are the
    reference's code with the log it has when compiled; how many elements the interpreted run rounds differently is recorded per
    case ("np_log_differs")."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def log(a):
        return H.host_log(a) if isinstance(a, np.ndarray) else math.log(a)


class host_log_in_reference:
    def __enter__(self):
        RC.np = HostLogNumpy()

    def __exit__(self, *a):
        RC.np = np


# seeded walks on a 0.01 price grid (H.grid_walk): name -> (function, seed, n, step, hold, window or None, warmup)
WALKS = {
    "rolling_w32":   ("rolling", 301, 1500, 35, 0.0, 32, 30),
    "rolling_w50":   ("rolling", 302, 1500, 35, 0.0, 50, 30),
    "rolling_w200":  ("rolling", 303, 1500, 35, 0.0, 200, 30),
    "rolling_w1000": ("rolling", 304, 1500, 35, 0.0, 1000, 30),
    "rolling_small_window": ("rolling", 305, 300, 35, 0.0, 5, 30),          # raised to warmup + 2
    "rolling_short": ("rolling", 306, 31, 35, 0.0, 50, 30),                 # n < warmup + 2: all NaN
    "developing":    ("developing", 307, 900, 35, 0.0, None, 30),
    "developing_w10": ("developing", 308, 400, 1, 0.8, None, 10),          # many repeated prices
}
TRANSFORM = (309, 3000, 35, 0.0)


def reference_test_calls():
    """The six calls of tests/structural_breaks/test_cusum.py, inputs as that file builds them."""
    growth = 100 * np.exp(0.001 * np.arange(100))
    np.random.seed(42)
    near_const = 100 + 0.01 * np.random.randn(100)
    np.random.seed(0)
    log_returns = (0.0 - 0.5 * 0.01 ** 2) * 1 + 0.01 * np.sqrt(1) * np.random.normal(0, 1, 1000)
    gbm = np.exp(np.log(100) + np.cumsum(log_returns))
    return {
        "developing_basic":     ("developing", growth, None, 10),
        "developing_constant":  ("developing", near_const, None, 30),
        "developing_random_walk": ("developing", gbm, None, 30),
        "last":                 ("last", growth, None, None),
        "rolling":              ("rolling", 100 * np.exp(0.0005 * np.arange(2000)), 1000, 30),
        "rolling_large_window": ("rolling", 100 * np.exp(0.001 * np.arange(500)), 1000, 30),
    }


def raising_calls():
    return {
        "rolling_zero":     ("rolling", np.array([100.0] * 40 + [0.0] + [100.0] * 9), 50, 30),
        "rolling_negative": ("rolling", np.array([-1.0] + [100.0] * 49), 50, 30),
    }


def odd_calls():
    """NaN, +inf, zero and negative prices: what IEEE arithmetic and the host's log make of the reference's code."""
    walk = H.grid_walk(1200, 41)
    nan_inf = walk.copy()
    nan_inf[400], nan_inf[800] = np.nan, np.inf
    zero_neg = walk[:300].copy()
    zero_neg[[50, 120, 121]] = [0.0, -3.0, -0.0]
    return {
        "rolling_nan_inf":          ("rolling", nan_inf, 50, 30),
        "developing_nan_inf":       ("developing", nan_inf[300:900], None, 30),
        "developing_zero_negative": ("developing", zero_neg, None, 30),
    }


def call(mod, fn, x, window, warmup, **kw):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            if fn == "rolling":
                r = mod.cusum_test_rolling(x, window, warmup, **kw)
            elif fn == "developing":
                r = mod.cusum_test_developing(x, warmup, **kw)
            else:
                r = tuple(np.array([v]) for v in mod.cusum_test_last(x, **kw))
            return ("ok", tuple(np.asarray(a, np.float64) for a in r))
    except Exception as e:                                        # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))


def run(name, fn, x, window, warmup):
    """The reference's answer (with the host's log); refuses the case unless both helper forms say the same.  -> (answer, the
    number of output elements the interpreted np.log rounds differently)."""
    with host_log_in_reference():
        ref = call(RC, fn, x, window, warmup)
    plain = call(RC, fn, x, window, warmup)
    differs = 0 if ref[0] != "ok" else sum(int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()) for a, b in zip(ref[1], plain[1]))
    for form in ("scalar", "vector"):
        own = call(H, fn, x, window, warmup, form=form)
        same = ref[0] == own[0] and (all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ref[1], own[1])) if ref[0] == "ok"
                                     else ref[1:] == own[1:])
        if not same:
            raise SystemExit(f"{name}: reference and helper ({form}) disagree -- case refused")
    return ref, differs


def main():
    out, manifest = {}, {}
    for name, (fn, seed, n, step, hold, window, warmup) in WALKS.items():
        res, differs = run(name, fn, H.grid_walk(n, seed, step, hold), window, warmup)
        for k, a in zip(NAMES, res[1]):
            out[f"walk.{name}.{k}"] = a
        manifest["walk." + name] = {"fn": fn, "seed": seed, "n": n, "step": step, "hold": hold, "window": window, "warmup": warmup,
                                    "finite": int(np.isfinite(res[1][0]).sum()), "np_log_differs": differs}
    for group, cases in (("refcall", reference_test_calls()), ("raising", raising_calls()), ("odd", odd_calls())):
        for name, (fn, x, window, warmup) in cases.items():
            res, differs = run(name, fn, x, window, warmup)
            key = f"{group}.{name}"
            out[key + ".x"] = np.asarray(x, np.float64)
            manifest[key] = {"fn": fn, "n": int(len(x)), "window": window, "warmup": warmup}
            if res[0] == "ok":
                for k, a in zip(NAMES, res[1]):
                    out[f"{key}.{k}"] = a
                manifest[key].update(finite=int(np.isfinite(res[1][0]).sum()), np_log_differs=differs)
            else:
                manifest[key].update(raises=res[1], message=res[2])
    # one CUSUMTest()(frame): the four arrays it is made from, and its six outputs
    seed, n, step, hold = TRANSFORM
    close = H.grid_walk(n, seed, step, hold)
    frame = pd.DataFrame({"close": close}, index=pd.date_range("2024-01-01", periods=n, freq="5min"))
    tr = RefCUSUMTest()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with host_log_in_reference():
            six = tr(frame, backend="nb")
    (_, four), differs = run("transform", "rolling", close, tr.window_size, tr.warmup_period)
    mine = H.cusum_transform(*four, max_age=tr.max_age)
    for s, m in zip(six, mine):
        if s.values.dtype != m.dtype or not np.array_equal(s.values, m, equal_nan=True):
            raise SystemExit(f"transform: reference and helper disagree on {s.name} -- case refused")
    for k, a in zip(NAMES, four):
        out[f"transform.{k}"] = a
    for s in six:
        out[f"transform.out.{s.name}"] = s.values
    manifest["transform"] = {"seed": seed, "n": n, "step": step, "hold": hold, "window": tr.window_size, "warmup": tr.warmup_period,
                             "max_age": tr.max_age, "names": [s.name for s in six], "dtypes": [str(s.values.dtype) for s in six],
                             "flags": [int(six[2].values.sum()), int(six[3].values.sum())], "np_log_differs": differs}
    for k in sorted(manifest):
        print(k, manifest[k])
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "cusum_test.npz"), **out)
    with open(os.path.join(gold, "cusum_test.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
