#!/usr/bin/env python3
"""Writes tests/golden/price_volume_corr.npz + price_volume_corr.json: outputs of the REFERENCE's rolling_price_volume_correlation
(feature/core/correlation.py) on the calls of the reference's own tests, on seeded walks that the tests regenerate
(tests/_corr_ref.py: grid_walk with dyadic or full-mantissa volumes), on NaN runs in either series, on zero, negative and infinite
prices and infinite volumes, on constant series, on strictly monotone series at every window 1 .. 10 (the reference's special case
for outputs 4 .. 9), on the edge lengths, and the refused arguments.  Build container only: imports the reference in pure-Python mode
through oracle/shim, like tools/gen_rolling_golden.py; no GPU, nothing of the product.

The reference is run as it is: its `sum(list)` is Python's, a plain left-to-right sum before Python 3.12 (compensated from 3.12 on,
which is no longer what Numba compiles: the generator refuses to run there).  A case is refused unless the reference and both forms
of tests/_corr_ref.py agree in every bit, NaN positions included.
    python tools/gen_corr_golden.py REFERENCE_CHECKOUT        (or FINMLKIT_REFERENCE in the environment)
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_corr_golden.py REFERENCE_CHECKOUT (or set FINMLKIT_REFERENCE)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

from finmlkit.feature.core.correlation import rolling_price_volume_correlation as reference  # noqa: E402

from tests import _corr_ref as H  # noqa: E402

NAN, INF = np.nan, np.inf


def case(price, volume, window, source=None):
    """`source`: how the tests regenerate the inputs ({"price": [generator, args], "volume": [...]}); without it they are stored."""
    return dict(price=np.asarray(price, np.float64), volume=np.asarray(volume, np.float64), window=window, source=source)


def reference_test_calls():
    """The eight calls of tests/features/test_price_volume_correlation.py, inputs as that file builds them (the two transform tests
    hand their frame's columns to the function)."""
    up = np.arange(10.0, 20.0)
    vol_up, vol_down = np.arange(100.0, 200.0, 10.0), np.arange(190.0, 90.0, -10.0)
    out = {}
    out["refcall.basic"] = case([10.0, 11.0, 12.0, 11.5, 11.0, 10.5, 11.0, 12.0, 13.0, 12.5],
                                [100.0, 110.0, 120.0, 115.0, 105.0, 95.0, 105.0, 110.0, 120.0, 115.0], 3)
    out["refcall.perfect"] = case(up, vol_up, 4)
    out["refcall.inverse"] = case(up, vol_down, 4)
    out["refcall.nan_handling"] = case([10.0, 11.0, NAN, 13.0, 14.0, 15.0, 16.0, NAN, 18.0, 19.0],
                                       [100.0, 110.0, 120.0, 130.0, NAN, 150.0, 160.0, 170.0, 180.0, NAN], 4)
    out["refcall.small_window"] = case(up[:5], vol_up[:5], 2)
    out["refcall.zero_price"] = case([10.0, 0.0, 12.0, 13.0, 14.0, 15.0, 16.0, 0.0, 18.0, 19.0], vol_up, 4)
    out["refcall.transform_basic"] = case(up, vol_up, 4)
    out["refcall.transform_custom_columns"] = case(up, vol_up, 4)
    return out


def walk_cases():
    out = {}
    n = 1000
    for k, window in enumerate((1, 2, 3, 4, 9, 10, 64, 65, 300)):
        for kind, gen in (("dyadic", "dyadic_volumes"), ("mantissa", "mantissa_volumes")):
            src = {"price": ["grid_walk", [n, 700 + k, 35, 0.0]], "volume": [gen, [n, 800 + k]]}
            out[f"walk.{kind}_w{window}"] = case(*H.generate(src), window, src)
    # held prices: zero returns, and windows whose returns are all equal (NaN)
    src = {"price": ["grid_walk", [600, 720, 1, 0.9]], "volume": ["dyadic_volumes", [600, 820]]}
    out["walk.held_w5"] = case(*H.generate(src), 5, src)
    return out


def nan_cases():
    """NaN runs in price, in volume and in both; a window left with 0, 1 and 2 valid pairs."""
    out = {}
    n, window = 400, 8
    base_p, base_v = H.grid_walk(n, 730), H.dyadic_volumes(n, 830)

    def runs(x):
        x = x.copy()
        x[40:43] = NAN                       # shorter than the window
        x[100:130] = NAN                     # longer
        x[200] = NAN
        return x
    out["nan.price_w8"] = case(runs(base_p), base_v, window)
    out["nan.volume_w8"] = case(base_p, runs(base_v), window)
    v = base_v.copy()
    v[41:46] = NAN
    v[210:214] = NAN
    out["nan.both_w8"] = case(runs(base_p), v, window)
    # a NaN price at i spoils ret[i] and ret[i+1]: at window 4 with prices 20 and 22 NaN the window of output 24 holds ret 21 .. 24,
    # of which 24 alone is valid (count 1), that of 25 two (count 2); with volume 24 NaN too output 25 has count 1 and 26 count 2;
    # output 23 (ret 20 .. 23 all NaN) has count 0 -- and NaN at its own position
    p = H.grid_walk(60, 731)
    p[[20, 22]] = NAN
    out["nan.counts_price_w4"] = case(p, H.dyadic_volumes(60, 831), 4)
    v = H.dyadic_volumes(60, 831)
    v[[24, 40, 41, 42]] = NAN
    out["nan.counts_both_w4"] = case(p, v, 4)
    p = H.grid_walk(60, 732)
    v = H.dyadic_volumes(60, 832)
    v[30:33] = NAN                            # window 4 at output 33: one valid pair, its own
    v[36] = NAN
    out["nan.counts_volume_w4"] = case(p, v, 4)
    return out


def odd_cases():
    """Zero, -0.0, negative and infinite prices, infinite volume; constant price and constant volume."""
    out = {}
    n = 200
    p, v = H.grid_walk(n, 740), H.dyadic_volumes(n, 840)
    p[30], p[60], p[90], p[91], p[120], p[150] = 0.0, -0.0, -3.0, -4.5, INF, -INF
    out["odd.prices_w6"] = case(p, v, 6)
    out["odd.prices_w20"] = case(p, v, 20)
    v2 = v.copy()
    v2[50], v2[100], v2[140] = INF, -INF, 0.0
    out["odd.volume_inf_w6"] = case(H.grid_walk(n, 741), v2, 6)
    out["odd.both_w12"] = case(p, v2, 12)
    out["const.price_w5"] = case(np.full(40, 101.5), H.dyadic_volumes(40, 842), 5)
    out["const.volume_w5"] = case(H.grid_walk(40, 743), np.full(40, 12.25), 5)
    out["const.both_w3"] = case(np.full(20, 7.0), np.full(20, 3.0), 3)
    pv = H.grid_walk(80, 744)
    vv = H.dyadic_volumes(80, 844)
    vv[20:40] = 5.5                           # constant inside the series: NaN windows between numbers
    pv[50:70] = pv[50]
    out["const.runs_w6"] = case(pv, vv, 6)
    return out


def monotone_cases():
    """Strictly monotone series at every window 1 .. 10: outputs 4 .. 9 are the special case's; window 10 shows where it ends.  The
    same with a NaN inside a special-case window, and with a NaN at the current position."""
    out = {}
    n = 14
    up = 10.0 + np.arange(n) * 1.0
    geo = 10.0 * 1.05 ** np.arange(n)                               # rising prices with returns that vary
    vol_up = 100.0 + 10.0 * np.arange(n) + (np.arange(n) % 3)
    vol_down = vol_up[::-1].copy()
    for window in range(1, 11):
        out[f"mono.up_up_w{window}"] = case(up, vol_up, window)
        out[f"mono.up_down_w{window}"] = case(up, vol_down, window)
        out[f"mono.geo_up_w{window}"] = case(geo, vol_up, window)
        out[f"mono.down_up_w{window}"] = case(up[::-1].copy(), vol_up, window)
        for name, vol in (("up", vol_up), ("down", vol_down)):
            p, v = up.copy(), vol.copy()
            v[5] = NAN                                              # inside the windows of outputs 6 .., current at 5
            out[f"mono.nan_volume_{name}_w{window}"] = case(p, v, window)
            p = up.copy()
            p[6] = NAN                                              # ret 6 and 7 NaN: current position of outputs 6 and 7
            out[f"mono.nan_price_{name}_w{window}"] = case(p, vol, window)
    flat = up.copy()
    flat[7] = flat[6]                                               # one equal step: not strictly rising
    out["mono.flat_step_w4"] = case(flat, vol_up, 4)
    eqv = vol_up.copy()
    eqv[7] = eqv[6]
    out["mono.equal_volume_w4"] = case(up, eqv, 4)
    return out


def clamp_cases():
    """Window 2: two points, so every output is +-1 up to the rounding of the quotient, or NaN; about three quarters are exactly
    +-1, the others one or two units below in magnitude or clamped from above."""
    src = {"price": ["grid_walk", [1000, 750, 35, 0.0]], "volume": ["mantissa_volumes", [1000, 850]]}
    return {"clamp.w2": case(*H.generate(src), 2, src)}


def length_cases():
    out = {}
    for window in (1, 5, 12):
        for n in sorted({1, 2, window, window + 1}):
            out[f"length.n{n}_w{window}"] = case(H.grid_walk(n, 760 + n), H.dyadic_volumes(n, 860 + n), window)
    return out


def refused_calls():
    p, v = H.grid_walk(20, 770), H.dyadic_volumes(20, 870)
    out = {"refused.w0": case(p, v, 0), "refused.w-3": case(p, v, -3), "refused.short_volume": case(p, v[:19], 4),
           "refused.short_price": case(p[:5], v, 4)}
    return out


def run(fn, c, **kw):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return ("ok", np.asarray(fn(c["price"].copy(), c["volume"].copy(), c["window"], **kw), np.float64))
    except Exception as e:                                        # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))


def differs(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()) if a.shape == b.shape else -1


def main():
    if sys.version_info >= (3, 12):
        raise SystemExit("Python 3.12 and later sum floats with compensation: the reference interpreted there is not the contract")
    out, manifest, cases = {}, {}, {}
    for group in (reference_test_calls, walk_cases, nan_cases, odd_cases, monotone_cases, clamp_cases, length_cases, refused_calls):
        cases.update(group())
    for name, c in cases.items():
        entry = {"window": c["window"], "n": int(len(c["price"]))}
        if c["source"]:
            entry["source"] = c["source"]
            entry["input_sha256"] = H.sha256(c["price"], c["volume"])
        else:
            out[name + ".price"], out[name + ".volume"] = c["price"], c["volume"]
        own = [run(H.rolling_price_volume_correlation, c, form=form) for form in ("scalar", "vector")]
        ref = run(reference, c)
        if name.startswith("refused."):
            if not all(o[0] == "raises" and o[1] == "ValueError" and o[1:] == own[0][1:] for o in own):
                raise SystemExit(f"{name}: the helper does not refuse this call")
            entry.update(raises=own[0][1], message=own[0][2],
                         reference=f"raises {ref[1]}" if ref[0] == "raises" else
                         f"returns ({int(np.isnan(ref[1]).sum())} NaN of {len(ref[1])})")
            manifest[name] = entry
            continue
        if ref[0] != "ok":
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        for form, o in zip(("scalar", "vector"), own):
            if o[0] != "ok" or o[1].dtype != np.float64 or differs(ref[1], o[1]) != 0:
                raise SystemExit(f"{name}: reference and helper ({form}) disagree -- case refused")
        r = ref[1]
        out[name + ".out"] = r
        inside = r[(np.abs(r) < 1.0)]
        entry.update(finite=int(np.isfinite(r).sum()), plus_one=int((r == 1.0).sum()), minus_one=int((r == -1.0).sum()),
                     nan_from_window=int(np.isnan(r[c["window"]:]).sum()), inside=int(len(inside)))
        manifest[name] = entry
    for k in sorted(manifest):
        print(k, {a: b for a, b in manifest[k].items() if a not in ("input_sha256", "source")})
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "price_volume_corr.npz"), **out)
    with open(os.path.join(gold, "price_volume_corr.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print(len(manifest), "cases,", os.path.getsize(os.path.join(gold, "price_volume_corr.npz")), "bytes")


if __name__ == "__main__":
    main()
