#!/usr/bin/env python3
"""Writes tests/golden/order_stats.npz + order_stats.json: outputs of the REFERENCE's windowed order statistics -- comp_burst_ratio
and pct_change (feature/core/utils.py), roc and stoch_k (feature/core/momentum.py) -- on seeded series that the tests regenerate
(tests/_order_ref.py: grid walks, a tie-heavy size series drawn from 8 levels, all-distinct values, OHLC walks; integer arithmetic),
on signed full-mantissa series with zeros of both signs, subnormals, +-inf and DBL_MAX at every window at which the kernels change
path (signed_sizes, alternating_sizes, signed_ohlc_walk), on series with NaN runs, +-inf, zeros and negative values, on a zero median, on the edge lengths, on the calls of the reference's
own tests, and the refused arguments.  Build container only: imports the reference in pure-Python mode through oracle/shim, like
tools/gen_rolling_golden.py; no GPU, nothing of the product.

No sum, log or exp occurs in these functions, so the truth is the UNTOUCHED reference: nothing is substituted in its `np`.  A case
is refused unless the reference and both forms of tests/_order_ref.py agree in every element, NaN positions included, and for
burst ratio, roc and pct_change in the sign of every zero (np.signbit).  %K stays on `==`: np.min / np.max over a window that holds
-0.0 and 0.0 has no defined winner, the reference's running min() / max() another one, and only the sign of a zero result can
differ.  stoch_k cases hold no NaN in low / high (the reference is path-dependent there; the project's rule is tested against the
restatement).  Cases of more than 2100 elements record `output_sha256` (over the output's bytes, every NaN made the canonical quiet
NaN) instead of the output: the host test recomputes it from the vector form, which gates the restatement on the reference at full
size.  The scalar form is slow and left out of the gate above a window of 4000.
    python tools/gen_order_golden.py [reference checkout]
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

import finmlkit.feature.core.momentum as RMO  # noqa: E402
import finmlkit.feature.core.utils as RUT  # noqa: E402

from tests import _order_ref as H  # noqa: E402


class Reference:
    """The reference's four functions under the names tests/_order_ref.call expects."""
    comp_burst_ratio = staticmethod(lambda x, w: RUT.comp_burst_ratio(x, w))
    pct_change = staticmethod(lambda x, p: RUT.pct_change(x, p))
    roc = staticmethod(lambda x, p: RMO.roc(x, p))
    stoch_k = staticmethod(lambda c, lo, hi, n: RMO.stoch_k(c, lo, hi, n))


GENERATORS = {"grid_walk": H.grid_walk, "tie_sizes": H.tie_sizes, "distinct_sizes": H.distinct_sizes, "ohlc_walk": H.ohlc_walk,
              "signed_sizes": H.signed_sizes, "alternating_sizes": H.alternating_sizes, "signed_ohlc_walk": H.signed_ohlc_walk}
STORED_MAX = 2100                      # longer cases record the hash of their output, not the output
SCALAR_MAX = 4000                      # the scalar form of the restatement is gated up to this window
SORT_TILE, SORT_WINDOW_MAX, WALK_TILE = 1024, 3073, 256     # csrc/fmk_order.hip: ORD_TILE, ORD_SORT_WINDOW_MAX, ORD_WALK_TILE
# alternating_sizes: the seed per even window at which a quarter of the medians and more is positive and a quarter and more is not
# (tests/test_order_host.py asserts the shares); odd windows alternate at any seed
ALT_SEEDS = {20: 1, 3072: 1, 3074: 80, 3842: 82, 8500: 76}


def case(fn, inputs, arg, gen=None, args=None):
    """`gen`, `args`: how the tests regenerate the inputs (a name of GENERATORS and its arguments); without them they are stored."""
    if fn == "stoch":
        inputs = tuple(np.asarray(a, np.float64) for a in inputs)
    else:
        inputs = np.asarray(inputs, np.float64)
    return dict(fn=fn, inputs=inputs, arg=arg, source={"gen": gen, "args": args} if gen else None)


def seeded(fn, arg, gen, *args):
    return case(fn, GENERATORS[gen](*args), arg, gen, list(args))


def series_cases():
    out = {}
    n = 1200
    for k, w in enumerate((1, 2, 3, 7, 8, 50, 51, 200, 1000)):
        out[f"walk.burst_w{w}"] = seeded("burst", w, "grid_walk", n, 500 + k, 35, 0.0)
    out["walk.burst_held_w20"] = seeded("burst", 20, "grid_walk", n, 520, 1, 0.9)
    for k, w in enumerate((1, 2, 3, 4, 50, 51, 64, 65, 200, 1000)):
        out[f"ties.burst_w{w}"] = seeded("burst", w, "tie_sizes", n, 530 + k)
    for k, w in enumerate((1, 2, 5, 50, 101)):
        out[f"distinct.burst_w{w}"] = seeded("burst", w, "distinct_sizes", n, 550 + k)
    for k, p in enumerate((0, 1, 3, 50, n - 1)):
        out[f"walk.roc_p{p}"] = seeded("roc", p, "grid_walk", n, 560 + k, 35, 0.0)
        out[f"walk.pct_p{p}"] = seeded("pct", p, "grid_walk", n, 560 + k, 35, 0.0)
        out[f"ties.pct_p{p}"] = seeded("pct", p, "tie_sizes", n, 570 + k)
    for k, length in enumerate((1, 2, 3, 14, 50, 200, 1000)):
        out[f"walk.stoch_l{length}"] = seeded("stoch", length, "ohlc_walk", n, 580 + k, 35, 30, 0.0)
    for k, length in enumerate((1, 2, 5, 14)):              # flat stretches: hi == lo gives NaN
        out[f"held.stoch_l{length}"] = seeded("stoch", length, "ohlc_walk", n, 590 + k, 2, 1, 0.9)
    return out


def value_class_cases():
    """Negative, zero, subnormal, infinite and DBL_MAX values through every path of the kernels: the sorted span at both its key
    widths' ends (windows 20 / 21, and 3072 / 3073 at 4096 entries), the bisection over one, two and three slabs."""
    out = {}
    for k, w in enumerate((20, 21, 3072, 3073, 3074, 3075, 3842, 8500, 8501, 12289)):
        n = w - 1 + (SORT_TILE if w <= SORT_WINDOW_MAX else WALK_TILE) + 1       # a full tile and a tile of one output
        out[f"signed.burst_w{w}"] = seeded("burst", w, "signed_sizes", n, 640 + k)
        out[f"alt.burst_w{w}"] = seeded("burst", w, "alternating_sizes", n, ALT_SEEDS.get(w, 5))
    for k, length in enumerate((14, 4097, 8500, 12289)):
        out[f"signed.stoch_l{length}"] = seeded("stoch", length, "signed_ohlc_walk", length - 1 + WALK_TILE + 1, 660 + k)
    out["hostile.stoch_l14"] = seeded("stoch", 14, "signed_ohlc_walk", 14 - 1 + 2 * WALK_TILE + 1, 21, True)
    for p in (0, 1, 300):
        out[f"signed.roc_p{p}"] = seeded("roc", p, "signed_sizes", 2000, 670)
        out[f"signed.pct_p{p}"] = seeded("pct", p, "signed_sizes", 2000, 670)
    return out


def odd_cases():
    """NaN runs shorter and longer than the window, +-inf, zeros and negative values, a zero median."""
    out = {}
    x = H.grid_walk(600, 601)
    x[50:53] = np.nan                      # shorter than the windows below
    x[150:190] = np.nan                    # longer
    x[300], x[350] = np.inf, -np.inf
    x[400], x[450], x[451] = 0.0, -3.0, -0.0
    x[500:503] = np.inf                    # an infinite median at window 3, inf / inf
    for w in (1, 2, 3, 20, 21):
        out[f"odd.burst_w{w}"] = case("burst", x, w)
    for p in (0, 1, 2, 20):
        out[f"odd.roc_p{p}"] = case("roc", x, p)
        out[f"odd.pct_p{p}"] = case("pct", x, p)
    z = H.tie_sizes(400, 602)
    z[z < 0.06] = 0.0                      # half the levels are zero: medians of exactly 0, and of (0 + level) / 2
    z[100:160] = -z[100:160]
    for w in (1, 2, 9, 10):
        out[f"zero.burst_w{w}"] = case("burst", z, w)
    out["zero.pct_p1"] = case("pct", z, 1)
    out["zero.roc_p1"] = case("roc", z, 1)
    c, lo, hi = H.ohlc_walk(400, 603)
    c[100], c[200], c[201] = np.nan, np.inf, -1.0          # close alone: low / high hold no NaN
    for length in (1, 14):
        out[f"odd.stoch_l{length}"] = case("stoch", (c, lo, hi), length)
    return out


def length_cases():
    out = {}
    w = 10
    for n in (0, 1, w - 1, w, w + 1):
        x = H.tie_sizes(max(n, 1), 610 + n)[:n]
        out[f"length.n{n}.burst"] = case("burst", x, w)
        out[f"length.n{n}.burst_w11"] = case("burst", x, w + 1)
        out[f"length.n{n}.roc"] = case("roc", x, w)
        out[f"length.n{n}.pct"] = case("pct", x, w)
        c, lo, hi = (a[:n] for a in H.ohlc_walk(max(n, 1), 620 + n))
        out[f"length.n{n}.stoch"] = case("stoch", (c, lo, hi), w)
    return out


def reference_test_calls():
    """The calls of the reference's tests/features/test_core_utils.py to comp_burst_ratio and pct_change, inputs as that file
    builds them."""
    out = {}
    out["refcall.burst"] = case("burst", np.array([1.0, 2.0, 3.0, 4.0, 5.0]), 3)
    out["refcall.burst_zero_median"] = case("burst", np.array([0.0, 1.0, 0.0, 1.0, 2.0]), 3)
    out["refcall.pct"] = case("pct", np.array([0.0, 1.0, 2.0, 4.0]), 1)
    out["refcall.pct_nonpositive_base"] = case("pct", np.array([-1.0, -0.5, 0.0]), 1)
    return out


def refused_calls():
    """Arguments this project refuses with ValueError; what the interpreted reference does with them is recorded beside."""
    x = H.grid_walk(40, 630)
    c, lo, hi = H.ohlc_walk(40, 631)
    out = {}
    for w in (0, -2):
        out[f"refused.burst_w{w}"] = case("burst", x, w)
        out[f"refused.stoch_l{w}"] = case("stoch", (c, lo, hi), w)
    out["refused.stoch_unequal"] = case("stoch", (c, lo[:-1], hi), 5)
    out["refused.roc_p-1"] = case("roc", x, -1)
    out["refused.pct_p-3"] = case("pct", x, -3)
    return out


def run(mod, c, **kw):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ins = tuple(a.copy() for a in c["inputs"]) if c["fn"] == "stoch" else c["inputs"].copy()
            r = H.call(c["fn"], ins, c["arg"], mod=mod, **kw)
        return ("ok", np.asarray(r, np.float64))
    except Exception as e:                                        # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))


def differs(a, b, signs=False):
    """The elements in which a and b differ (NaN equals NaN); signs: a zero of the other sign differs as well."""
    if a.shape != b.shape:
        return -1
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    if signs:
        bad |= (a == b) & (np.signbit(a) != np.signbit(b))
    return int(bad.sum())


def main():
    out, manifest = {}, {}
    cases = {}
    for group in (series_cases, value_class_cases, odd_cases, length_cases, reference_test_calls, refused_calls):
        cases.update(group())
    for name, c in cases.items():
        ins = c["inputs"] if c["fn"] == "stoch" else (c["inputs"],)
        entry = {"fn": c["fn"], "arg": c["arg"], "n": int(len(ins[0]))}
        if c["source"]:
            entry["source"] = c["source"]
            entry["input_sha256"] = [H.sha256(a) for a in ins]
        else:
            for k, a in enumerate(ins):
                out[f"{name}.in{k}"] = a
        forms = ("scalar", "vector") if c["arg"] <= SCALAR_MAX else ("vector",)
        own = [run(None, c, form=form) for form in forms]
        ref = run(Reference, c)
        if name.startswith("refused."):
            if not all(o[0] == "raises" and o[1] == "ValueError" and o[1:] == own[0][1:] for o in own):
                raise SystemExit(f"{name}: the helper does not refuse this call")
            entry.update(raises=own[0][1], message=own[0][2],
                         reference=f"raises {ref[1]}" if ref[0] == "raises" else
                         f"returns ({int(np.isnan(ref[1]).sum())} NaN, {int(np.isinf(ref[1]).sum())} inf of {len(ref[1])})")
            manifest[name] = entry
            continue
        if ref[0] != "ok":
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        signs = c["fn"] != "stoch"
        for form, o in zip(forms, own):
            if o[0] != "ok" or differs(ref[1], o[1], signs) != 0:
                raise SystemExit(f"{name}: reference and helper ({form}) disagree ({o[0]}, {differs(ref[1], o[1], signs) if o[0] == 'ok' else o[1:]})"
                                 " -- case refused")
        if len(ref[1]) <= STORED_MAX:
            out[name + ".out"] = ref[1]
        else:
            entry["output_sha256"] = H.sha256(H.nan_canonical(ref[1]))
        entry.update(finite=int(np.isfinite(ref[1]).sum()), nan=int(np.isnan(ref[1]).sum()))
        manifest[name] = entry
    for k in sorted(manifest):
        print(k, {a: b for a, b in manifest[k].items() if not a.endswith("_sha256")})
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "order_stats.npz"), **out)
    with open(os.path.join(gold, "order_stats.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print(len(manifest), "cases,", os.path.getsize(os.path.join(gold, "order_stats.npz")), "bytes")


if __name__ == "__main__":
    main()
