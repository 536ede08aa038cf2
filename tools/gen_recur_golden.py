#!/usr/bin/env python3
"""Writes tests/golden/recur.npz + recur.json: outputs of the REFERENCE's recursive indicators -- ewma (feature/core/ma.py),
rsi_wilder (feature/core/momentum.py), true_range and atr (feature/core/volatility.py), adx_core (feature/core/trend.py) -- on seeded
series that the tests regenerate (tests/_recur_ref.py: grid walks and OHLC walks in integer arithmetic), on series with NaN in and
after the seed windows, on the edge lengths, on atr's window 0, and the refused arguments.  Build container only: imports the
reference in pure-Python mode through oracle/shim, like tools/gen_order_golden.py; no GPU, nothing of the product.

The truth is the UNTOUCHED reference.  A case is refused unless the reference and tests/_recur_ref.py agree in every element, NaN
positions and the sign of every zero included: the restatement is sequential, so it can.  (The one place where the two could part
is the order in which a `max` meets a NaN in adx_core, which has no NaN checks; the restatement takes Python's order, the first of
the largest, and the gate below shows that nothing differs.)  Cases of more than 2100 elements record `output_sha256` (over the
output's bytes, every NaN made the canonical quiet NaN) instead of the output: the host test recomputes it from the restatement.

The group runs.* (flat, one-sided, rangeless and zero runs behind a walk, up to and past the step at which a decaying state leaves
the normal range, and memories of several tiles) also records, from the same recurrences in np.longdouble (tests/_recur_ref.py:
exact_states, compare_mask): `compare`, the index ranges in which every live state is exactly 0.0 or at least 2^-969; `left_out`,
how many elements lie outside them; `ref_dev`, the restatement's largest deviation from the long-double output over `compare` in
the function's measure.  The GPU tests take their tolerance from `ref_dev`, never from a kernel's output.
    python tools/gen_recur_golden.py <reference checkout>
"""
import json
import math
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_recur_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

import finmlkit.feature.core.ma as RMA  # noqa: E402
import finmlkit.feature.core.momentum as RMO  # noqa: E402
import finmlkit.feature.core.trend as RTR  # noqa: E402
import finmlkit.feature.core.volatility as RVO  # noqa: E402

from tests import _recur_ref as H  # noqa: E402


class Reference:
    """The reference's five functions under the names tests/_recur_ref.call expects."""
    ewma = staticmethod(RMA.ewma)
    rsi_wilder = staticmethod(RMO.rsi_wilder)
    true_range = staticmethod(RVO.true_range)
    atr = staticmethod(RVO.atr)
    adx_core = staticmethod(RTR.adx_core)


GENERATORS = {"grid_walk": lambda *a: (H.grid_walk(*a),), "hlc_walk": H.hlc_walk,
              "run_close": lambda *a: (H.run_series(*a)[2],), "run_hlc": H.run_series}
TILE = 2048                            # elements per workgroup of the scans (csrc/fmk_recur_core.h: RC_TILE)
STORED_MAX = 2100                      # longer cases record the hash of their output, not the output
WINDOWS = (1, 2, 3, 14, 100)


def case(fn, inputs, args, gen=None, gen_args=None):
    """`gen`, `gen_args`: how the tests regenerate the inputs (a name of GENERATORS and its arguments); without them they are stored."""
    return dict(fn=fn, inputs=tuple(np.asarray(a, np.float64) for a in inputs), args=list(args),
                source={"gen": gen, "args": gen_args} if gen else None)


def seeded(fn, args, gen, *gen_args):
    return case(fn, GENERATORS[gen](*gen_args), args, gen, list(gen_args))


def series_cases():
    out = {}
    n = 1200
    for k, w in enumerate(WINDOWS):
        out[f"walk.ewma_s{w}"] = seeded("ewma", [w], "grid_walk", n, 700 + k, 35, 0.0)
        out[f"walk.rsi_w{w}"] = seeded("rsi", [w], "grid_walk", n, 710 + k, 35, 0.0)
        out[f"walk.atr_sma_w{w}"] = seeded("atr", [w, False, False], "hlc_walk", n, 720 + k)
        out[f"walk.atr_ema_w{w}"] = seeded("atr", [w, True, False], "hlc_walk", n, 720 + k)
        out[f"walk.adx_l{w}"] = seeded("adx", [w], "hlc_walk", n, 730 + k)
    out["walk.atr_sma_norm_w14"] = seeded("atr", [14, False, True], "hlc_walk", n, 740)
    out["walk.atr_ema_norm_w14"] = seeded("atr", [14, True, True], "hlc_walk", n, 740)
    out["walk.tr"] = seeded("tr", [], "hlc_walk", n, 741)
    out["held.rsi_w14"] = seeded("rsi", [14], "grid_walk", n, 742, 1, 0.9)       # flat stretches: no loss for a while
    out["held.adx_l14"] = seeded("adx", [14], "hlc_walk", n, 743, 2, 1, 0.9)     # bars without a range: zero sums
    out["held.atr_ema_w14"] = seeded("atr", [14, True, False], "hlc_walk", n, 743, 2, 1, 0.9)
    out["held.tr"] = seeded("tr", [], "hlc_walk", n, 743, 2, 1, 0.9)
    for fn, args, gen in (("ewma", [14], "grid_walk"), ("rsi", [14], "grid_walk"), ("atr", [14, True, False], "hlc_walk"),
                          ("atr", [14, False, True], "hlc_walk"), ("adx", [14], "hlc_walk"), ("tr", [], "hlc_walk")):
        tag = fn + ("_ema" if args[1:2] == [True] else "_sma" if fn == "atr" else "")
        out[f"long.{tag}"] = seeded(fn, args, gen, 70_000, 750)
    return out


def nan_cases():
    out = {}
    y = H.grid_walk(600, 760)
    y[300] = np.nan
    out["nan.ewma_s14"] = case("ewma", (y,), [14])
    c = H.grid_walk(600, 761)
    c[5] = np.nan                          # inside the first window of 14: NaN everywhere
    out["nan.rsi_seed_w14"] = case("rsi", (c,), [14])
    c = H.grid_walk(600, 762)
    c[300] = np.nan                        # after it: two differences count as no gain and no loss
    out["nan.rsi_after_w14"] = case("rsi", (c,), [14])
    h, lo, c = (a.copy() for a in H.hlc_walk(600, 763))
    h[50:53] = np.nan                      # shorter than the windows below
    lo[150:190] = np.nan                   # longer
    c[300] = np.nan
    out["nan.tr"] = case("tr", (h, lo, c), [])
    for w in (1, 2, 3, 14):
        out[f"nan.atr_sma_w{w}"] = case("atr", (h, lo, c), [w, False, False])
    out["nan.atr_sma_norm_w14"] = case("atr", (h, lo, c), [14, False, True])
    out["nan.atr_ema_w14"] = case("atr", (h, lo, c), [14, True, False])
    h, lo, c = (a.copy() for a in H.hlc_walk(600, 764))
    lo[3] = np.nan                         # in the first window: skipped by the seed's mean
    out["nan.atr_ema_seed_w14"] = case("atr", (h, lo, c), [14, True, True])
    h, lo, c = (a.copy() for a in H.hlc_walk(60, 765))
    h[2] = lo[2] = c[2] = np.nan           # the reference's NaN at bar 2
    for w in (1, 2, 3, 4):
        out[f"quirk.atr_sma_w{w}"] = case("atr", (h, lo, c), [w, False, False])
    h, lo, c = (a.copy() for a in H.hlc_walk(60, 765))
    h[2] = lo[2] = np.nan                  # close is a number: no quirk
    out["quirk.atr_sma_close_w3"] = case("atr", (h, lo, c), [3, False, False])
    h, lo, c = (a.copy() for a in H.hlc_walk(600, 766))
    h[9] = np.nan                          # in the seed window of the sums: all zeros
    out["nan.adx_seed_l14"] = case("adx", (h, lo, c), [14])
    h, lo, c = (a.copy() for a in H.hlc_walk(600, 767))
    c[300] = np.nan                        # after the seeds: dx is 0.0 from there on
    out["nan.adx_after_l14"] = case("adx", (h, lo, c), [14])
    h, lo, c = (a.copy() for a in H.hlc_walk(600, 768))
    lo[20] = np.nan                        # between the two seeds
    out["nan.adx_between_l14"] = case("adx", (h, lo, c), [14])
    return out


def length_cases():
    out = {}
    w = 10
    for n in (0, 1, 2, w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1):
        y = H.grid_walk(max(n, 2), 770 + n)[:n]
        h, lo, c = (a[:n] for a in H.hlc_walk(max(n, 2), 780 + n))
        if n:
            out[f"length.n{n}.ewma"] = case("ewma", (y,), [w])
        out[f"length.n{n}.rsi"] = case("rsi", (y,), [w])
        if n:
            out[f"length.n{n}.tr"] = case("tr", (h, lo, c), [])
            out[f"length.n{n}.atr_sma"] = case("atr", (h, lo, c), [w, False, False])
            out[f"length.n{n}.atr_ema"] = case("atr", (h, lo, c), [w, True, False])
        out[f"length.n{n}.adx"] = case("adx", (h, lo, c), [w])
    h, lo, c = H.hlc_walk(40, 790)
    out["window0.atr_sma"] = case("atr", (h, lo, c), [0, False, False])
    out["window0.atr_ema"] = case("atr", (h, lo, c), [0, True, True])
    return out


RUN_FUNCTIONS = (("rsi_flat", "rsi", "flat"), ("rsi_rising", "rsi", "rising"), ("atr_ema", "atr", "flat"), ("atr_ema_norm", "atr", "flat"),
                 ("adx", "adx", "flat"), ("ewma_zeros", "ewma", "zeros"))
RUN_STARTS = (TILE, TILE + 1000 + 3)   # on a tile edge and off one
# window -> run lengths inside the contract (0.9 x the horizon at the longest) and whether the run is tried off the tile edge too
RUN_LENGTHS = {2: ((100, True), (870, True)), 3: ((1490, True),), 5: ((TILE + 8, False), (2700, True)),
               14: ((TILE + 8, False), (2 * TILE + 100, True), (8156, True)), 100: ((3 * TILE, True),)}


def run_args(tag, fn, w):
    """ewma takes the span with the same a = (w - 1) / w, adx_core the window as its length."""
    return {"rsi": [w], "atr": [w, True, tag.endswith("norm")], "adx": [w], "ewma": [2 * w - 1]}[fn]


def run_case(tag, fn, kind, w, start, length, seed):
    gen = "run_close" if fn in ("rsi", "ewma") else "run_hlc"
    return seeded(fn, run_args(tag, fn, w), gen, kind, start + length + 1500, seed, start, length)


def runs_cases():
    """b: decaying runs inside the contract; c: 1.3 x the steps to the smallest subnormal; e: memories of several tiles."""
    out = {}
    seed = 900
    for w, lengths in RUN_LENGTHS.items():
        for length, both in lengths:
            for start in RUN_STARTS if both else RUN_STARTS[:1]:
                for tag, fn, kind in RUN_FUNCTIONS:
                    seed += 1
                    out[f"runs.b.{tag}.w{w}.s{start}.l{length}"] = run_case(tag, fn, kind, w, start, length, seed)
    for w in (2, 3, 14):
        length = int(1.3 * math.log(2.0 ** -1074) / math.log((w - 1) / w))
        for start in RUN_STARTS:
            for tag, fn, kind in (RUN_FUNCTIONS[0], RUN_FUNCTIONS[2], RUN_FUNCTIONS[4]):
                if w == 2 and fn != "rsi":
                    continue
                seed += 1
                out[f"runs.c.{tag}.w{w}.s{start}.l{length}"] = run_case(tag, fn, kind, w, start, length, seed)
    for w in (3 * TILE + 1, 10 * TILE - 1):
        out[f"runs.e.rsi.w{w}"] = seeded("rsi", [w], "grid_walk", w + TILE + 9, 1101, 35, 0.0)
        out[f"runs.e.atr_ema.w{w}"] = seeded("atr", [w, True, False], "hlc_walk", w - 1 + TILE + 9, 1102)
    for length in (2 * TILE + 1, 5 * TILE):
        out[f"runs.e.adx.l{length}"] = seeded("adx", [length], "hlc_walk", 2 * length - 1 + TILE + 9, 1103)
    for span in (4097, 200_001):
        out[f"runs.e.ewma.s{span}"] = seeded("ewma", [span], "grid_walk", 4 * TILE + 9, 1104, 35, 0.0)
    return out


def exact_record(name, c, own):
    """compare, left_out, ref_dev of a runs.* case; refuses one whose restatement and long-double evaluation part in a NaN or,
    for adx_core, in a zero over `compare`."""
    states, exact = H.exact_states(c["fn"], c["inputs"], c["args"])
    mask = H.compare_mask(c["fn"], c["args"], states)
    e64 = exact.astype(np.float64)
    if (np.isnan(own) != np.isnan(e64))[mask].any() or (c["fn"] == "adx" and ((own == 0) != (e64 == 0))[mask].any()):
        raise SystemExit(f"{name}: restatement and long-double evaluation differ in a NaN or a zero inside `compare` -- case refused")
    return dict(compare=H.mask_ranges(mask), left_out=int((~mask).sum()), ref_dev=H.deviation(c["fn"], own, exact, mask))


def refused_calls():
    """Arguments this project refuses with ValueError; what the interpreted reference does with them is recorded beside."""
    y = H.grid_walk(40, 791)
    h, lo, c = H.hlc_walk(40, 792)
    out = {}
    out["refused.ewma_s0"] = case("ewma", (y,), [0])
    out["refused.rsi_w0"] = case("rsi", (y,), [0])
    out["refused.adx_l0"] = case("adx", (h, lo, c), [0])
    out["refused.atr_w-1"] = case("atr", (h, lo, c), [-1, False, False])
    out["refused.tr_unequal"] = case("tr", (h, lo[:-1], c), [])
    out["refused.atr_unequal"] = case("atr", (h, lo, c[:-1]), [5, False, False])
    return out


def run(mod, c):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            r = H.call(c["fn"], tuple(a.copy() for a in c["inputs"]), c["args"], mod=mod)
        return ("ok", np.asarray(r, np.float64))
    except Exception as e:                                        # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))


def differs(a, b):
    """The elements in which a and b differ: NaN equals NaN, a zero of the other sign differs."""
    if a.shape != b.shape:
        return -1
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    bad |= (a == b) & (np.signbit(a) != np.signbit(b))
    return int(bad.sum())


def main():
    out, manifest = {}, {}
    cases = {}
    for group in (series_cases, nan_cases, length_cases, refused_calls, runs_cases):
        cases.update(group())
    for name, c in cases.items():
        ins = c["inputs"]
        entry = {"fn": c["fn"], "args": c["args"], "n": int(len(ins[0]))}
        if c["source"]:
            entry["source"] = c["source"]
            entry["input_sha256"] = [H.sha256(a) for a in ins]
        else:
            for k, a in enumerate(ins):
                out[f"{name}.in{k}"] = a
        own, ref = run(None, c), run(Reference, c)
        if name.startswith("refused."):
            if not (own[0] == "raises" and own[1] == "ValueError"):
                raise SystemExit(f"{name}: the helper does not refuse this call")
            entry.update(raises=own[1], message=own[2],
                         reference=f"raises {ref[1]}" if ref[0] == "raises" else
                         f"returns ({int(np.isnan(ref[1]).sum())} NaN, {int(np.isinf(ref[1]).sum())} inf of {len(ref[1])})")
            manifest[name] = entry
            continue
        if ref[0] != "ok":
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        if own[0] != "ok" or differs(ref[1], own[1]) != 0:
            raise SystemExit(f"{name}: reference and helper disagree ({own[0]}, {differs(ref[1], own[1]) if own[0] == 'ok' else own[1:]})"
                             " -- case refused")
        if any(np.isinf(a).any() for a in ins):
            raise SystemExit(f"{name}: an infinite input -- outside the contract")
        if len(ref[1]) <= STORED_MAX:
            out[name + ".out"] = ref[1]
        else:
            entry["output_sha256"] = H.sha256(H.nan_canonical(ref[1]))
        entry.update(finite=int(np.isfinite(ref[1]).sum()), nan=int(np.isnan(ref[1]).sum()), zeros=int((ref[1] == 0).sum()))
        if name.startswith("runs."):
            entry.update(exact_record(name, c, own[1]))
        manifest[name] = entry
    for k in sorted(manifest):
        print(k, {a: b for a, b in manifest[k].items() if not a.endswith("_sha256")})
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "recur.npz"), **out)
    with open(os.path.join(gold, "recur.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print(len(manifest), "cases,", os.path.getsize(os.path.join(gold, "recur.npz")), "bytes")


if __name__ == "__main__":
    main()
