#!/usr/bin/env python3
"""Writes tests/golden/vp_edges.npz + vp_edges.json: what the REFERENCE's volume_profile_rolling (feature/core/volume.py:393-456)
returns on the hand-built footprints of tests/_vp_ref.py -- every case of volume kind 1 (multiples of 2**-4: every float32 sum is
exact), the kind-3 cases (NaN / +inf volumes) on which the gate below holds -- and how it answers the refused calls.  Build container
only: imports the reference in its pinned pure-Python mode through oracle/shim, by the recipe of oracle/gen_vp_stages.py
(numba.typed.List of per-bar arrays); no GPU, nothing of the product.

Stored: the four outputs of every recorded case (one flat array each; the manifest holds where a case starts), the case's
parameters and the sha256 of its inputs, for a one-window case the sha256 of the reference's stage outputs (aggregate_footprint,
bucket_price_levels, comp_poc_hva_lva, calc_volume_percentage_above_poc), for a refused call the exception's type and message or
"returns".  Inputs are regenerated from the table; nothing of the reference's text is stored.

The gate.  On every recorded case the restatement equals the reference in every bit (rolling outputs and stages).
Scalar semantics.  The interpreted reference keeps np.float32 scalars where the typed function has float64 (the walk's sums, the
threshold, the share's sum and quotient: DESIGN.md section 5 rows T1 / T3).  Per recorded case the smallest |cum - threshold| over
every test of the walk's condition is computed ("walk_gap"): it must be exactly 0 with a threshold the float32 reading computes
exactly (zero, or va_pct / 100 and the product representable), or larger than the float32 rounding of the threshold (|thr| * 2**-22: one
rounding of va_pct / 100, one of the product) -- else the case is a mistake in the table.  The share is compared bit for bit.
    python tools/gen_vp_edges_golden.py <reference checkout>
"""
import json
import math
import os
import sys
import warnings
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_vp_edges_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402
from finmlkit.feature.core import volume as RV  # noqa: E402
from numba.typed import List as NList  # noqa: E402

from tests import _vp_ref as H  # noqa: E402

KEYS = ("poc", "hva", "lva", "pct")


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: two runs write the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.ascontiguousarray(arrays[key]), allow_pickle=False)


def ragged(off, a):
    return NList([a[off[i]:off[i + 1]] for i in range(len(off) - 1)])


def reference_rolling(data, window, n_bins, tick, va):
    ts, hi, lo, off, lv, bv, sv = data
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return RV.volume_profile_rolling(ts, hi, lo, ragged(off, lv), ragged(off, bv), ragged(off, sv), window, n_bins, tick, va)


def walk_gap(name):
    """The smallest |cum - threshold| over the walks of a case, and whether each threshold met exactly is float32-exact."""
    c = H.CASES[name]
    ts, hi, lo, off, lv, bv, sv = H.inputs(name)
    gap, exact_ok, thr_at = math.inf, True, 0.0
    wn = int(c["window"] * 1e9)
    for i in range(H.first_bar(ts, c["window"]), len(ts)):
        levels, ab, as_ = H.aggregate_footprint(ts, hi, lo, off, lv, bv, sv, int(ts[i]) - wn, int(ts[i]), c["tick"])
        tot = ab + as_
        if c["n_bins"] is not None:
            levels, tot = H.bucket_price_levels(levels, tot, c["n_bins"])
        trace = []
        H.comp_poc_hva_lva(levels, tot, c["va"], trace=trace)
        for cum, thr in trace:
            if not (math.isfinite(cum) and math.isfinite(thr)):
                continue                                         # NaN / inf: `cum < thr` reads the same in float32 and float64
            g = abs(cum - thr)
            if g == 0.0:
                f = c["va"] / 100.0
                exact_ok = exact_ok and (thr == 0.0 or (float(np.float32(f)) == f and float(np.float32(thr)) == thr))
            elif g < gap:
                gap, thr_at = g, thr
    return gap, exact_ok, thr_at


def main():
    flat = {k: [] for k in KEYS}
    manifest, left_out, at = {}, [], 0
    n_stage = 0
    for name, c in H.CASES.items():
        if c["kind"] == 2:
            continue
        data = H.inputs(name)
        (own, _info) = H.expected(name)
        ref = reference_rolling(data, c["window"], c["n_bins"], c["tick"], c["va"])
        same = all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and
                   np.array_equal(a.view(np.uint32)[~np.isnan(a.astype(np.float64))], b.view(np.uint32)[~np.isnan(b.astype(np.float64))])
                   for a, b in zip(own, ref))
        if not same and c["kind"] == 3:
            left_out.append(name)                                # inexact volumes with a NaN / inf: the float32 scalars went elsewhere
            continue
        assert same, f"{name}: the restatement differs from the reference"
        gap, exact_ok, thr_at = walk_gap(name)
        if c["kind"] == 1:
            assert exact_ok, f"{name}: cum == threshold on a threshold float32 does not compute exactly"
            assert gap > abs(thr_at) * 2.0 ** -22, f"{name}: walk gap {gap} within the float32 rounding of the threshold {thr_at}"
        entry = dict(window=c["window"], n_bins=c["n_bins"], tick=c["tick"], va=c["va"], kind=c["kind"], n=int(len(ref[0])), at=at,
                     input_sha256=H.input_hash(name), walk_gap=(None if math.isinf(gap) else gap))
        if c["one"]:
            r = H.stage_outputs(RV, data, c["n_bins"], c["tick"], c["va"], as_lists=ragged)
            o = H.stage_outputs(H, data, c["n_bins"], c["tick"], c["va"])
            assert len(r) == len(o) and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() or
                                            (a.shape == b.shape and np.isnan(a).any() and np.array_equal(a, b, equal_nan=True))
                                            for a, b in zip(r, o)), f"{name}: a stage of the restatement differs from the reference"
            entry["stages_sha256"] = H.stages_hash(r)
            n_stage += 1
        for k, a in zip(KEYS, ref):
            flat[k].append(a)
        at += len(ref[0])
        manifest[name] = entry
    refused = {}
    for name, c in H.REFUSALS.items():
        if name == "above_16m_levels":
            refused[name] = dict(reference="not run: the reference has no limit; the refusal is the product's capacity")
            continue
        try:
            out = reference_rolling(c["inputs"], c["window"], c["n_bins"], c["tick"], c["va"])
            refused[name] = dict(reference="returns", poc=[int(x) for x in out[0]])
        except Exception as e:                                   # noqa: BLE001 -- whatever the reference raises is the record
            refused[name] = dict(reference=type(e).__name__, message=str(e))
        refused[name]["input_sha256"] = H.sha256(*c["inputs"])
    out = dict(cases=manifest, refused=refused, left_out=sorted(left_out),
               note="walk_gap: the smallest non-zero |cum - threshold| of the case's walks; no seed had to be changed for the share")
    gold = os.path.join(ROOT, "tests", "golden")
    save_npz(os.path.join(gold, "vp_edges.npz"), {k: np.concatenate(v) for k, v in flat.items()})
    with open(os.path.join(gold, "vp_edges.json"), "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print(len(manifest), "cases recorded,", n_stage, "with stages,", at, "outputs each;", os.path.getsize(os.path.join(gold, "vp_edges.npz")), "+",
          os.path.getsize(os.path.join(gold, "vp_edges.json")), "bytes; left out:", left_out)
    for n, r in refused.items():
        print("  refused", n, "->", r["reference"], r.get("message", ""))


if __name__ == "__main__":
    main()
