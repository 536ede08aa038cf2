#!/usr/bin/env python3
"""Writes tests/golden/vpdev_edges.npz + vpdev_edges.json: what the REFERENCE's volume_profile_developing and trim_trailing_zeros
(feature/core/volume.py:459-569) return on the hand-built footprints of tests/_vpdev_ref.py, and how the reference answers the refused
calls.  Build container only: imports the reference in its pinned pure-Python mode through oracle/shim, as tools/gen_vp_edges_golden.py
does; no GPU, nothing of the product.

Position.  The reference writes bar t's outputs at index t of arrays as long as the range, which fails for every range that does not
begin at bar 0.  Every range is therefore given to the reference on the arrays SLICED from its first bar (same stamps): that is the
yardstick of include/fmk.h item 5.
Stored: poc / hva / lva of every recorded range (one flat array each; the manifest holds where a case starts and how long its ranges
are), the case's parameters and the sha256 of its inputs; trim_trailing_zeros on the profiles of _vpdev_ref.TRIM_PROFILES; for a refused call the type and
message of what the reference did, or "returns".  Inputs are regenerated from the table; nothing of the reference's text is stored.

Gates.  On every exact-volume (kind 1) case the restatement equals the reference in every bit, and the walk_gap gate of
tools/gen_vp_edges_golden.py holds (float32 against float64 walk scalars).  A lognormal (kind 2) or NaN / inf (kind 3) case on which
the reference differs from the restatement is listed under left_out, not recorded; more than 5 % of them left out fails the run.
Refusals: where include/fmk.h follows the reference (empty range, NaN low or high, NaN tick, all-zero profile under bucketing) the
reference must raise ValueError as the restatement does, and the calls that must return are compared bit for bit; where the contract
departs from the interpreted reference on purpose (DEPARTS below) the reference's behaviour is only recorded.
    python tools/gen_vpdev_golden.py <reference checkout>
"""
import contextlib
import io
import json
import math
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_vpdev_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
sys.path.insert(3, HERE)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402
from finmlkit.feature.core import volume as RV  # noqa: E402

from gen_vp_edges_golden import ragged, save_npz  # noqa: E402
from tests import _vp_ref as H  # noqa: E402
from tests import _vpdev_ref as D  # noqa: E402

KEYS = ("poc", "hva", "lva")
LEFT_OUT_CAP = 0.05
# the level rules, a tick that is not positive and n_bins 0: include/fmk.h refuses where the interpreted reference folds the level onto
# the lowest one, raises IndexError / OverflowError, or divides by zero into 0; the capacity is the product's own
DEPARTS = ("level_below.first64", "level_below.rest", "level_above.first64", "level_above.rest", "n_bins_0", "tick_0", "tick_negative",
           "above_16m_levels")


def reference(data, start_ts, end_ts, n_bins, tick, va):
    """The reference on the arrays sliced from the range's first bar."""
    ts, hi, lo, off, lv, bv, sv = data
    s = int(np.searchsorted(ts, start_ts))
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        return RV.volume_profile_developing(ts[s:], hi[s:], lo[s:], ragged(off[s:], lv), ragged(off[s:], bv), ragged(off[s:], sv),
                                            start_ts, end_ts, n_bins, tick, va)


def same(own, ref):
    return all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(own, ref))


def walk_gap(name):
    c = D.CASES[name]
    ts, hi, lo, off, lv, bv, sv = D.inputs(name)
    gap, exact_ok, thr_at = math.inf, True, 0.0
    for s, e in D.bar_ranges(name):
        trace = []
        D.developing_range(hi, lo, off, lv, bv, sv, s, e, c["n_bins"], c["tick"], c["va"], trace=trace)
        for cum, thr in trace:
            if not (math.isfinite(cum) and math.isfinite(thr)):
                continue
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
    for name, c in D.CASES.items():
        own, _info = D.expected(name)
        refs = [reference(D.inputs(name), a, b, c["n_bins"], c["tick"], c["va"]) for a, b in D.stamps(name)]
        ok = all(same(o, r) for o, r in zip(own, refs))
        if not ok and c["kind"] != 1:
            left_out.append(name)
            continue
        assert ok, f"{name}: the restatement differs from the reference"
        gap = math.inf
        if c["kind"] == 1:
            gap, exact_ok, thr_at = walk_gap(name)
            assert exact_ok, f"{name}: cum == threshold on a threshold float32 does not compute exactly"
            assert gap > abs(thr_at) * 2.0 ** -22, f"{name}: walk gap {gap} within the float32 rounding of the threshold {thr_at}"
        lens = [int(len(r[1])) for r in refs]
        manifest[name] = dict(n_bins=c["n_bins"], tick=c["tick"], va=c["va"], kind=c["kind"], at=at, lens=lens, input_sha256=D.input_hash(name),
                              walk_gap=(None if math.isinf(gap) else gap))
        for r in refs:
            for k, a in zip(KEYS, r[1:]):
                flat[k].append(np.asarray(a, np.int32))
        at += sum(lens)
    inexact = [n for n, c in D.CASES.items() if c["kind"] != 1]
    assert len(left_out) <= LEFT_OUT_CAP * len(inexact), f"left out {len(left_out)} of {len(inexact)}: {left_out}"
    refused = {}
    for name, c in list(D.REFUSALS.items()) + list(D.RETURNS.items()):
        if name == "above_16m_levels":
            refused[name] = dict(reference="not run: the reference has no limit; the refusal is the product's capacity")
            continue
        a, b = D.refusal_stamps(c)
        try:
            out = reference(c["inputs"], a, b, c["n_bins"], c["tick"], c["va"])
            refused[name] = dict(reference="returns", poc=[int(x) for x in out[1]], hva=[int(x) for x in out[2]], lva=[int(x) for x in out[3]])
        except Exception as e:                                   # noqa: BLE001 -- whatever the reference raises is the record
            refused[name] = dict(reference=type(e).__name__, message=str(e))
        refused[name]["input_sha256"] = H.sha256(*c["inputs"])
        if name in D.RETURNS:
            s, e = c["span"]
            own = D.developing_range(*c["inputs"][1:], s, e, c["n_bins"], c["tick"], c["va"])
            assert refused[name]["reference"] == "returns" and [refused[name][k] for k in KEYS] == [[int(x) for x in o] for o in own], name
        elif name not in DEPARTS:
            assert refused[name]["reference"] == "ValueError" and issubclass(c["error"], ValueError), (name, refused[name])
    # trim_trailing_zeros: inputs, trimmed levels and volumes of all profiles in ONE float64 array (every value is exact there)
    trims, parts = {}, []
    arrays = {k: np.concatenate(v) for k, v in flat.items()}
    for j, v in enumerate(D.TRIM_PROFILES):
        lv = np.arange(100, 100 + len(v), dtype=np.int32)
        rl, rv = RV.trim_trailing_zeros(lv, v)
        assert np.asarray(rv).dtype == v.dtype
        parts += [v.astype(np.float64), np.asarray(rl, np.float64), np.asarray(rv, np.float64)]
        trims[f"trim{j}"] = dict(n_in=len(v), n_out=len(rl), dtype=v.dtype.name)
    arrays["trim"] = np.concatenate(parts)
    out = dict(cases=manifest, refused=refused, left_out=sorted(left_out), trims=trims,
               note="walk_gap: the smallest non-zero |cum - threshold| of the case's walks")
    gold = os.path.join(ROOT, "tests", "golden")
    save_npz(os.path.join(gold, "vpdev_edges.npz"), arrays)
    with open(os.path.join(gold, "vpdev_edges.json"), "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print(len(manifest), "cases recorded,", at, "rows;", os.path.getsize(os.path.join(gold, "vpdev_edges.npz")), "+",
          os.path.getsize(os.path.join(gold, "vpdev_edges.json")), "bytes; left out:", left_out)
    for n, r in refused.items():
        print("  refused", n, "->", r["reference"], r.get("message", "")[:100])


if __name__ == "__main__":
    main()
