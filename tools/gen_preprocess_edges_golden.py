#!/usr/bin/env python3
"""Writes tests/golden/preprocess_edges.json + preprocess_edges.npz: the outputs of the REFERENCE's merge_split_trades and
comp_trade_side_vector (finmlkit/bar/utils.py) on every case of tests/_preprocess_ref.py -- the second trip of the one-block scans,
moves and heads placed at thread, wave, row and tile edges, the 1e-12 and 1e-8 thresholds hit exactly, NaN / inf / -0.0 prices and
sizes, float32 absorption, timestamps at the int64 ends --, what the reference does with empty input, and the frames that
TimeBarReader._resample (finmlkit/bar/io.py, pandas' own groupby with the pandas installed here) returns for the resampling cases:
70 000 groups, groups of 1 .. 4097 rows in the four dtype combinations, the weighted-median, first / last and Kahan-sum edges.
Build container only: imports the reference in pure-Python mode through oracle/shim, like tools/gen_corr_golden.py; no GPU, nothing
of the product.

The reference is run as it is.  A case is refused unless the reference and the restatement of tests/_preprocess_ref.py agree in
every bit (dtype, length, NaN positions); its structural assertions (check_structure) must hold on the reference's output.  Outputs of
more than 2 100 elements are recorded as a sha256; inputs come from the generators and are recorded as a sha256 only.  The files
are written without timestamps and in sorted order: two runs give the same bytes.
    python tools/gen_preprocess_edges_golden.py REFERENCE_CHECKOUT        (or FINMLKIT_REFERENCE in the environment)
"""
import io
import json
import os
import sys
import warnings
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_preprocess_edges_golden.py REFERENCE_CHECKOUT (or set FINMLKIT_REFERENCE)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402

from finmlkit.bar.io import TimeBarReader  # noqa: E402
from finmlkit.bar.utils import comp_trade_side_vector, merge_split_trades  # noqa: E402

from tests import _preprocess_ref as H  # noqa: E402


def run(fn, *args):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            with np.errstate(all="ignore"):
                out = fn(*[None if a is None else a.copy() for a in args])
        return ("ok", out)
    except Exception as e:                                        # noqa: BLE001 -- recorded as data
        return ("raises", type(e).__name__, str(e))


def record(store, key, array):
    """-> the manifest entry of one output array; the array itself goes to the npz when it is short."""
    array = np.asarray(array)
    entry = {"dtype": str(array.dtype), "len": int(array.size), "sha256": H.sha256(array)}
    if array.size <= H.HASH_ABOVE:
        store[key] = array
    return entry


def write_npz(path, arrays):
    """np.savez stamps every member with the clock: write the members ourselves, in sorted order, dated 1980-01-01."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    store, manifest = {}, {}
    for name in H.TICK_CASES:
        px = H.inputs(name)
        ref = run(comp_trade_side_vector, px)
        if ref[0] != "ok":
            raise SystemExit(f"{name}: the reference raises {ref[1:]} -- case refused")
        H.same(H.expected_uncached(name), ref[1], f"{name}: restatement against the reference")
        info = H.check_structure(name, ref[1])
        manifest[name] = {"kind": "tick", "n": int(len(px)), "input_sha256": H.sha256(px), "out": record(store, name + "__out", ref[1]),
                          "structure": {k: int(v) for k, v in info.items()}}
        print(name, manifest[name]["n"], manifest[name]["structure"], flush=True)
    for name in H.MERGE_CASES:
        ts, px, am, ibm = H.inputs(name)
        entry = {"kind": "merge", "n": int(len(ts)), "input_sha256": H.sha256(ts, px, am, ibm)}
        outs = {}
        for tag, flag in (("side", ibm), ("noside", None)):
            ref = run(merge_split_trades, ts, px, am, flag)
            if ref[0] != "ok":
                raise SystemExit(f"{name} ({tag}): the reference raises {ref[1:]} -- case refused")
            own = H.expected_uncached(name, flag is not None)
            for k, a, b in zip(H.MERGE_KEYS, own, ref[1]):
                H.same(a, b, f"{name} ({tag}): restatement against the reference, {k}")
            outs[tag] = ref[1]
            entry[tag] = {k: record(store, f"{name}__{tag}_{k}", a) for k, a in zip(H.MERGE_KEYS, ref[1])}
            entry[tag]["m"] = int(len(ref[1][0]))
        entry["structure"] = {k: int(v) for k, v in H.check_structure(name, outs["side"], outs["noside"]).items()}
        manifest[name] = entry
        print(name, entry["n"], entry["side"]["m"], entry["noside"]["m"], entry["structure"], flush=True)
    for name, (kind, make) in H.REFUSED_CASES.items():
        args = make()
        ref = run(comp_trade_side_vector, args) if kind == "tick" else run(merge_split_trades, *args)
        own = run(H.comp_trade_side_vector, args) if kind == "tick" else run(H.merge_split_trades, *args)
        if ref[0] != "raises" or own[0] != "raises" or own[1] != ref[1]:
            raise SystemExit(f"{name}: reference {ref[:2]}, restatement {own[:2]} -- case refused")
        manifest[name] = {"kind": kind, "n": 0, "refused": True, "raises": ref[1], "reason": ref[2]}
        print(name, manifest[name], flush=True)
    for name in H.RESAMPLE_CASES:
        seg, cols = H.rs_inputs(name)
        df, timeframe = H.rs_frame(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = TimeBarReader._resample(None, df.copy(), timeframe)        # pandas' own groupby, this machine's pandas
        if list(res.columns) != list(H.RS_COLS):
            raise SystemExit(f"{name}: the reference returns the columns {list(res.columns)} -- case refused")
        own = H.rs_expected(name)
        kept = res.index.values.astype("datetime64[ns]").astype(np.int64) // (86_400 * 1_000_000_000)
        valid = np.zeros(len(seg) - 1, dtype=np.uint8)
        valid[kept] = 1
        H.same(own[8], valid, f"{name}: which groups the reference keeps")
        entry = {"kind": "resample", "n": int(seg[-1]), "groups": int(len(seg) - 1), "kept": int(valid.sum()),
                 "input_sha256": H.sha256(seg, *cols), "pandas": __import__("pandas").__version__, "out": {}}
        for k, a in zip(H.RS_COLS, own):
            H.same(a[valid == 1], res[k].values, f"{name}: restatement against the reference, {k}")
            entry["out"][k] = record(store, f"{name}__out_{k}", res[k].values)
        entry["out"]["valid"] = record(store, f"{name}__out_valid", valid)
        entry["structure"] = {k: int(v) for k, v in H.rs_check_structure(name, own).items()}
        manifest[name] = entry
        print(name, entry["groups"], entry["kept"], entry["structure"], flush=True)
    gold = os.path.join(ROOT, "tests", "golden")
    write_npz(os.path.join(gold, "preprocess_edges.npz"), store)
    with open(os.path.join(gold, "preprocess_edges.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(len(manifest), "cases,", len(store), "arrays,", os.path.getsize(os.path.join(gold, "preprocess_edges.npz")), "bytes")


if __name__ == "__main__":
    main()
