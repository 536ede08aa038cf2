#!/usr/bin/env python3
"""Writes tests/golden/clock.npz + clock.json: outputs of the REFERENCE's BarDuration, BarDurationEWMA, BarRate, ORBBreak._pd and
DirRunLen.numba_core (finmlkit/feature/transforms.py:1511-1548, :1460-1508, :1210-1270, :1122-1207, :1636-1664) on the cases of
tests/_clock_ref.py (`cases`), whose seeded inputs the tests regenerate: the inputs are recorded as digests and sources only.  Build
container only: imports the reference through oracle/shim, like tools/gen_shape_golden.py; needs the built library for the kernels'
tile sizes alone (finmlkit_amd.feature.core.clock.geometry: no GPU), nothing else of the product.

The truth is the UNTOUCHED reference.  A case is refused unless the reference and the restatement (tests/_clock_ref.py) agree: in
every bit for bar_duration, bar_rate, dir_run_len and orb_break; for bar_duration_ewma in every NaN position and within 1e-9
relative (the project's contract for recurrence scans), the largest deviation measured being recorded under "dew_ref_dev".
DirRunLen.numba_core runs under the interpreter here, where NumPy 2 raises OverflowError on the int8 store of a run of 128: the
untouched reference pins runs up to 127, the cases marked "reference": false are the restatement's alone (the compiled store keeps
the low 8 bits), and the JSON says so; a single element is such a case too (the reference reads x[1], IndexError here).  The names the reference gives its outputs are recorded under "names".
    python tools/gen_clock_golden.py <reference checkout>
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FINMLKIT_REFERENCE")
if not REF:
    raise SystemExit("usage: gen_clock_golden.py <reference checkout>   (or FINMLKIT_REFERENCE in the environment)")
sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)
os.environ["NUMBA_DISABLE_JIT"] = "1"

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import finmlkit.feature.transforms as RT  # noqa: E402

from finmlkit_amd.feature.core import clock  # noqa: E402
from tests import _clock_ref as H  # noqa: E402


def frame(ts, **cols):
    cols = cols or {"close": np.zeros(len(ts))}
    return pd.DataFrame(cols, index=pd.DatetimeIndex(np.asarray(ts, np.int64)))


def reference(fn, inputs, args):
    """The untouched reference on the case -> a tuple of arrays."""
    if fn == "dur":
        return (np.asarray(RT.BarDuration(*args)(frame(inputs[0]), backend="pd").values, np.float64),)
    if fn == "dew":
        return (np.asarray(RT.BarDurationEWMA(*args)(frame(inputs[0]), backend="pd").values, np.float64),)
    if fn == "rate":
        return (np.asarray(RT.BarRate(pd.Timedelta(seconds=args[0]))(frame(inputs[0]), backend="pd").values, np.float64),)
    if fn == "run":
        return (np.asarray(RT.DirRunLen.numba_core(np.asarray(inputs[0], np.float64))),)
    ts, high, low, close = inputs
    lg, sh = RT.ORBBreak()._pd(frame(ts, high=high, low=low, close=close))
    return (np.asarray(lg.values), np.asarray(sh.values))


def names():
    """What the reference calls its outputs: the returned Series' names and the transforms' output_name."""
    f = frame(H.stamps(40, 1)[0], close=np.ones(40), ret1=np.ones(40), high=np.ones(40), low=np.ones(40))
    out = {}
    for key, t in (("BarDuration()", RT.BarDuration()), ("BarDuration(3)", RT.BarDuration(3)),
                   ("BarDuration(2, 'vwap')", RT.BarDuration(2, "vwap")), ("BarDurationEWMA()", RT.BarDurationEWMA()),
                   ("BarDurationEWMA(7)", RT.BarDurationEWMA(7)), ("BarRate(6min)", RT.BarRate(pd.Timedelta(minutes=6))),
                   ("BarRate(90s)", RT.BarRate(pd.Timedelta(seconds=90))), ("BarRate(30min)", RT.BarRate(pd.Timedelta(minutes=30))),
                   ("DirRunLen()", RT.DirRunLen()), ("DirRunLen('close')", RT.DirRunLen("close")), ("ORBBreak()", RT.ORBBreak())):
        g = f.rename(columns={"close": "vwap"}) if "vwap" in key else f
        res = t(g, backend="pd")
        series = [s.name for s in res] if isinstance(res, tuple) else res.name
        out[key] = {"series": series, "output_name": t.output_name, "requires": list(t.requires), "produces": list(t.produces)}
    return out


def main():
    geo = clock.geometry()
    out, manifest, worst = {}, {}, 0.0
    for name, c in H.cases(geo).items():
        fn, args = c["fn"], c["args"]
        inputs = H.generate(c["source"])
        entry = {"fn": fn, "args": args, "source": c["source"], "n": int(len(inputs[0])), "input_sha256": H.sha256(*inputs),
                 "reference": bool(c["reference"])}
        own = H.call(fn, inputs, args)
        if c["reference"]:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = reference(fn, [np.array(a) for a in inputs], args)
            if len(ref) != len(own):
                raise SystemExit(f"{name}: the reference gives {len(ref)} outputs")
            for r, o in zip(ref, own):
                if H.EXACT[fn]:
                    if not H.same_bits(np.asarray(r, o.dtype) if r.dtype.kind == o.dtype.kind else r, o):
                        bad = np.flatnonzero(~((r == o) | ((r != r) & (o != o))))[:5] if r.shape == o.shape else "shape"
                        raise SystemExit(f"{name}: the reference and the restatement disagree at {bad} -- case refused")
                else:
                    dev = H.dew_deviation(o, r)
                    if dev is None or dev > H.DEW_BOUND:
                        raise SystemExit(f"{name}: the reference and the restatement disagree ({dev}) -- case refused")
                    entry["ref_dev"] = dev
                    worst = max(worst, dev)
            keep = ref
        else:
            try:
                reference(fn, [np.array(a) for a in inputs], args)
                raise SystemExit(f"{name}: the reference runs this case after all -- mark it reference: True")
            except (OverflowError, IndexError) as e:
                entry["reference_raises"] = f"{type(e).__name__}: {e}"
            keep = own
        for k, a in enumerate(keep):
            out[f"{name}.out{k}"] = np.asarray(a, own[k].dtype)
        manifest[name] = entry
        print(name, {a: b for a, b in entry.items() if a not in ("input_sha256", "source")})
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "clock.npz"), **out)
    note = ("DirRunLen.numba_core runs under the interpreter in the generator: NumPy 2 raises OverflowError on the int8 store of a run "
            "of 128 and more, so the untouched reference pins runs up to 127; cases with reference false hold the restatement's "
            "output (the low 8 bits, as the compiled store).")
    with open(os.path.join(gold, "clock.json"), "w") as fh:
        json.dump({"geometry": geo, "dew_bound": H.DEW_BOUND, "dew_ref_dev": worst, "dir_run_len_note": note, "names": names(),
                   "pandas": pd.__version__, "numpy": np.__version__, "cases": manifest}, fh, indent=1, sort_keys=True)
    print(len(manifest), "cases,", os.path.getsize(os.path.join(gold, "clock.npz")), "bytes; dew_ref_dev", worst)


if __name__ == "__main__":
    main()
