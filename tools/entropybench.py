#!/usr/bin/env python3
"""Times the rolling approximate entropy (fmk_approximate_entropy_dev: csrc/fmk_entropy.hip) against the z-score (fmk_zscore_dev:
csrc/fmk_rolling.hip), the existing two-walk kernel, in one run: both on the one-step log returns of a resident synthetic price
column of n = 1e7 elements, m = 2, tolerance 0.2, at the windows 24 and 64 (the row-mask path) and 256 (the plain path).  Per
launch one untimed call, then REPS timed ones with the context's HIP-event timer; the median counts.  Prints one JSON line (the
times and the ratios entropy / z-score) and, with an output path, writes it there.
usage: entropybench.py [SCALE [OUT.json]]        SCALE < 1 shrinks n (a smoke run)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else None
REPS = 7
WINDOWS = (24, 64, 256)
M, TOLERANCE = 2, 0.2


def main():
    ctx = _ffi.default_context()
    n = max(4000, int(1e7 * SCALE))
    t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
    price = t.price.to_host()
    ret = np.zeros(n)
    ret[1:] = np.diff(np.log(price))
    returns = DeviceArray.from_host(ctx, ret)
    out = DeviceArray(ctx, n, np.float64)
    res = {"tool": "entropybench", "n": n, "reps": REPS, "m": M, "tolerance": TOLERANCE, "calls": {}, "ratio_over_zscore": {}}
    for window in WINDOWS:
        calls = {"apen": lambda: ctx.call("fmk_approximate_entropy_dev", returns.p, c_i64(n), c_i64(window), c_i64(M), c_f64(TOLERANCE),
                                          out.p),
                 "zscore": lambda: ctx.call("fmk_zscore_dev", returns.p, c_i64(n), c_i64(window), c_i64(0), out.p)}
        for name, call in calls.items():
            call()
            ms = []
            for _ in range(REPS):
                ctx.timer_start()
                call()
                ms.append(ctx.timer_stop())
            head = out.view(0, min(n, 100_000)).to_host()
            res["calls"][f"{name}_w{window}"] = {"window": window, "ms_median": statistics.median(ms), "ms": ms,
                                                 "finite_in_head": int(np.isfinite(head).sum()),
                                                 "checksum": float(np.nansum(head))}
        res["ratio_over_zscore"][f"apen_w{window}"] = (res["calls"][f"apen_w{window}"]["ms_median"] /
                                                       res["calls"][f"zscore_w{window}"]["ms_median"])
    line = json.dumps(res)
    print(line)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
