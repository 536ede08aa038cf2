#!/usr/bin/env python3
"""Times the rolling price-volume correlation (fmk_price_volume_corr_dev: csrc/fmk_corr.hip) against the z-score
(fmk_zscore_dev: csrc/fmk_rolling.hip), the existing two-walk kernel, in one run: both on resident synthetic columns at
(n = 1e7, window 64) and (n = 1e7, window 1000).  Per launch one untimed call, then REPS timed ones with the context's HIP-event
timer; the median counts.  Prints one JSON line (the four times and the two ratios correlation / z-score) and, with an output
path, writes it there.
usage: corrbench.py [SCALE [OUT.json]]        SCALE < 1 shrinks n (a smoke run)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_i64  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else None
REPS = 7


def main():
    ctx = _ffi.default_context()
    n = max(4000, int(1e7 * SCALE))
    t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
    # volumes: the synthetic amounts (float32 on the device) as a resident float64 column
    volume = DeviceArray.from_host(ctx, t.amount.to_host().astype(np.float64))
    out = DeviceArray(ctx, n, np.float64)
    res = {"tool": "corrbench", "n": n, "reps": REPS, "calls": {}, "ratio_corr_over_zscore": {}}
    for window in (64, 1000):
        calls = {
            "price_volume_corr": lambda: ctx.call("fmk_price_volume_corr_dev", t.price.p, volume.p, c_i64(n), c_i64(window), out.p),
            "zscore": lambda: ctx.call("fmk_zscore_dev", t.price.p, c_i64(n), c_i64(window), c_i64(0), out.p),
        }
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
        res["ratio_corr_over_zscore"][f"w{window}"] = (res["calls"][f"price_volume_corr_w{window}"]["ms_median"] /
                                                       res["calls"][f"zscore_w{window}"]["ms_median"])
    line = json.dumps(res)
    print(line)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
