#!/usr/bin/env python3
"""Times the windowed order statistics (fmk_burst_ratio_dev, fmk_stoch_k_dev, fmk_roc_dev, fmk_pct_change_dev: csrc/fmk_order.hip)
on a resident synthetic price column with the context's HIP-event timer, `fmk_sma_dev` at the same shapes beside them as the
yardstick, and prints one JSON line.

Shapes: n = 1e7 with windows 50 and 1000, and with the first window of the rolling median's bisection path (3074).  Per shape and
entry one untimed call on a short series (the code object is loaded), then REPS timed calls (the minimum counts).
usage: orderbench.py [SCALE]        SCALE < 1 shrinks n (a smoke run)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_i64  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
SORT_WINDOW_MAX = 3073                 # csrc/fmk_order.hip: ORD_SORT_WINDOW_MAX
REPS = 3


def main():
    ctx = _ffi.default_context()
    n = max(8000, int(1e7 * SCALE))
    t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
    out = DeviceArray(ctx, n, np.float64)
    res = {"tool": "orderbench", "n": n, "reps": REPS, "ms": {}}
    x = t.price.p
    for window in (50, 1000, SORT_WINDOW_MAX + 1):
        calls = {
            "sma": lambda m: ctx.call("fmk_sma_dev", x, c_i64(m), c_i64(window), out.p),
            "burst_ratio": lambda m: ctx.call("fmk_burst_ratio_dev", x, c_i64(m), c_i64(window), out.p),
            "stoch_k": lambda m: ctx.call("fmk_stoch_k_dev", x, x, x, c_i64(m), c_i64(window), out.p),
            "roc": lambda m: ctx.call("fmk_roc_dev", x, c_i64(m), c_i64(window), out.p),
            "pct_change": lambda m: ctx.call("fmk_pct_change_dev", x, c_i64(m), c_i64(window), out.p),
        }
        for name, call in calls.items():
            call(min(n, window + 2000))
            ctx.sync()
            ms = []
            for _ in range(REPS):
                ctx.timer_start()
                call(n)
                ms.append(ctx.timer_stop())
            res["ms"][f"{name}_w{window}"] = min(ms)
            print(name, window, res["ms"][f"{name}_w{window}"], file=sys.stderr, flush=True)
    res["checksum"] = float(np.nansum(out.view(0, min(n, 100_000)).to_host()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
