#!/usr/bin/env python3
"""Times the rolling-window moments (fmk_zscore_dev, fmk_rolling_variance_dev, fmk_variance_ratio_1_4_dev: csrc/fmk_rolling.hip) on
a resident synthetic price column with the context's HIP-event timer and prints one JSON line.

Workloads: (n = 1e7, window 1000) and (n = 1e8, window 50).  Per workload and function one untimed call, then REPS timed ones (the
minimum counts).  "window_elements" is what the call walks: outputs x window, twice for the z-score (the sum, then the squared
deviations) and for the ratio (the variances of the 1-step and of the 4-step returns) -> window elements per second, the figure to
hold against the pair rate of tools/breakbench.py.
usage: rollbench.py [SCALE]        SCALE < 1 shrinks every n (a smoke run)"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_i64  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
REPS = 3


def main():
    ctx = _ffi.default_context()
    res = {"tool": "rollbench", "reps": REPS, "calls": {}}

    def run(n, window):
        t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
        out = DeviceArray(ctx, n, np.float64)
        head = (t.price.p, c_i64(n), c_i64(window))
        calls = {
            "zscore": (2, lambda: ctx.call("fmk_zscore_dev", *head, c_i64(0), out.p)),
            "rolling_variance": (1, lambda: ctx.call("fmk_rolling_variance_dev", *head, c_i64(1), c_i64(1), out.p)),
            "variance_ratio_1_4": (2, lambda: ctx.call("fmk_variance_ratio_1_4_dev", *head, c_i64(0), C.c_int(1), out.p)),
        }
        for name, (walks, call) in calls.items():
            call()
            ms = []
            for _ in range(REPS):
                ctx.timer_start()
                call()
                ms.append(ctx.timer_stop())
            best = min(ms)
            elements = walks * (n - window + 1) * window
            res["calls"][f"{name}_w{window}"] = {"n": n, "window": window, "ms_min": best, "ms": ms, "window_elements": elements,
                                                 "window_elements_per_s": elements / (best * 1e-3),
                                                 "checksum": float(np.nansum(out.view(0, min(n, 100_000)).to_host()))}

    run(max(2000, int(1e7 * SCALE)), 1000)
    run(max(2000, int(1e8 * SCALE)), 50)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
