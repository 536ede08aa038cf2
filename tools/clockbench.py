#!/usr/bin/env python3
"""Times the five `_dev` entries of csrc/fmk_clock.hip -- fmk_bar_duration_dev, fmk_bar_duration_ewma_dev, fmk_bar_rate_dev (a
window whose slices fit the LDS stage and one whose slices do not), fmk_dir_run_len_dev, fmk_orb_break_dev -- on a synthetic resident
tape (DeviceTrades.synth, n = 1e8 rows, mean gap 50 ms): the clock features on the tape's own stamps, dir_run_len on the one-step
pct_change of the price column, orb_break with the price column as high, low and close.  Per entry WARM untimed calls, then REPS
samples of INNER calls each with the context's HIP-event timer; the median sample / INNER counts.  `bytes_per_row` is the account of
DESIGN.md section 7i (what the launches of one call read and write per row when nothing is reused between launches), kept here with
the benchmark; `gb_per_s` is that account over the measured time, not a counter reading.  Prints one JSON line and, with an output
path, writes it there.
usage: clockbench.py [SCALE [OUT.json]]        SCALE < 1 shrinks n (a smoke run)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64  # noqa: E402
from finmlkit_amd.feature.core import clock  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else None
WARM, REPS, INNER = 2, 7, 5
HEAD = 1_000_000                     # rows the checksum covers: the synthetic tape opens its first whole day after some 128 000
# ts read by the two passes of a scan counts twice; bar_duration's lagged stamp and bar_rate's look-back are reuse inside a launch
BYTES_PER_ROW = {"bar_duration": 8 + 8, "bar_duration_ewma": 2 * 8 + 8, "bar_rate_5s": 8 + 8, "bar_rate_1800s": 8 + 8,
                 "dir_run_len": 2 * 8 + 1, "orb_break": 2 * 8 + 8 + 2}


def main():
    ctx = _ffi.default_context()
    n = max(10_000, int(1e8 * SCALE))
    t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
    ret = t.pct_change(t.price, 1)
    f64 = DeviceArray(ctx, n, np.float64)
    i8 = DeviceArray(ctx, n, np.int8)
    u8 = (DeviceArray(ctx, n, np.uint8), DeviceArray(ctx, n, np.uint8))
    calls = {
        "bar_duration": (lambda: ctx.call("fmk_bar_duration_dev", t.ts.p, c_i64(n), c_i64(1), f64.p), f64),
        "bar_duration_ewma": (lambda: ctx.call("fmk_bar_duration_ewma_dev", t.ts.p, c_i64(n), c_f64(20.0), f64.p), f64),
        "bar_rate_5s": (lambda: ctx.call("fmk_bar_rate_dev", t.ts.p, c_i64(n), c_f64(5.0), c_i64(clock.window_ns(5.0)), f64.p), f64),
        "bar_rate_1800s": (lambda: ctx.call("fmk_bar_rate_dev", t.ts.p, c_i64(n), c_f64(1800.0), c_i64(clock.window_ns(1800.0)), f64.p),
                           f64),
        "dir_run_len": (lambda: ctx.call("fmk_dir_run_len_dev", ret.p, c_i64(n), i8.p), i8),
        "orb_break": (lambda: ctx.call("fmk_orb_break_dev", t.ts.p, t.price.p, t.price.p, t.price.p, c_i64(n), u8[0].p, u8[1].p), u8),
    }
    res = {"tool": "clockbench", "n": n, "warm": WARM, "reps": REPS, "inner": INNER, "geometry": clock.geometry(), "calls": {}}
    for name, (call, out) in calls.items():
        for _ in range(WARM):
            call()
        ms = []
        for _ in range(REPS):
            ctx.timer_start()
            for _ in range(INNER):
                call()
            ms.append(ctx.timer_stop() / INNER)
        med = statistics.median(ms)
        outs = out if isinstance(out, tuple) else (out,)                 # orb_break: both series
        head = np.concatenate([o.view(0, min(n, HEAD)).to_host().astype(np.float64) for o in outs])
        res["calls"][name] = {"ms_per_call": med, "ms": ms, "bytes_per_row": BYTES_PER_ROW[name],
                              "gb_per_s": BYTES_PER_ROW[name] * n / (med * 1e-3) / 1e9,
                              "finite_in_head": int(np.isfinite(head).sum()), "checksum": float(np.nansum(head))}
    line = json.dumps(res)
    print(line)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
