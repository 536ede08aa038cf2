#!/usr/bin/env python3
"""Times the imbalance / run bar indexers (fmk_flow_bar_indexer_dev) on a resident synthetic tape with the context's HIP-event timer
and prints one JSON line.

Tape: DeviceTrades.synth(N) (default 1e8 ticks): sides +-1 with equal odds, lots uniform on (1 .. 4096) / 1024 (mean 2, mean square
16 / 3).  Workloads: both rules, sizes "tick" and "volume", two thresholds each, chosen from those moments for mean bars of about 250
and about 4 000 ticks (imbalance: thr^2 / E[x^2]; run: thr / (E[size] / 2)); the mean length that came out is reported.  Yardstick,
same tape, same process: volume_bar_index at thresholds of the same mean bar lengths (its code predates these indexers).
Per workload: one untimed call, then REPS timed ones (min and median), the rung that answered, the longest link and the table span.
bytes_min: what the four passes of the tables rung move by construction -- side 1 B and amount 0 / 4 B read, prefix 8 B (run: 16 B)
written and read once, link 4 B written and read once, level-0 row 8 B written per tick; blocks a bar closes in are read again.
usage: flowbarbench.py [N]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
REPS = 3
WORKLOADS = (("imbalance", "tick", 16.0), ("imbalance", "tick", 63.0), ("imbalance", "volume", 36.5), ("imbalance", "volume", 146.0),
             ("run", "tick", 125.0), ("run", "tick", 2000.0), ("run", "volume", 250.0), ("run", "volume", 4000.0))
YARDSTICK = (500.0, 8000.0)


def timed(ctx, fn):
    out = fn()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        out = fn()
        ms.append(ctx.timer_stop())
    return out, float(np.median(ms)), float(min(ms))


def main():
    ctx = _ffi.default_context()
    t = engine.DeviceTrades.synth(N, seed=42, ctx=ctx)
    res = {"tool": "flowbarbench", "ticks": N, "reps": REPS, "calls": {}}
    for rule, kind, thr in WORKLOADS:
        fn = (t.imbalance_bar_index if rule == "imbalance" else t.run_bar_index)
        out, med, best = timed(ctx, lambda: fn(thr, kind=kind))
        d = _ffi.flow_bars_last()
        p = 8 if rule == "imbalance" else 16
        b = 1 + (4 if kind == "volume" else 0) + 2 * p + 4 + 4 + 8
        res["calls"][f"{rule}_{kind}_{thr:g}"] = {
            "ms_median": med, "ms_min": best, "closes": out.n - 1, "mean_bar": N / max(out.n - 1, 1), **d,
            "bytes_min_per_tick": b, "gbps_at_bytes_min": b * N / (best * 1e-3) / 1e9,
            "checksum": int(out.to_host().sum())}
        del out
    for thr in YARDSTICK:
        out, med, best = timed(ctx, lambda: t.volume_bar_index(thr))
        res["calls"][f"volume_bars_{thr:g}"] = {"ms_median": med, "ms_min": best, "closes": out.n - 1, "mean_bar": N / max(out.n - 1, 1),
                                                "checksum": int(out.to_host().sum())}
        del out
    for k, v in res["calls"].items():
        if not k.startswith("volume_bars"):
            y = res["calls"]["volume_bars_500" if v["mean_bar"] < 1000 else "volume_bars_8000"]
            v["ratio_to_volume_bars"] = v["ms_min"] / y["ms_min"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
