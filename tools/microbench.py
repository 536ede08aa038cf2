#!/usr/bin/env python3
"""Per-call timings of DeviceTrades.bar_microstructure on N resident ticks at ~250-tick and ~4 000-tick bars, with bar_directional --
which reads the same three columns -- on the same tape and closes as the yardstick, and two figures that say what bounds the kernel:
the same call on a tape whose price never moves (p / p_prev == 1 takes the logarithm's shortcut, everything else runs), and the
streaming read of the 13 B per tick the call needs (fmk_diag_read_bandwidth).  Device-event times around calls that end in a wait.
usage: microbench.py [N] [--out profiles/microbench.json] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from finmlkit_amd import _ffi, engine
from finmlkit_amd._ffi import DeviceArray

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=float, default=1e8)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "microbench.json"))
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
n = int(args.n)
ctx = _ffi.default_context()
t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
flat = engine.DeviceTrades(ctx, t.ts, DeviceArray.from_host(ctx, np.full(n, 100.0)), t.amount, t.side)
flat.amount_is_f64 = t.amount_is_f64


def timed(fn):
    for _ in range(3):
        fn()
    ctx.sync()
    ms = []
    for _ in range(args.reps):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def read_ms(nbytes):
    buf = DeviceArray(ctx, nbytes // 8, np.int64)
    buf.zero()
    ms, best = C.c_double(), []
    for _ in range(6):
        ctx.call("fmk_diag_read_bandwidth", buf.p, C.c_size_t(nbytes), C.c_int(1), C.c_int(16), C.byref(ms))
        best.append(ms.value)
    return float(np.median(best[1:]))


res = {"n_ticks": n, "amounts": "float64" if t.amount_is_f64 else "float32", "bytes_per_tick": 8 + (8 if t.amount_is_f64 else 4) + 1,
       "reps": args.reps, "stream_read_of_the_same_bytes_ms": read_ms(n * (8 + (8 if t.amount_is_f64 else 4) + 1) // 8 * 8), "bars": {}}
for ticks in (250, 4000):
    ci = t.tick_bar_index(ticks)
    r = {"n_bars": ci.n - 1,
         "bar_microstructure": timed(lambda: t.bar_microstructure(ci)),
         "bar_microstructure_flat_price": timed(lambda: flat.bar_microstructure(ci)),
         "bar_directional": timed(lambda: t.bar_directional(ci))}
    r["ratio_to_bar_directional"] = r["bar_microstructure"]["median_ms"] / r["bar_directional"]["median_ms"]
    r["gb_per_s"] = res["bytes_per_tick"] * n / r["bar_microstructure"]["median_ms"] / 1e6
    res["bars"][str(ticks)] = r
    print(ticks, json.dumps(r), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
