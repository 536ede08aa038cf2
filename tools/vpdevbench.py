#!/usr/bin/env python3
"""Timings of the developing volume profile (fmk_volume_profile_developing_dev) on the 1-minute bars / footprints of N resident ticks
of the synthetic tape (the footprints of tools/nextbench.py: price tick 0.01): 1440-bar sessions and ONE range over everything, without
bucketing and with 27 bins (and once with va_pct 0, where no value-area walk takes a step), and -- beside them, from the same run, on the same footprints -- the rolling profile with 30-bar windows.
Device events round every call (the call ends in a read-back, so the device is idle when the second event is recorded); the best and
the median of `reps` repetitions after one warm-up call per shape.  Nothing is asserted about any time.
usage: vpdevbench.py [N] [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from finmlkit_amd import _ffi, engine
from finmlkit_amd._ffi import DeviceArray, c_i64, c_f64, ptr

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ctx = _ffi.default_context()
t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
clock, ci = t.time_bar_index(60.0)
nb = ci.n - 1
o = t.bar_ohlcv(ci, want_median=True)
off, flat, bar, bad = t.bar_footprints(ci, o["low"], o["high"], 0.01)
bts = t.gather_ts(ci).to_host()[1:]
n_lev = int(flat["price_levels"].n)
lo, hi = o["low"].to_host(), o["high"].to_host()
print(f"{n} ticks -> {nb} one-minute bars, {n_lev} footprint rows, price tick 0.01; {reps} repetitions", flush=True)


def timed(fn):
    fn(); ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timer_start(); fn(); ms.append(ctx.timer_stop())
    return min(ms), float(np.median(ms))


def developing(starts, ends, bins, va=68.34):
    rs, re_ = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(ends, np.int64)
    oo = np.concatenate([[0], np.cumsum(re_ - rs)[:-1]]).astype(np.int64)
    outs = [DeviceArray(ctx, int((re_ - rs).sum()), np.int32) for _ in range(3)]
    return lambda: ctx.call("fmk_volume_profile_developing_dev", o["high"].p, o["low"].p, off.p, flat["price_levels"].p, flat["buy_volumes"].p,
                            flat["sell_volumes"].p, c_i64(nb), ptr(rs), ptr(re_), ptr(oo), c_i64(len(rs)), c_i64(bins), c_f64(0.01),
                            c_f64(va), c_i64(0), *[x.p for x in outs]), (rs, re_, oo, outs)


def widest(starts, ends):
    return max(int(round(hi[s:e].max() / 0.01)) - int(round(lo[s:e].min() / 0.01)) + 1 for s, e in zip(starts, ends))


edges = np.arange(0, nb + 1440, 1440).clip(max=nb)
edges = np.unique(edges)
shapes = (("1440-bar sessions", edges[:-1], edges[1:]), ("one range", np.array([0]), np.array([nb])))
for what, s, e in shapes:
    for bins in (-1, 27):
        fn, keep = developing(s, e, bins)
        b, m = timed(fn)
        print(f"volume_profile_developing  {what:18s} {len(s):5d} ranges, widest {widest(s, e):7d} levels, n_bins {bins:3d}: best {b:9.2f} ms, "
              f"median {m:9.2f} ms  ({nb / b / 1e3:8.1f} bars / us)", flush=True)

# the same sessions with va_pct 0: the value-area walk of every bar ends at its first test, everything else is as above
fn, keep = developing(edges[:-1], edges[1:], -1, va=0.0)
b, m = timed(fn)
print(f"volume_profile_developing  1440-bar sessions, va_pct 0 (no walk steps)              n_bins  -1: best {b:9.2f} ms, median {m:9.2f} ms", flush=True)

first_bar = int(np.searchsorted(bts, bts[0] + 30 * 60 * 10**9))
outs = [DeviceArray(ctx, nb, np.int32) for _ in range(3)] + [DeviceArray(ctx, nb, np.float32)]
ts_bars = DeviceArray.from_host(ctx, np.ascontiguousarray(bts))
for bins in (-1, 27):
    b, m = timed(lambda: ctx.call("fmk_volume_profile_rolling_dev", ts_bars.p, o["high"].p, o["low"].p, off.p, flat["price_levels"].p,
                                  flat["buy_volumes"].p, flat["sell_volumes"].p, c_i64(nb), c_i64(first_bar), c_i64(30 * 60 * 10**9),
                                  c_i64(bins), c_f64(0.01), c_f64(68.34), *[x.p for x in outs]))
    print(f"volume_profile_rolling     30-bar windows                                            n_bins {bins:3d}: best {b:9.2f} ms, "
          f"median {m:9.2f} ms", flush=True)
