#!/usr/bin/env python3
"""Times the three label calls on a resident synthetic tape with the context's HIP-event timer and prints one JSON line.

Tape: DeviceTrades.synth(N) (default 1e9 ticks).  Events: the closes of the CUSUM configuration of tools/cusumbench.py (EWM sigma of
5 s log returns, half-life 60 s, floor 1e-5, multiplier 2), thinned to at most MAX_EVENTS and to those with a full 10-minute window.
Targets: that sigma at the event, times TARGET_MULT (a 5 s volatility scaled towards the move of a 10-minute window).  Symmetric
barriers, min_close_time 1 s; a 10-minute vertical barrier (the direct walk; also forced through the block tables) and a disabled
one (the block tables; the direct walk would follow a path that never touches to the end of the tape with one wave).  Per call: one untimed run, then REPS timed ones (median and min); ticks walked and blocks opened from
fmk_diag_label_last; bytes by construction: 8 B per walked tick, 8 B/tick read + 16 B per 1024 ticks written for the tables,
10 B/tick for the weights pass, 4 B/tick x 3 + 2 for the concurrency scan.
usage: labelbench.py [N] [MAX_EVENTS] [TARGET_MULT]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
MAX_EVENTS = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
TARGET_MULT = float(sys.argv[3]) if len(sys.argv) > 3 else 10.0
REPS = 3
PEAK = 8e12


def timed(ctx, fn):
    fn()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        out = fn()
        ms.append(ctx.timer_stop())
    return out, float(np.median(ms)), float(min(ms))


def diag(ctx):
    out = (C.c_int64 * 5)()
    _ffi.check(_ffi.lib().fmk_diag_label_last(ctx.handle, out), ctx.handle)
    return dict(zip(("schedule", "events", "skipped", "opened", "walked"), [int(x) for x in out]))


def main():
    ctx = _ffi.default_context()
    t = engine.DeviceTrades.synth(N, seed=42, ctx=ctx)
    ret = t.lagged_returns(5.0, True)
    sig = t.ewmst(ret, 60.0)
    del ret
    m = c_i64()
    d_all = DeviceArray(ctx, N, np.int64)
    ctx.call("fmk_cusum_bar_indexer_dev", t.ts.p, t.price.p, sig.p, c_i64(N), c_f64(1e-5), c_f64(2.0), d_all.p, c_i64(N),
             C.byref(m), None)
    closes = d_all.view(1, m.value - 1).to_host()
    d_all.free()
    closes = closes[::max(1, -(-len(closes) // MAX_EVENTS))]
    ts_ev = t.gather_ts(DeviceArray.from_host(ctx, closes)).to_host()
    ev = closes[ts_ev + 600 * 10 ** 9 <= t.first_last_ts()[1]]
    d_ev = DeviceArray.from_host(ctx, ev)
    d_tg = DeviceArray(ctx, len(ev), np.float64)
    ctx.call("fmk_gather_i64_dev", sig.p, c_i64(N), d_ev.p, c_i64(len(ev)), d_tg.p)       # an 8-byte gather of sigma
    tg = d_tg.to_host() * TARGET_MULT
    d_tg = DeviceArray.from_host(ctx, tg)
    del sig
    res = {"tool": "labelbench", "ticks": N, "events": int(len(ev)), "cusum_closes": int(m.value - 1), "target_mult": TARGET_MULT,
           "target_median": float(np.median(tg)), "reps": REPS, "calls": {}}
    keep = {}
    for name, vb, force in (("tb_10min_default", 600.0, None), ("tb_10min_forced_tables", 600.0, "long"),
                            ("tb_inf_default", float("inf"), None)):
        os.environ.pop("FMK_LABEL_SCHEDULE", None)
        if force:
            os.environ["FMK_LABEL_SCHEDULE"] = force
        out, med, best = timed(ctx, lambda: t.triple_barrier(d_ev, d_tg, (1.0, 1.0), vb, 1.0))
        os.environ.pop("FMK_LABEL_SCHEDULE", None)
        d = diag(ctx)
        table_bytes = (8 * N + 16 * (N // 1024 + N // 65536)) if d["schedule"] else 0
        walk_bytes = 8 * d["walked"]
        touch = out[1].to_host()
        res["calls"][name] = {"ms_median": med, "ms_min": best, **d, "bytes_walk": walk_bytes, "bytes_tables": table_bytes,
                              "frac_of_8TBs": (walk_bytes + table_bytes) / (best * 1e-3) / PEAK,
                              "mean_path_ticks": float(np.mean(touch - ev)), "max_path_ticks": int(np.max(touch - ev)),
                              "vertical_touches": int((out[3].to_host() != 1.0).sum())}
        keep[name] = out[1]
    for name, tb in (("10min", "tb_10min_default"), ("inf", "tb_inf_default")):
        d_tc = keep[tb]
        conc, med, best = timed(ctx, lambda: t.label_concurrency(d_ev, d_tc))
        b = 14 * N
        res["calls"]["concurrency_" + name] = {"ms_median": med, "ms_min": best, "bytes": b, "frac_of_8TBs": b / (best * 1e-3) / PEAK}
        _, med, best = timed(ctx, lambda: t.label_weights(d_ev, d_tc, conc))
        length = (d_tc.to_host() - ev + 1).astype(np.float64)
        b = 10 * N + int(np.sum(np.minimum(length, 2048.0) * 10 + length / 1024 * 16))
        res["calls"]["weights_" + name] = {"ms_median": med, "ms_min": best, "bytes": b, "frac_of_8TBs": b / (best * 1e-3) / PEAK,
                                           "mean_event_ticks": float(length.mean())}
        del conc
    print(json.dumps(res))


if __name__ == "__main__":
    main()
