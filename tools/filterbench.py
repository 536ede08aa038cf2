#!/usr/bin/env python3
"""Times the symmetric CUSUM event filter (fmk_cusum_filter_dev) on a resident synthetic tape with the context's HIP-event timer and
prints one JSON line.

Tape: DeviceTrades.synth(N) (default 1e9 ticks); the series is its price column.  Workloads:
  const_dense : one constant threshold, DENSE (default 1.5e-5: an event every few hundred ticks)             8 B/tick
  per_sigma   : one threshold per element, the EWM sigma (half-life 60 s) of 5 s log returns, as tools/labelbench.py   16 B/tick
  const_sparse: one constant threshold, SPARSE (default 2.2e-4: an event about every 1e5 ticks) -- the regime the chain tier of
                the bar indexer serves and the filter does not have; skipped with SPARSE = 0
Yardstick, same tape, same process: fmk_cusum_bar_indexer_dev with that sigma, floor 1e-5, multiplier 2 (24 B/tick).
Per workload: one untimed call, then REPS timed ones (min and median); the form that answered, the launches after pass A and the
chunks pending after the first fix-up from fmk_diag_cusum_filter_last.  Bytes by construction: the input columns once per pass over
the chunks that are walked (pass A reads CS1_W / CS1_L more for the warm-up), 2 B per event staged and 8 B per event written.
usage: filterbench.py [N] [DENSE] [SPARSE]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
DENSE = float(sys.argv[2]) if len(sys.argv) > 2 else 1.5e-5
SPARSE = float(sys.argv[3]) if len(sys.argv) > 3 else 2.2e-4
REPS = 3
PEAK = 8e12
L, W = 4096, 512


def timed(ctx, fn):
    fn()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return float(np.median(ms)), float(min(ms))


def diag():
    v = [c_i64() for _ in range(4)]
    _ffi.lib().fmk_diag_cusum_filter_last(*[C.byref(x) for x in v])
    return dict(zip(("form", "launches", "pending_first", "chunks"), (int(x.value) for x in v)))


def main():
    ctx = _ffi.default_context()
    t = engine.DeviceTrades.synth(N, seed=42, ctx=ctx)
    ret = t.lagged_returns(5.0, True)
    sig = t.ewmst(ret, 60.0)
    del ret
    res = {"tool": "filterbench", "ticks": N, "reps": REPS, "calls": {}}
    out = DeviceArray(ctx, max(1024, N // 16), np.int64)
    m, rounds = c_i64(), c_i64()

    def run(name, thr, n_thr, per_tick):
        def call():
            ctx.call("fmk_cusum_filter_dev", t.price.p, c_i64(N), thr.p, c_i64(n_thr), out.p, c_i64(out.n), C.byref(m), C.byref(rounds))
        med, best = timed(ctx, call)
        d = diag()
        b = per_tick * N * (L + W) // L + 10 * m.value                  # pass A; the launches after it re-read what they walk
        res["calls"][name] = {"ms_median": med, "ms_min": best, "events": int(m.value), "rounds": int(rounds.value), **d,
                              "form_name": "rewalk" if d["form"] else "onepass", "bytes_pass_a": b,
                              "frac_of_8TBs_pass_a": b / (best * 1e-3) / PEAK,
                              "checksum": int(out.view(0, min(m.value, out.n)).to_host().sum())}

    run("const_dense", DeviceArray.from_host(ctx, np.array([DENSE])), 1, 8)
    run("per_sigma", sig, N, 16)
    if SPARSE > 0:
        run("const_sparse", DeviceArray.from_host(ctx, np.array([SPARSE])), 1, 8)
    del out
    # the yardstick: the bar indexer on the same tape (it forward-fills sigma in place: last)
    bars = DeviceArray(ctx, N, np.int64)

    def bar_call():
        ctx.call("fmk_cusum_bar_indexer_dev", t.ts.p, t.price.p, sig.p, c_i64(N), c_f64(1e-5), c_f64(2.0), bars.p, c_i64(N),
                 C.byref(m), C.byref(rounds))
    med, best = timed(ctx, bar_call)
    u, fl, pf, ch = c_i64(), c_i64(), c_i64(), c_i64()
    _ffi.lib().fmk_diag_cusum_onepass(C.byref(u), C.byref(fl), C.byref(pf), C.byref(ch))
    res["calls"]["bar_indexer_floor_1e-5"] = {"ms_median": med, "ms_min": best, "closes": int(m.value), "rounds": int(rounds.value),
                                              "onepass_used": int(u.value), "launches": int(fl.value), "pending_first": int(pf.value),
                                              "chunks": int(ch.value), "bytes_pass_a": 24 * N * (L + W) // L}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
