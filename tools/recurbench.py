#!/usr/bin/env python3
"""Times the recursive indicators (fmk_ewma_dev, fmk_rsi_wilder_dev, fmk_true_range_dev, fmk_atr_dev in both modes, fmk_adx_dev:
csrc/fmk_recur.hip) and the running-sum indicators (fmk_bollinger_percent_b_dev, fmk_vwap_distance_dev, fmk_flow_acceleration_dev,
fmk_vpin_dev, fmk_parkinson_range_dev: csrc/fmk_runsum.hip) on resident synthetic columns with the context's HIP-event timer,
`fmk_ewms_dev` (the scan of csrc/fmk_ticklevel.hip) at the same sizes beside them as the yardstick, and prints one JSON line.

Workloads: n = 1e7 and n = 1e8, window 14.  Every timed step (one function at one size: an untimed call, then REPS timed ones, the
minimum counts) runs in a child process of its own under a time limit, so that a step that hangs ends alone; after a step that
fails nothing more is started.  "bytes_per_element" is what the algorithm has to move: a scan reads its input series twice and writes
once (ewma 2 x 8 + 8, rsi the same, atr and adx 2 x 24 + 8, adx also the dx series: written once, read twice, + 24), true_range and
the SMA mode read three series and write one; bollinger 2 x 8 + 8 (its lagged read is the same series), vwap_distance 2 x 16 + 8,
flow_acceleration 2 x 8 + 12 for the prefix sum and the 4-byte count of non-zero bars, which are read again, + 12 + 8, vpin 2 x 16 + 40 for
three prefix sums and two series of counts, read again, + 40 + 4, parkinson_range 16 + 8) -> bytes per second, to hold against the HBM rate.
usage: recurbench.py [SCALE]        SCALE < 1 shrinks every n (a smoke run)
       recurbench.py --step NAME N  (internal) one step, prints its JSON"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
WINDOW = 14
STEP_LIMIT_S = 120
# name -> (entry, input series, bytes per element)
STEPS = {
    "ewms": ("fmk_ewms_dev", 1, 24),
    "ewma": ("fmk_ewma_dev", 1, 24),
    "rsi_wilder": ("fmk_rsi_wilder_dev", 1, 24),
    "true_range": ("fmk_true_range_dev", 3, 32),
    "atr_sma": ("fmk_atr_dev", 3, 32),
    "atr_ema": ("fmk_atr_dev", 3, 56),
    "adx": ("fmk_adx_dev", 3, 80),
    "bollinger_percent_b": ("fmk_bollinger_percent_b_dev", 1, 24),
    "vwap_distance": ("fmk_vwap_distance_dev", 2, 40),
    "flow_acceleration": ("fmk_flow_acceleration_dev", 1, 48),
    "vpin": ("fmk_vpin_dev", 2, 116),
    "parkinson_range": ("fmk_parkinson_range_dev", 2, 24),
}


def step(name, n):
    import numpy as np

    from finmlkit_amd import _ffi, engine
    from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64
    ctx = _ffi.default_context()
    entry, nin, bpe = STEPS[name]
    t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
    close = t.price
    # low and high around the price column: any finite series serve, the kernels' work does not depend on the values
    host = close.view(0, min(n, 1 << 20)).to_host()
    reps = -(-n // len(host))
    low = DeviceArray.from_host(ctx, np.tile(host - 0.25, reps)[:n])
    high = DeviceArray.from_host(ctx, np.tile(host + 0.25, reps)[:n])
    out = DeviceArray(ctx, n, np.float64)
    # (two series: high and low stand for close and volume, for the buy and the sell volume, and for themselves)
    ins = {1: (close.p,), 2: (high.p, low.p), 3: (high.p, low.p, close.p)}[nin]
    tail = {"ewms": (c_i64(WINDOW),), "ewma": (c_f64(float(WINDOW)),), "rsi_wilder": (c_i64(WINDOW),), "true_range": (),
            "atr_sma": (c_i64(WINDOW), C.c_int(0), C.c_int(0)), "atr_ema": (c_i64(WINDOW), C.c_int(1), C.c_int(0)),
            "adx": (c_i64(WINDOW),), "bollinger_percent_b": (c_i64(WINDOW), c_f64(2.0)), "vwap_distance": (c_i64(WINDOW), C.c_int(1)),
            "flow_acceleration": (c_i64(WINDOW), c_i64(5)), "vpin": (c_i64(WINDOW),), "parkinson_range": ()}[name]

    def call():
        ctx.call(entry, *ins, c_i64(n), *tail, out.p)

    call()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        call()
        ms.append(ctx.timer_stop())
    best = min(ms)
    head = out.view(0, min(n, 50_000)).to_host()                     # (vpin writes float32 into the front of the buffer)
    print(json.dumps({"n": n, "window": WINDOW, "ms_min": best, "ms": ms, "bytes_per_element": bpe,
                      "bytes_per_s": bpe * n / (best * 1e-3), "ns_per_element": best * 1e6 / n,
                      "checksum": float(np.nansum(head.view(np.float32) if name == "vpin" else head))}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]))
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    res = {"tool": "recurbench", "reps": REPS, "window": WINDOW, "calls": {}}
    for n in (max(5000, int(1e7 * scale)), max(5000, int(1e8 * scale))):
        for name in STEPS:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(n)], capture_output=True, text=True,
                                   timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired:
                res["stopped"] = f"{name} n={n}: no result within {STEP_LIMIT_S} s"
                print(json.dumps(res))
                return 1
            if p.returncode != 0:
                res["stopped"] = f"{name} n={n}: exit status {p.returncode}: {p.stderr.strip()[-300:]}"
                print(json.dumps(res))
                return 1
            res["calls"][f"{name}_n{n}"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
