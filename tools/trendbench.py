#!/usr/bin/env python3
"""Times trend scanning (fmk_trend_scanning_dev, csrc/fmk_trend.hip) on a resident synthetic tape with the context's HIP-event timer,
prints one JSON line and writes it to profiles/trendbench.json.

Tape: DeviceTrades.synth(N) (default 1e8 ticks).  Events: the symmetric CUSUM filter's (DeviceTrades.cusum_filter at THRESHOLD,
default 1.5e-5: an event every few hundred ticks) on the price column, thinned to at most MAX_EVENTS (default 1e6) and to those
whose longest span fits.  Calls: min_len 5, step 1, max_len 256 and
4 096.  Every step (one max_len: an untimed call, then REPS timed ones, the minimum counts) runs in a child process of its own
under a time limit, so that a step that hangs ends alone; after a step that fails nothing more is started.  Per step: the spans
evaluated (events x (max_len - min_len + 1)) per second, the ticks walked (events x max_len) and the bytes that is by
construction, 8 B x max_len per event, against the time; no parent commit has a figure to compare with.
usage: trendbench.py [N] [MAX_EVENTS] [THRESHOLD]
       trendbench.py --step MAX_LEN N MAX_EVENTS THRESHOLD  (internal) one step, prints its JSON"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 3
MIN_LEN = 5
MAX_LENS = (256, 4096)
STEP_LIMIT_S = 180
PEAK = 8e12


def step(max_len, n, max_events, threshold):
    import numpy as np

    from finmlkit_amd import _ffi, engine
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
    ev = t.cusum_filter(threshold).to_host()
    found = len(ev)
    ev = ev[ev + max_len <= n]
    ev = ev[::max(1, -(-len(ev) // max_events))]
    d_ev = DeviceArray.from_host(ctx, ev)

    def call():
        return t.trend_scanning(d_ev, MIN_LEN, max_len, 1)

    call()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        out = call()
        ms.append(ctx.timer_stop())
    best = min(ms)
    labels, tval, touch = out[0].to_host(), out[1].to_host(), out[2].to_host()
    spans = len(ev) * (max_len - MIN_LEN + 1)
    walk_bytes = 8 * len(ev) * max_len
    print(json.dumps({"max_len": max_len, "min_len": MIN_LEN, "step": 1, "ticks": n, "events": int(len(ev)), "cusum_events": int(found),
                      "ms_min": best, "ms": ms, "spans": spans, "spans_per_s": spans / (best * 1e-3), "bytes_walk": walk_bytes,
                      "bytes_per_s": walk_bytes / (best * 1e-3), "frac_of_8TBs": walk_bytes / (best * 1e-3) / PEAK,
                      "n_skipped": int(out[4].to_host()[0]), "labels": {str(k): int((labels == k).sum()) for k in (-1, 0, 1)},
                      "infinite_t": int(np.isinf(tval).sum()), "mean_span": float(np.mean(touch - ev + 1)) if len(ev) else 0.0}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]))
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    max_events = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
    threshold = float(sys.argv[3]) if len(sys.argv) > 3 else 1.5e-5
    res = {"tool": "trendbench", "reps": REPS, "calls": {}}
    rc = 0
    for max_len in MAX_LENS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(max_len), str(n), str(max_events),
                                repr(threshold)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            res["stopped"] = f"max_len={max_len}: no result within {STEP_LIMIT_S} s"
            rc = 1
            break
        if p.returncode != 0:
            res["stopped"] = f"max_len={max_len}: exit status {p.returncode}: {p.stderr.strip()[-300:]}"
            rc = 1
            break
        res["calls"][f"max_len_{max_len}"] = json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if rc == 0:
        with open(os.path.join(ROOT, "profiles", "trendbench.json"), "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
