#!/usr/bin/env python3
"""Times the ADF / SADF statistic (fmk_sadf_dev, csrc/fmk_sadf.hip) on a resident synthetic tape with the context's HIP-event timer,
prints one JSON line and writes it to profiles/sadfbench.json.

Calls, all with lags 1, trend "c", min_len 12, step 1 on the price column as it is:
  every    DeviceTrades.synth(N) (default 1e7 rows), every element an end point, max_len 256 and 1 024;
  events   DeviceTrades.synth(EVENT_N) (default 1e8 ticks), the end points the symmetric CUSUM filter's events at THRESHOLD (default
           1.5e-5: the events tools/trendbench.py labels, 412 035 with the one whose forward span does not fit), max_len 256 and 1 024;
  cusum    cusum_test_rolling (csrc/fmk_break.hip) on the first tape at window 256 and 1 024, warm-up 30: it walks the same
           number of (t, s) pairs, with a handful of operations per pair where the ADF regression has some thirty moments.
Every step (an untimed call, then REPS timed ones, the minimum counts) runs in a child process of its own under a time limit, so that
a step that hangs ends alone; after a step that fails nothing more is started.  Per step: the (end point, start point) pairs per
second and the bytes that is by construction, 8 B x (lags + 2) x rows walked, against the time.
usage: sadfbench.py [N] [EVENT_N] [THRESHOLD]
       sadfbench.py --step KIND MAX_LEN N THRESHOLD  (internal) one step, prints its JSON"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 3
MIN_LEN = 12
LAGS = 1
MAX_LENS = (256, 1024)
STEP_LIMIT_S = 180


def step(kind, max_len, n, threshold):
    import numpy as np

    from finmlkit_amd import _ffi, engine
    ctx = _ffi.default_context()
    t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
    res = {"kind": kind, "max_len": max_len, "rows": n}
    if kind == "cusum":
        def call():
            return t.cusum_test_rolling(max_len, 30)
        ends = n
    else:
        d_ev = t.cusum_filter(threshold) if kind == "events" else None
        ends = n if d_ev is None else d_ev.n

        def call():
            return t.sadf(MIN_LEN, max_len, LAGS, "c", 1, end_idx=d_ev)
    call()
    ms = []
    for _ in range(REPS):
        ctx.timer_start()
        out = call()
        ms.append(ctx.timer_stop())
    best = min(ms)
    pairs = ends * (max_len - (30 if kind == "cusum" else MIN_LEN) + 1)
    res.update({"end_points": int(ends), "ms_min": best, "ms": ms, "pairs": pairs, "pairs_per_s": pairs / (best * 1e-3)})
    if kind != "cusum":
        stat, start = out[0].to_host(), out[1].to_host()
        walk_bytes = 8 * (LAGS + 2) * ends * max_len
        res.update({"min_len": MIN_LEN, "lags": LAGS, "trend": "c", "bytes_walk": walk_bytes, "bytes_per_s": walk_bytes / (best * 1e-3),
                    "n_skipped": int(out[2].to_host()[0]), "infinite": int(np.isinf(stat).sum()),
                    "mean_window": float(np.mean((np.arange(n) if kind == "every" else d_ev.to_host())[start >= 0] - start[start >= 0] + 1)),
                    "max_stat": float(np.nanmax(stat))})
    print(json.dumps(res))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]))
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    event_n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 100_000_000
    threshold = float(sys.argv[3]) if len(sys.argv) > 3 else 1.5e-5
    res = {"tool": "sadfbench", "reps": REPS, "calls": {}}
    rc = 0
    for kind, rows in (("every", n), ("cusum", n), ("events", event_n)):
        for max_len in MAX_LENS:
            name = f"{kind}_max_len_{max_len}"
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(max_len), str(rows), repr(threshold)],
                                   capture_output=True, text=True, timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired:
                res["stopped"] = f"{name}: no result within {STEP_LIMIT_S} s"
                rc = 1
                break
            if p.returncode != 0:
                res["stopped"] = f"{name}: exit status {p.returncode}: {p.stderr.strip()[-300:]}"
                rc = 1
                break
            res["calls"][name] = json.loads(p.stdout.strip().splitlines()[-1])
        if rc:
            break
    line = json.dumps(res)
    print(line)
    if rc == 0:
        with open(os.path.join(ROOT, "profiles", "sadfbench.json"), "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
