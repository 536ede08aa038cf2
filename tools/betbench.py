#!/usr/bin/env python3
"""Times bet sizing on resident spans of a long tape with the context's HIP-event timer and writes one JSON object,
profiles/betbench.json.

Tape axis: TICKS ticks (default 1e9); nothing of a tape is read, the spans alone live on it.  Events: EVENTS of them (default 1e6 and
1e7), starts uniform on the axis, lengths exponential with a mean of 6 000 ticks and capped at 12 000 -- the five to ten minutes a
triple-barrier label lives on the benchmark's synthetic tape of 20 ticks a second -- so the mean concurrency is near 6 and near 60.
Signals uniform on [-1, 1], sides their signs.  Per call one untimed run, then REPS timed ones (all kept, median reported):
bet_size_path without and with the count and with step 0.1, bet_size_budget, bet_size_at on the events' own ticks.  The yardstick is
label_concurrency on the same spans, the nearest existing kernel family; with --yardstick-root DIR it is ALSO measured by a fresh
child process that imports the package (and its library) from DIR, a checkout of the parent commit, on the same seeded spans.
Bytes by construction, per tick: label_concurrency 4 (memset) + 4 (tile sums) + 4 + 2 (apply) = 14; bet_size_path 12 + 12 + 12 + 8 = 44
(+ 2 with the count); bet_size_budget 8 + 8 + 8 + 8 + 8 = 40; bet_size_at 44 and 16 B per index.
usage: betbench.py [--ticks 1e9] [--events 1e6 1e7] [--reps 5] [--out profiles/betbench.json] [--yardstick-root DIR]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8e12


def spans(ticks, events, seed=2024):
    import numpy as np
    rng = np.random.default_rng(seed + events)
    ev = np.sort(rng.integers(0, ticks - 12001, events)).astype(np.int64)
    length = np.minimum(rng.exponential(6000.0, events), 12000.0).astype(np.int64) + 1
    sig = rng.uniform(-1.0, 1.0, events)
    return ev, ev + length, sig


def timed(ctx, fn, reps):
    import numpy as np
    fn()
    ms = []
    for _ in range(reps):
        ctx.timer_start()
        out = fn()
        ms.append(ctx.timer_stop())
        del out
    return {"ms_median": float(np.median(ms)), "ms": ms}


def yardstick(root, ticks, events, reps):
    """label_concurrency on the spans, with the package found under `root` -> {events: timing}"""
    sys.path.insert(0, root)
    import numpy as np
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray, c_i64
    ctx = _ffi.default_context()
    out = {"library": os.path.realpath(_ffi.LIB_PATH)}
    for m in events:
        ev, tc, _ = spans(ticks, m)
        d_ev, d_tc = DeviceArray.from_host(ctx, ev), DeviceArray.from_host(ctx, tc)
        conc = DeviceArray(ctx, ticks, np.int16)
        r = timed(ctx, lambda: ctx.call("fmk_label_concurrency_dev", d_ev.p, d_tc.p, c_i64(m), c_i64(ticks), conc.p), reps)
        r["bytes"] = 14 * ticks
        r["frac_of_8TBs"] = r["bytes"] / (r["ms_median"] * 1e-3) / PEAK
        out[str(m)] = r
        for a in (d_ev, d_tc, conc):
            a.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=float, default=1e9)
    ap.add_argument("--events", type=float, nargs="+", default=[1e6, 1e7])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "betbench.json"))
    ap.add_argument("--yardstick-root", default=None)
    ap.add_argument("--yardstick-only", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    ticks, events = int(args.ticks), [int(e) for e in args.events]
    if args.yardstick_only:
        print(json.dumps(yardstick(args.yardstick_only, ticks, events, args.reps)))
        return
    res = {"tool": "betbench", "ticks": ticks, "reps": args.reps, "layout": "int64 sums + int32 counts (two arrays)", "events": {}}
    if args.yardstick_root:                                              # a fresh process, before this one opens the device
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ticks", str(ticks), "--events", *[str(e) for e in events],
                            "--reps", str(args.reps), "--yardstick-only", os.path.abspath(args.yardstick_root)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"the yardstick process failed ({r.returncode}):\n{r.stderr[-2000:]}")
        res["label_concurrency_parent_library"] = json.loads(r.stdout.strip().split("\n")[-1])
    sys.path.insert(0, ROOT)
    import numpy as np
    from finmlkit_amd import _ffi, engine
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    empty = DeviceArray(ctx, 0, np.float32)
    axis = DeviceArray(ctx, 0, np.int64)
    t = engine.DeviceTrades(ctx, axis, DeviceArray(ctx, 0, np.float64), empty, None)
    t.n = ticks                                                          # the spans' axis; no column of a tape is read
    res["label_concurrency"] = yardstick(ROOT, ticks, events, args.reps)
    for m in events:
        ev, tc, sig = spans(ticks, m)
        d_ev, d_tc, d_sig = (DeviceArray.from_host(ctx, a) for a in (ev, tc, sig))
        d_side = DeviceArray.from_host(ctx, np.sign(sig).astype(np.int8))
        calls = {
            "bet_size_path": (lambda: t.bet_size_path(d_ev, d_tc, d_sig), 44 * ticks),
            "bet_size_path_count": (lambda: t.bet_size_path(d_ev, d_tc, d_sig, return_count=True), 46 * ticks),
            "bet_size_path_step_0.1": (lambda: t.bet_size_path(d_ev, d_tc, d_sig, 0.1), 44 * ticks),
            "bet_size_budget": (lambda: t.bet_size_budget(d_ev, d_tc, d_side), 40 * ticks),
            "bet_size_at_events": (lambda: t.bet_size_at(d_ev, d_tc, d_sig), 44 * ticks + 16 * m),
        }
        one = {"mean_span_ticks": float(np.mean(tc - ev)), "mean_concurrency": float(np.sum(tc - ev) / ticks)}
        for name, (fn, nbytes) in calls.items():
            r = timed(ctx, fn, args.reps)
            r["bytes"] = nbytes
            r["frac_of_8TBs"] = nbytes / (r["ms_median"] * 1e-3) / PEAK
            one[name] = r
            ctx.trim()
        yard = res["label_concurrency"][str(m)]
        one["path_over_label_concurrency"] = {"time_ratio": one["bet_size_path"]["ms_median"] / yard["ms_median"],
                                              "byte_ratio": 44 / 14}
        res["events"][str(m)] = one
        for a in (d_ev, d_tc, d_sig, d_side):
            a.free()
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
