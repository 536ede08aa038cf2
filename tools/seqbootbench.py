#!/usr/bin/env python3
"""Wall time of label.sequential_bootstrap (host-pointer form: compression, upload, the launches, download) on synthetic label spans:
m events at irregular ticks, as a CUSUM filter leaves them, each span ending at a barrier touch somewhere inside a ten-minute
vertical barrier, so that a dozen labels overlap at a time.  K = m draws; R = 1 run and R = one run per compute unit.  Every timed
call runs in a process of its own after a short warm-up call there (the same events, one launch's draws); the figure is the minimum
of three.  The yardstick is the compressed form of tools/seqboot_check.cpp on one host thread for R = 1: its cost per draw does not
depend on the draw's number, so it is timed over --host-draws draws, whose results also have to equal the first draws of the GPU's
run 0.  One JSON line for profiles/seqbootbench.json.
usage: seqbootbench.py [--m 10000 100000] [--out profiles/seqbootbench.json] [--host-draws 2000]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SEED = 7


def spans(m):
    """-> (event_idx, touch_idx, n): gaps of 50 ticks on average between events, a vertical barrier 1 000 ticks ahead, the touch
    anywhere in its last four fifths"""
    rng = np.random.default_rng(m)
    ev = np.cumsum(rng.geometric(1 / 50.0, m)).astype(np.int64)
    tc = ev + rng.integers(200, 1001, m)
    return ev, tc.astype(np.int64), int(tc.max()) + 1


def child(m, runs, out_path):
    from finmlkit_amd import _ffi
    from finmlkit_amd.label import bootstrap, sequential_bootstrap
    ev, tc, n = spans(m)
    ctx = _ffi.default_context()
    if runs == 0:
        v = C.c_int64()
        ctx.call("fmk_diag_n_cu", C.byref(v))
        runs = int(v.value)
    sequential_bootstrap(ev, tc, bootstrap.geometry()["draws_per_launch"], runs, SEED, n=n)            # the warm-up
    t0 = time.perf_counter()
    draws = sequential_bootstrap(ev, tc, m, runs, SEED, n=n)
    dt = time.perf_counter() - t0
    with open(out_path, "w") as f:
        json.dump({"runs": runs, "seconds": dt, "run0_head": draws[0, :4096].tolist(), "distinct_in_run0": int(len(np.unique(draws[0])))}, f)


def host_yardstick(exe, m, k_host):
    ev, tc, n = spans(m)
    text = " ".join(str(x) for x in [m, n, k_host, 1, SEED, 0] + [int(v) for p in zip(ev, tc) for v in p]) + "\n"
    r = subprocess.run([exe, "time"], input=text, capture_output=True, text=True, check=True)
    lines = r.stdout.strip().split("\n")
    return float(lines[0].split()[1]), [int(x) for x in lines[1].split()[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqbootbench.json"))
    ap.add_argument("--host-draws", type=int, default=2000)
    ap.add_argument("--child", nargs=3, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(int(args.child[0]), int(args.child[1]), args.child[2])
    tmp = tempfile.mkdtemp(prefix="seqbootbench_")
    exe = os.path.join(tmp, "seqboot_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "seqboot_check.cpp"), "-o", exe])
    res = {"seed": SEED, "timed_calls": 3, "rows": []}
    for m in args.m:
        ev, tc, n = spans(m)
        n_intervals = int(len(np.unique(np.concatenate([ev, tc + 1]))) - 1)
        k_host = min(m, args.host_draws)
        host_s, host_draws = host_yardstick(exe, m, k_host)
        for runs in (1, 0):                                       # 0: one run per compute unit
            got = []
            for rep in range(3):
                path = os.path.join(tmp, f"r_{m}_{runs}_{rep}.json")
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(m), str(runs), path])
                got.append(json.load(open(path)))
                kk = min(k_host, 4096)
                assert got[-1]["run0_head"][:kk] == host_draws[:kk], "the GPU's run 0 and the host form differ"
            best = min(g["seconds"] for g in got)
            row = {"m": m, "n_intervals": n_intervals, "n_draws": m, "n_runs": got[0]["runs"], "seconds_min_of_3": best,
                   "seconds_all": [g["seconds"] for g in got], "us_per_draw_of_a_run": best / m * 1e6,
                   "us_per_draw_over_all_runs": best / m / got[0]["runs"] * 1e6, "distinct_in_run0": got[0]["distinct_in_run0"],
                   "host_draws_timed": k_host, "host_us_per_draw": host_s / k_host * 1e6}
            row["host_over_gpu_per_draw_over_all_runs"] = row["host_us_per_draw"] / row["us_per_draw_over_all_runs"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
