#!/usr/bin/env python3
"""Times the optimal-trading-rule mesh (csrc/fmk_otr.hip), in one run:
  - the book's workload (snippet 13.2): 25 parameter sets (forecasts 10, 5, 0, -5, -10 x half-lives 5, 10, 25, 50, 100, sigma 1), the
    21 x 21 mesh linspace(0, 10, 21), 10^5 paths, max_hp 100; the same with 10^6 paths; one set (forecast 0, half-life 5) at 10^5;
  - what generating the normals costs: the one-set workload with normals= given (the generator's own variates), and beside both
    variants the same call on a 1 x 1 mesh of zero levels, where every path ends at its first step -- what is left of the call there
    is its fixed part (checks, upload of the normals, launches, read-back), and the difference is the walk;
  - tools/otr_check on one host thread on a slice of the book's workload (SLICE paths of every set), scaled to the whole, and the
    device's mesh of that slice against the tool's, bit for bit.
Per workload one untimed call, then REPS timed ones (wall time of the call, which waits for its results); the median counts.  A path
step is one (set, path, step) of the nominal n_cfg * n_paths * max_hp; the walk makes fewer where a path stops early, and the
tool's count of the steps it walked is recorded with the slice.  Prints one JSON line and writes it to the output path.
usage: otrbench.py [SCALE [OUT.json]]        SCALE < 1 shrinks the path counts (a smoke run)"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd.label import otr  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "otrbench.json")
REPS, MAX_HP, SLICE = 5, 100, 1000
FORECASTS, HALF_LIVES = (10.0, 5.0, 0.0, -5.0, -10.0), (5.0, 10.0, 25.0, 50.0, 100.0)
LEVELS = np.linspace(0.0, 10.0, 21)
FIELDS = ("mean", "std", "sharpe", "n_profit", "n_stop", "n_time", "hold")


def timed(call):
    call()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        mesh = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return mesh, ms


def entry(n_cfg, n_paths, ms, **more):
    med = statistics.median(ms)
    return dict(n_cfg=n_cfg, n_paths=n_paths, max_hp=MAX_HP, ms_median=med, ms=ms,
                path_steps_per_s=n_cfg * n_paths * MAX_HP / (med * 1e-3), **more)


def main():
    f = np.repeat(FORECASTS, len(HALF_LIVES))
    hl = np.tile(HALF_LIVES, len(FORECASTS))
    n5, n6 = max(1000, int(1e5 * SCALE)), max(1000, int(1e6 * SCALE))
    res = {"tool": "otrbench", "reps": REPS, "geometry": otr.geometry(), "calls": {}}
    calls = res["calls"]

    mesh, ms = timed(lambda: otr.optimal_trading_rule(f, hl, 1.0, LEVELS, LEVELS, MAX_HP, n5, 13))
    calls["book_1e5"] = entry(25, n5, ms, best=[list(mesh.best(c)) for c in (0, 12, 24)], mean_hold_max=float(mesh.mean_hold.max()))
    _, ms = timed(lambda: otr.optimal_trading_rule(f, hl, 1.0, LEVELS, LEVELS, MAX_HP, n6, 13))
    calls["book_1e6"] = entry(25, n6, ms)
    one, ms = timed(lambda: otr.optimal_trading_rule(0.0, 5.0, 1.0, LEVELS, LEVELS, MAX_HP, n5, 13))
    calls["one_set_1e5"] = entry(1, n5, ms)

    # the generator's share: the same variates handed in
    exe_dir = tempfile.mkdtemp()
    exe = os.path.join(exe_dir, "otr_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "otr_check.cpp"), "-o", exe])
    n_given = min(n5, 20000)                                         # the reference generator is Python: a share of the paths
    from tests import _otr_ref
    z = np.ascontiguousarray(_otr_ref.normals(13, n_given, MAX_HP))
    zero = np.zeros(1)
    gen, ms_gen = timed(lambda: otr.optimal_trading_rule(0.0, 5.0, 1.0, LEVELS, LEVELS, MAX_HP, n_given, 13))
    giv, ms_giv = timed(lambda: otr.optimal_trading_rule(0.0, 5.0, 1.0, LEVELS, LEVELS, MAX_HP, n_given, 13, normals=z))
    _, ms_gen0 = timed(lambda: otr.optimal_trading_rule(0.0, 5.0, 1.0, zero, zero, MAX_HP, n_given, 13))
    _, ms_giv0 = timed(lambda: otr.optimal_trading_rule(0.0, 5.0, 1.0, zero, zero, MAX_HP, n_given, 13, normals=z))
    same = all(np.array_equal(getattr(gen, k), getattr(giv, k), equal_nan=(k == "sharpe")) for k in FIELDS)
    walk_gen = statistics.median(ms_gen) - statistics.median(ms_gen0)
    walk_giv = statistics.median(ms_giv) - statistics.median(ms_giv0)
    calls["normals_share"] = dict(n_paths=n_given, ms_generated=ms_gen, ms_given=ms_giv, ms_generated_first_step_only=ms_gen0,
                                  ms_given_first_step_only=ms_giv0, walk_ms_generated=walk_gen, walk_ms_given=walk_giv,
                                  generator_share_of_walk=(1.0 - walk_giv / walk_gen) if walk_gen > 0 else None,
                                  given_equals_generated=bool(same))

    # one host thread on a slice of the book's workload
    n_slice = min(SLICE, n5)
    dev = otr.optimal_trading_rule(f, hl, 1.0, LEVELS, LEVELS, MAX_HP, n_slice, 13)
    host_s, host_steps, equal = 0.0, 0, True
    for c in range(25):
        args = [str(n_slice), str(MAX_HP), "13", float(dev.forecast[c]).hex(), float(dev.phi[c]).hex(), float(dev.sigma[c]).hex(), "21", "21"]
        args += [float(v).hex() for v in LEVELS] * 2
        out = subprocess.run([exe, "mesh"] + args, capture_output=True, text=True, check=True).stdout
        for line in out.splitlines():
            w = line.split()
            if w[0] == "node":
                i, j = int(w[1]), int(w[2])
                got = [float.fromhex(x) for x in w[3:6]] + [int(x) for x in w[6:]]
                for k, g in zip(FIELDS, got):
                    d = getattr(dev, k)[c, i, j]
                    equal = equal and bool(g == d or (g != g and d != d))
            elif w[0] == "steps":
                host_steps += int(w[1])
                host_s += float(w[3])
    calls["host_one_thread"] = dict(slice_paths=n_slice, n_cfg=25, seconds_slice=host_s, steps_walked_slice=host_steps,
                                    nominal_steps_slice=25 * n_slice * MAX_HP, seconds_scaled_to_book_1e5=host_s * n5 / n_slice,
                                    path_steps_per_s=25 * n_slice * MAX_HP / host_s, device_equals_host_bit_for_bit=equal)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
