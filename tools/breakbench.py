#!/usr/bin/env python3
"""Times the CSW CUSUM structural-break test (fmk_cusum_test_rolling_dev / fmk_cusum_test_developing_dev) on a resident synthetic
price column with the context's HIP-event timer and prints one JSON line.

Workloads: rolling at (n = 1e7, window 1000) and (n = 1e8, window 50), developing at n = 2e5.  Per workload one untimed call, then
REPS timed ones (the minimum counts); pairs from fmk_diag_cusum_test_last -> pairs per second.  The kernel is compute bound and the
only meaningful bound is the issue rate, so the line also carries the VALU instructions of one pair step of k_brk_pairs, counted in
the ISA the build's own flags give (needs hipcc; "valu_per_pair": null without it).
usage: breakbench.py [SCALE]        SCALE < 1 shrinks every n (a smoke run)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_i64  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
REPS = 3
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math".split()


def valu_per_pair():
    """VALU instructions in the innermost loop of the pair pass of k_brk_pairs: the loop body that holds the v_div_scale_f64 of the
    quotient (one pair per lane and trip)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "finmlkit_amd", "csrc", "fmk_break.hip")
    try:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "brk.s")
            subprocess.check_call([hipcc, *FLAGS, "--cuda-device-only", "-S", "-o", out, src], stderr=subprocess.DEVNULL)
            txt = open(out).read()
    except (OSError, subprocess.CalledProcessError):
        return None
    m = re.search(r"^_ZN\S*k_brk_pairs\S*:[^\n]*\n(.*?)\n\s*s_endpgm", txt, flags=re.S | re.M)
    if not m:
        return None
    # the pair step: the innermost loop that holds the quotient's v_div_scale_f64 -- from its header label to the branch back to it
    body = m.group(1).split("\n")
    labels = {ln.split(":")[0]: i for i, ln in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", ln)}
    best = None
    for i, ln in enumerate(body):
        b = re.match(r"\s*s_c?branch\w* (\.LBB\d+_\d+)", ln)
        if b and b.group(1) in labels and labels[b.group(1)] < i:
            blk = body[labels[b.group(1)]:i]
            if any("v_div_scale_f64" in x for x in blk):
                n = sum(1 for x in blk if re.match(r"\s*v_", x))
                best = n if best is None else min(best, n)
    return best


def main():
    ctx = _ffi.default_context()
    res = {"tool": "breakbench", "reps": REPS, "valu_per_pair": valu_per_pair(), "calls": {}}

    def run(name, n, window):
        t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
        out = [DeviceArray(ctx, n, np.float64) for _ in range(4)]

        def call():
            if window is None:
                ctx.call("fmk_cusum_test_developing_dev", t.price.p, c_i64(n), c_i64(30), *[o.p for o in out])
            else:
                ctx.call("fmk_cusum_test_rolling_dev", t.price.p, c_i64(n), c_i64(window), c_i64(30), *[o.p for o in out])
        call()
        ms = []
        for _ in range(REPS):
            ctx.timer_start()
            call()
            ms.append(ctx.timer_stop())
        d = (C.c_int64 * 6)()
        ctx.call("fmk_diag_cusum_test_last", d)
        best = min(ms)
        res["calls"][name] = {"n": n, "window": window, "ms_min": best, "ms": ms, "pairs": int(d[1]), "quotients": int(d[3]),
                              "slabs": int(d[2]), "workgroups": int(d[5]), "pairs_per_s": int(d[1]) / (best * 1e-3),
                              "checksum": float(np.nansum(out[0].view(0, min(n, 100_000)).to_host()))}

    run("rolling_w1000", max(2000, int(1e7 * SCALE)), 1000)
    run("rolling_w50", max(2000, int(1e8 * SCALE)), 50)
    run("developing", max(2000, int(2e5 * SCALE ** 0.5)), None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
