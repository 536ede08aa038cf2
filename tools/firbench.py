#!/usr/bin/env python3
"""Times the causal FIR filter (fmk_fir_dev: csrc/fmk_fir.hip) on a resident synthetic log-price series with the weights of the
fractional differentiation: n = 1e8 at W = 55, 282 and 1458 (d = 0.4 at the thresholds 1e-3, 1e-4, 1e-5) and n = 1e6 at W = 4076
(d = 0.1 at 1e-5).  Per shape one untimed call, then REPS timed ones with the context's HIP-event timer (the upload of the weights is
part of the call and of the time); the median counts.  Prints one JSON line -- per shape the times and the achieved fused
multiply-adds per second, n * W / t -- and, with an output path, writes it there.
usage: firbench.py [SCALE [OUT.json]]        SCALE < 1 shrinks n (a smoke run)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi, engine  # noqa: E402
from finmlkit_amd._ffi import DeviceArray  # noqa: E402
from finmlkit_amd.feature.core import fracdiff  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else None
REPS = 7
SHAPES = ((1e8, 0.4, 1e-3, 55), (1e8, 0.4, 1e-4, 282), (1e8, 0.4, 1e-5, 1458), (1e6, 0.1, 1e-5, 4076))


def main():
    ctx = _ffi.default_context()
    n_max = max(10_000, int(1e8 * SCALE))
    logp = DeviceArray.from_host(ctx, np.log(engine.DeviceTrades.synth(n_max, seed=42, ctx=ctx).price.to_host()))
    out = DeviceArray(ctx, n_max, np.float64)
    tile, taps = fracdiff.geometry()
    res = {"tool": "firbench", "reps": REPS, "tile": tile, "taps": taps, "calls": {}}
    for full_n, d, threshold, width in SHAPES:
        n = max(10_000, int(full_n * SCALE))
        w = fracdiff.frac_diff_weights(d, threshold)
        assert len(w) == width
        entry = fracdiff.entries()[1]

        def call():
            _ffi.check(entry(ctx.handle, logp.p, n, _ffi.ptr(w), width, out.p), ctx.handle)
        call()
        ms = []
        for _ in range(REPS):
            ctx.timer_start()
            call()
            ms.append(ctx.timer_stop())
        head = out.view(0, min(n, 100_000)).to_host()
        med = statistics.median(ms)
        res["calls"][f"n{n}_w{width}"] = {"n": n, "width": width, "d": d, "threshold": threshold, "ms_median": med, "ms": ms,
                                         "fma_per_s": n * width / (med * 1e-3), "bytes_per_s": 16.0 * n / (med * 1e-3),
                                         "finite_in_head": int(np.isfinite(head).sum()), "checksum": float(np.nansum(head))}
    line = json.dumps(res)
    print(line)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
