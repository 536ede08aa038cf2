#!/usr/bin/env python3
"""Times the encoded-series entropies (csrc/fmk_lz.hip) on resident messages of n = 1e7 codes, in one run:
  - fmk_match_lengths_dev at the lookbacks 16, 64, 256 and 1024 on a random binary message AND on a constant one: the kernel's work
    is meant not to depend on the data, and the ratio constant / random says whether it does;
  - fmk_kontoyiannis_entropy_dev (lookback = window / 4) and fmk_plugin_entropy_dev (binary, word 2; and word 8 at the windows that
    hold one) at the windows 64, 256 and 1024 on the random message; fmk_encode_dev of the returns with one edge and with 254;
  - beside them, as yardsticks, fmk_approximate_entropy_dev (m = 2, tolerance 0.2) and fmk_zscore_dev at the same windows on the
    float64 returns the message encodes.
Per call one untimed launch, then REPS timed ones with the context's HIP-event timer; the median counts.  Prints one JSON line and,
with an output path, writes it there.
usage: lzbench.py [SCALE [OUT.json]]        SCALE < 1 shrinks n (a smoke run)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from finmlkit_amd import _ffi  # noqa: E402
from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64  # noqa: E402
from finmlkit_amd.feature.core import lz  # noqa: E402

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lzbench.json")
REPS = 5
LOOKBACKS = (16, 64, 256, 1024)
WINDOWS = (64, 256, 1024)


def main():
    ctx = _ffi.default_context()
    n = max(8192, int(1e7 * SCALE))
    rng = np.random.default_rng(18)
    ret = rng.normal(0.0, 1e-4, n)
    returns = DeviceArray.from_host(ctx, ret)
    random = DeviceArray.from_host(ctx, (ret >= 0.0).astype(np.uint8))
    constant = DeviceArray.from_host(ctx, np.ones(n, np.uint8))
    out64 = DeviceArray(ctx, n, np.float64)
    out16 = DeviceArray(ctx, n, np.uint16)
    out8 = DeviceArray(ctx, n, np.uint8)
    res = {"tool": "lzbench", "n": n, "reps": REPS, "calls": {}, "constant_over_random": {}}

    def timed(key, call, out, **note):
        call()                                                       # warm-up: the code object, the pool's blocks
        ms = []
        for _ in range(REPS):
            ctx.timer_start()
            call()
            ms.append(ctx.timer_stop())
        head = out.view(0, min(n, 100_000)).to_host().astype(np.float64)
        res["calls"][key] = dict(note, ms_median=statistics.median(ms), ms=ms, finite_in_head=int(np.isfinite(head).sum()),
                                 checksum=float(np.nansum(head)))
        print(key, res["calls"][key]["ms_median"], file=sys.stderr, flush=True)

    match = lz.entries("match_lengths")[1]
    for lookback in LOOKBACKS:
        for name, msg in (("random", random), ("constant", constant)):
            timed(f"match_lengths_{name}_n{lookback}",
                  lambda: _ffi.check(match(ctx.handle, msg.p, n, lookback, out16.p), ctx.handle), out16, lookback=lookback, message=name,
                  ballots=n // 64 * lookback * (1 + (lookback + 62) // 64))
        res["constant_over_random"][f"n{lookback}"] = (res["calls"][f"match_lengths_constant_n{lookback}"]["ms_median"] /
                                                       res["calls"][f"match_lengths_random_n{lookback}"]["ms_median"])
    konto, plugin, encode = (lz.entries(f)[1] for f in ("kontoyiannis_entropy", "plugin_entropy", "encode"))
    for window in WINDOWS:
        timed(f"kontoyiannis_w{window}", lambda: _ffi.check(konto(ctx.handle, random.p, n, window, window // 4, out64.p), ctx.handle),
              out64, window=window, lookback=window // 4)
        for word in (2, 8):
            timed(f"plugin_w{window}_word{word}", lambda: _ffi.check(plugin(ctx.handle, random.p, n, window, word, 2, out64.p), ctx.handle),
                  out64, window=window, word=word, alphabet=2)
        timed(f"apen_w{window}", lambda: ctx.call("fmk_approximate_entropy_dev", returns.p, c_i64(n), c_i64(window), c_i64(2), c_f64(0.2),
                                                  out64.p), out64, window=window)
        timed(f"zscore_w{window}", lambda: ctx.call("fmk_zscore_dev", returns.p, c_i64(n), c_i64(window), c_i64(0), out64.p), out64,
              window=window)
    for n_edges in (1, 254):
        edges = np.ascontiguousarray(np.linspace(-3e-4, 3e-4, n_edges) if n_edges > 1 else np.zeros(1))
        timed(f"encode_e{n_edges}", lambda: _ffi.check(encode(ctx.handle, returns.p, n, _ffi.ptr(edges), n_edges, out8.p), ctx.handle),
              out8, n_edges=n_edges)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
