#!/usr/bin/env python3
"""The two 1024-wide scan clients of csrc/fmk_wgscan.h that no other tool times, on N resident ticks of the synthetic tape: ms for
comp_trade_side_vector on its price column, and for _cusum_bar_indexer at floor 5e-4 with one NaN put back into sigma before every call
and FMK_CUSUM_LAZY_FILL=0, so that the forward fill (k_ff_tile, the scan of the tile aggregates, k_ff_apply) runs each time.  Four calls
per row: the first is the untimed one.  usage: scanbench.py [N]"""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["FMK_CUSUM_LAZY_FILL"] = "0"
import numpy as np
from finmlkit_amd import _ffi, engine
from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
ctx = _ffi.default_context()
t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
side = DeviceArray(ctx, n, np.int8)
sig = t.ewmst(t.lagged_returns(5.0, True), 60.0)
out, m, rounds = DeviceArray(ctx, n, np.int64), c_i64(), c_i64()
for rep in range(4):
    ctx.timer_start()
    ctx.call("fmk_comp_trade_side_vector_dev", t.price.p, c_i64(n), side.p)
    a = ctx.timer_stop()
    ctx.call("fmk_memset", sig.view(n // 2, 1).p, C.c_int(0xFF), C.c_size_t(8))       # eight 0xFF bytes: a NaN behind the first valid sigma
    ctx.timer_start()
    ctx.call("fmk_cusum_bar_indexer_dev", t.ts.p, t.price.p, sig.p, c_i64(n), c_f64(5e-4), c_f64(2.0), out.p, c_i64(n), C.byref(m), C.byref(rounds))
    b = ctx.timer_stop()
    print("scanbench: tick rule %.3f ms, cusum with sigma fill %.3f ms; %d closes (checksums %d %d)" %
          (a, b, m.value, int(side.view(0, min(n, 1_000_000)).to_host().astype(np.int64).sum()), int(out.view(0, m.value).to_host().sum() % 1000003)), flush=True)
