"""Device-resident tick->bar pipeline (no PCIe traffic between stages).

`DeviceTrades` holds the four trade columns in HBM; the methods enqueue the HIP kernels of
csrc/ on the context's stream through the *_dev entry points of include/fmk.h and return
`DeviceArray`s.  The NumPy drop-in functions of finmlkit_amd.bar / finmlkit_amd.feature and
bench.py are thin layers over this module.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np

from . import _ffi
from ._ffi import (DIRECTIONAL_FIELDS, FOOTPRINT_BAR_FIELDS, FOOTPRINT_FLAT_FIELDS, MICROSTRUCTURE_FIELDS, Context, DeviceArray,
                   DirectionalOut, FootprintOut, MicrostructureOut, c_f64, c_i64, c_vp)
from .feature.core import clock, fracdiff, lz
from .feature.core.structural_break import adf
from .feature.series_ops import OPS, resident

DENSE_GAP_MOD = 100_000_000          # mean gap 50 ms, no empty 1-min bar
SPARSE_GAP_MOD = 500_000_000_000     # "sparse" variant: exercises empty bars

OHLCV_FIELDS = [("open", np.float64), ("high", np.float64), ("low", np.float64), ("close", np.float64),
                ("volume", np.float32), ("vwap", np.float64), ("trades", np.int64),
                ("median_trade_size", np.float64)]


class DeviceTrades:
    """Trade columns resident in HBM: ts int64 ns, price f64, amount f32|f64, side int8."""
    ctx: Optional[Context] = None        # set by __init__; the series features refuse their arguments without one

    def __init__(self, ctx: Context, ts: DeviceArray, price: DeviceArray, amount: DeviceArray,
                 side: Optional[DeviceArray]):
        self.ctx, self.ts, self.price, self.amount, self._side = ctx, ts, price, amount, side
        self._side_host = None
        self.n = price.n
        self.amount_is_f64 = int(amount.dtype == np.float64)
        # the tape's certified int32 price grid (csrc/fmk_common.h): set by the constructors that know the price column is final
        # (from_numpy, synth without head-room) and carried by place(); a hand-built trade set and a with_halo view have none
        self.price_k, self.price_grid = None, None

    @property
    def side(self) -> Optional[DeviceArray]:
        """The side column; with from_numpy(..., lazy_side=True) it is uploaded when something first asks for it (build_ohlcv,
        the threshold indexers and the tick-level features never do)."""
        if self._side is None and self._side_host is not None:
            self._side = DeviceArray.from_host(self.ctx, self._side_host)
            self._side_host = None
        return self._side

    @side.setter
    def side(self, v):
        self._side, self._side_host = v, None

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_numpy(cls, ts, price, amount, side=None, ctx: Optional[Context] = None, lazy_side: bool = False) -> "DeviceTrades":
        ctx = ctx or _ffi.default_context()
        am, _ = _ffi.amount_array(amount)
        # np.ascontiguousarray / asarray copy only when the dtype or the layout differs (a frame's columns arrive as they are)
        host = [np.ascontiguousarray(ts, dtype=np.int64), np.ascontiguousarray(price, dtype=np.float64), am]
        sd = None if side is None else np.ascontiguousarray(side, dtype=np.int8)
        if sd is not None and not lazy_side:
            host.append(sd)
        dev = _ffi.upload_columns(ctx, host)      # ONE call for the frame (csrc/fmk_upload.hip)
        t = cls(ctx, dev[0], dev[1], dev[2], dev[3] if len(dev) > 3 else None)
        if sd is not None and lazy_side:
            t._side_host = sd                     # a reference to the caller's column (or its int8 copy); uploaded on first use
        t._build_price_grid()
        return t

    def _build_price_grid(self):
        """One pass over the FINAL price column, once per tape: the int32 grid column, where every price certifies."""
        self.price_k, self.price_grid = _ffi.price_grid_build(self.ctx, self.price)

    @classmethod
    def synth(cls, n: int, seed: int = 42, first: int = 0, gap_mod: int = DENSE_GAP_MOD,
              ctx: Optional[Context] = None, headroom: int = 0, into=None) -> "DeviceTrades":
        """Ticks [first, first+n) of the synthetic stream, generated on the device.

        `headroom` reserves that many elements *in front* of every column (multi-GPU halo)."""
        ctx = ctx or _ffi.default_context()
        if into is not None:
            # the four columns carved out of ONE caller-owned allocation at byte offset `into[1]` (each column on a 2 MiB boundary):
            # bench.py's placement probe -- the level of the reducers depends on where in device memory the columns lie
            slab, off = into
            cols, at = [], int(off)
            for dt in (np.int64, np.float64, np.float32, np.int8):
                nb = (n + headroom) * np.dtype(dt).itemsize
                assert at + nb <= slab.nbytes, "DeviceTrades.synth(into=...): the slab is too small"
                cols.append(DeviceArray(ctx, n + headroom, dt, slab.ptr + at, owner=slab))
                at += (nb + (2 << 20) - 1) // (2 << 20) * (2 << 20)
        else:
            cols = [DeviceArray(ctx, n + headroom, dt) for dt in (np.int64, np.float64, np.float32, np.int8)]
        v = [c.view(headroom, n) for c in cols]
        ctx.call("fmk_synth_trades_dev", C.c_uint64(seed), c_i64(first), c_i64(n), C.c_uint64(gap_mod),
                 v[0].p, v[1].p, v[2].p, v[3].p)
        t = cls(ctx, *v)
        t._backing = cols if into is None else []
        t._headroom = headroom
        if headroom == 0:                         # (a shard's halo elements are written later: its price column is not final)
            t._build_price_grid()
        return t

    # ------------------------------------------------------------------ placement (opt-in)
    def place(self, probe, positions: int = 7, stride: int = 16 << 30, reps: int = 6, warm: int = 3):
        """Opt-in, and it DOUBLES the device memory of the columns for the life of the returned object (the slab and the original
        columns both stay): choose WHERE in device memory the columns lie.  A trade set with head-room in front of it (a shard made for
        the halo exchange, `with_halo`) is refused -- place the columns before sharding.  The reducers that stream whole bars (k_bar_ohlcv_small ...) run up to
        10 % slower when their input columns fall into certain physical blocks of HBM (profiles/r04_placement_regions.txt: whole
        16 .. 128 GiB stretches, constant for an allocation's life; small separate allocations land in them more often than one
        large one).  `place` makes ONE allocation that holds `positions` copies' worth of address space, copies the columns to every
        `stride` bytes of it in turn, times `probe(trades)` -- the caller's own first call, e.g. `lambda t: t.time_bars_ohlcv(60.0)`
        -- on each with the context's HIP-event timer (`warm` untimed + `reps` timed calls), and returns the trade set at the fastest
        position (the original columns are left alone and also take part as position 0).

        -> (DeviceTrades, info) with info = {"probe_ms": [...], "offset_gib": [None, 0, ...], "chosen": k}.  The slab stays
        allocated for the life of the returned object (releasing it moved the level of other allocations: r04_sharded_step.txt).
        Costs positions x (a device-to-device copy of the columns + the probes): set-up, once per trade set."""
        ctx = self.ctx
        if getattr(self, "_headroom", 0):
            raise ValueError("place(): this trade set has head-room for a halo in front of its columns (a shard); the placed copy "
                             "would lose it -- place the columns before sharding")
        cols = [c for c in (self.ts, self.price, self.amount, self.side) if c is not None]
        if self.price_k is not None:              # the grid column travels with the others: every position is probed alike
            cols.append(self.price_k)
        span = sum((c.nbytes + (2 << 20) - 1) // (2 << 20) * (2 << 20) for c in cols)
        span = (span + (1 << 30) - 1) // (1 << 30) * (1 << 30)
        # positions 1 .. P-1 lie every `step` bytes of ONE slab (they may overlap: one copy lives at a time, the best is copied again
        # at the end); as many as fit beside 8 GiB of working memory
        step = max(int(stride), 2 << 20)
        free, _ = ctx.mem_info()
        k = max(0, int(positions) - 1)
        while k > 0 and (k - 1) * step + span > free - (8 << 30):
            k -= 1
        slab = None
        while k > 0 and slab is None:
            try:
                slab = DeviceArray(ctx, (k - 1) * step + span, np.uint8)
            except Exception:                                        # noqa: BLE001 -- a refused allocation: fewer positions
                k -= 1

        def timed(t):
            for _ in range(warm):
                probe(t)
            best = None
            for _ in range(reps):
                ctx.timer_start()
                probe(t)
                ms = ctx.timer_stop()
                best = ms if best is None else min(best, ms)
            return best

        def at(off):
            out, o = [], int(off)
            for c in cols:
                out.append(DeviceArray(ctx, c.n, c.dtype, slab.ptr + o, owner=slab))
                o += (c.nbytes + (2 << 20) - 1) // (2 << 20) * (2 << 20)
            for src, dst in zip(cols, out):
                ctx.call("fmk_d2d", dst.p, src.p, C.c_size_t(src.nbytes))
            k = out.pop() if self.price_k is not None else None
            if self.side is None:
                out.append(None)
            t = DeviceTrades(ctx, *out)
            t._first_last = getattr(self, "_first_last", None)
            t.price_k, t.price_grid = k, (self.price_grid if k is not None else None)
            return t

        ms, offs = [timed(self)], [None]
        if slab is not None:
            for i in range(k):
                ms.append(timed(at(i * step)))
                offs.append(i * step)
        best = min(range(len(ms)), key=lambda i: ms[i])
        chosen = self if best == 0 else at(offs[best])
        if chosen is not self:
            chosen._placement_keep = (slab, self)
        return chosen, {"probe_ms": ms, "offset_gib": [None if o is None else o / float(1 << 30) for o in offs], "chosen": best}

    def without_grid(self) -> "DeviceTrades":
        """The same columns (no copy) as a trade set that carries no price grid: its reducers read the float64 price column."""
        if self.price_k is None:
            return self
        import copy
        t = copy.copy(self)
        t.price_k, t.price_grid = None, None
        return t

    def with_halo(self, k: int) -> "DeviceTrades":
        """View that also covers the k elements in front of the shard (already filled by the caller)."""
        assert k <= getattr(self, "_headroom", 0)
        h = self._headroom
        cols = [b.view(h - k, self.n + k) for b in self._backing]
        t = DeviceTrades(self.ctx, *cols)
        t._backing, t._headroom = self._backing, h - k
        return t

    def to_numpy(self):
        return (self.ts.to_host(), self.price.to_host(), self.amount.to_host(),
                None if self.side is None else self.side.to_host())

    # ------------------------------------------------------------------ indexers
    def first_last_ts(self) -> Tuple[int, int]:
        """timestamps[0], timestamps[-1] (what the reference reads from its host array, logic.py:33-36);
        fetched from the device once per trade set and cached -- the columns are immutable."""
        if getattr(self, "_first_last", None) is None:
            a = self.ts.view(0, 1).to_host()[0]
            b = self.ts.view(self.n - 1, 1).to_host()[0]
            self._first_last = (int(a), int(b))
        return self._first_last

    def time_bar_index(self, interval_seconds: float, clock_params=None,
                       out: Optional[Tuple[DeviceArray, DeviceArray]] = None) -> Tuple[DeviceArray, DeviceArray]:
        """_time_bar_indexer (logic.py:12-51) -> (bar_clock, bar_close_indices) on the device.

        `out` = preallocated (clock, idx) buffers with capacity >= n_edges (views of them are returned)."""
        if clock_params is None:
            t0, t1 = self.first_last_ts()
            ne, e0, d = c_i64(), c_i64(), c_i64()
            _ffi.check(_ffi.lib().fmk_time_bar_clock(c_i64(t0), c_i64(t1), c_f64(interval_seconds),
                                                     C.byref(ne), C.byref(e0), C.byref(d)))
            clock_params = (ne.value, e0.value, d.value)
        ne, e0, d = clock_params
        if out is not None:
            clock, idx = out[0].view(0, ne), out[1].view(0, ne)
        else:
            clock = DeviceArray(self.ctx, ne, np.int64)
            idx = DeviceArray(self.ctx, ne, np.int64)
        self.ctx.call("fmk_time_bar_indexer_dev", self.ts.p, c_i64(self.n), c_i64(e0), c_i64(d), c_i64(ne),
                      clock.p, idx.p)
        return clock, idx

    def time_bars_ohlcv(self, interval_seconds: float, want_median: bool = True, clock_params=None,
                        out_index: Optional[Tuple[DeviceArray, DeviceArray]] = None,
                        out: Optional[Dict[str, DeviceArray]] = None):
        """TimeBarKit.build_ohlcv on the resident columns in ONE library call (kit.py:42-66 -> base.py:126-158):
        _time_bar_indexer + comp_bar_ohlcv -> (bar_clock, bar_close_indices, ohlcv dict), the same values as
        time_bar_index() followed by bar_ohlcv().  For 1-minute-sized bars it is one kernel launch (the edge search runs
        inside the OHLCV + median kernel)."""
        if clock_params is None:
            t0, t1 = self.first_last_ts()
            ne, e0, d = c_i64(), c_i64(), c_i64()
            _ffi.check(_ffi.lib().fmk_time_bar_clock(c_i64(t0), c_i64(t1), c_f64(interval_seconds),
                                                     C.byref(ne), C.byref(e0), C.byref(d)))
            clock_params = (ne.value, e0.value, d.value)
        ne, e0, d = clock_params
        t0, t1 = self.first_last_ts()
        if out_index is not None:
            clock, idx = out_index[0].view(0, ne), out_index[1].view(0, ne)
        else:
            clock, idx = DeviceArray(self.ctx, ne, np.int64), DeviceArray(self.ctx, ne, np.int64)
        out = out or self.alloc_ohlcv(max(ne - 1, 0), want_median)
        med = out["median_trade_size"].p if (want_median and "median_trade_size" in out) else None
        grid = self._grid_args()
        self.ctx.call("fmk_time_bars_ohlcv" + ("_grid_dev" if grid else "_dev"), self.ts.p, self.price.p, self.amount.p,
                      C.c_int(self.amount_is_f64),
                      c_i64(self.n), c_i64(t0), c_i64(t1), c_i64(e0), c_i64(d), c_i64(ne), clock.p, idx.p,
                      out["open"].p, out["high"].p, out["low"].p, out["close"].p, out["volume"].p, out["vwap"].p,
                      out["trades"].p, med, *grid)
        return clock, idx, out

    def _grid_args(self):
        """The two extra arguments of the *_grid_dev entry points; empty without a certified grid."""
        return () if self.price_k is None else (self.price_k.p, C.byref(self.price_grid))

    def tick_bar_index(self, threshold: int) -> DeviceArray:
        m = c_i64()
        self.ctx.call("fmk_tick_bar_indexer_dev", c_i64(self.n), c_i64(int(threshold)), None, c_i64(0), C.byref(m))
        out = DeviceArray(self.ctx, m.value, np.int64)
        self.ctx.call("fmk_tick_bar_indexer_dev", c_i64(self.n), c_i64(int(threshold)), out.p, c_i64(m.value),
                      C.byref(m))
        return out

    def _threshold_index(self, fn, cols, threshold) -> DeviceArray:
        m, unc = c_i64(), c_i64()
        self.ctx.call(fn, *cols, c_i64(self.n), c_f64(threshold), None, c_i64(0), C.byref(m), C.byref(unc))
        out = DeviceArray(self.ctx, m.value, np.int64)
        self.ctx.call(fn, *cols, c_i64(self.n), c_f64(threshold), out.p, c_i64(m.value), C.byref(m), C.byref(unc))
        self.last_uncertified = unc.value
        return out

    def volume_bar_index(self, threshold: float) -> DeviceArray:
        return self._threshold_index("fmk_volume_bar_indexer_dev", (self.amount.p, C.c_int(self.amount_is_f64)),
                                     threshold)

    def dollar_bar_index(self, threshold: float) -> DeviceArray:
        return self._threshold_index("fmk_dollar_bar_indexer_dev",
                                     (self.price.p, self.amount.p, C.c_int(self.amount_is_f64)), threshold)

    def _flow_bar_index(self, rule: str, threshold: float, kind: str) -> DeviceArray:
        _ffi.flow_kind(kind)
        if self.side is None:
            raise ValueError(f"{rule} bars need the side column of the trades")
        if self.n == 0:
            d = DeviceArray(self.ctx, 1, np.int64)
            d.zero()
            return d
        return _ffi.flow_bar_index(self.ctx, rule, kind, self.price, self.amount, self.amount_is_f64, self.side, self.n,
                                   float(threshold))

    def imbalance_bar_index(self, threshold: float, kind: str = "volume") -> DeviceArray:
        """Imbalance bars with a fixed threshold on the resident columns (bar.logic._imbalance_bar_indexer)."""
        return self._flow_bar_index("imbalance", threshold, kind)

    def run_bar_index(self, threshold: float, kind: str = "volume") -> DeviceArray:
        """Run bars with a fixed threshold on the resident columns (bar.logic._run_bar_indexer)."""
        return self._flow_bar_index("run", threshold, kind)

    def gather_ts(self, close_idx: DeviceArray) -> DeviceArray:
        out = DeviceArray(self.ctx, close_idx.n, np.int64)
        self.ctx.call("fmk_gather_i64_dev", self.ts.p, c_i64(self.n), close_idx.p, c_i64(close_idx.n), out.p)
        return out

    # ------------------------------------------------------------------ reducers
    def alloc_ohlcv(self, n_bars: int, want_median: bool = True) -> Dict[str, DeviceArray]:
        return {k: DeviceArray(self.ctx, n_bars, dt) for k, dt in OHLCV_FIELDS
                if want_median or k != "median_trade_size"}

    def bar_ohlcv(self, close_idx: DeviceArray, want_median: bool = True,
                  out: Optional[Dict[str, DeviceArray]] = None) -> Dict[str, DeviceArray]:
        """comp_bar_ohlcv (base.py:306-407) on device-resident columns."""
        nb = close_idx.n - 1
        out = out or self.alloc_ohlcv(max(nb, 0), want_median)
        med = out["median_trade_size"].p if (want_median and "median_trade_size" in out) else None
        grid = self._grid_args()
        self.ctx.call("fmk_comp_bar_ohlcv" + ("_grid_dev" if grid else "_dev"), self.price.p, self.amount.p,
                      C.c_int(self.amount_is_f64),
                      c_i64(self.n), close_idx.p, c_i64(close_idx.n), out["open"].p, out["high"].p,
                      out["low"].p, out["close"].p, out["volume"].p, out["vwap"].p, out["trades"].p, med, *grid)
        return out

    def bar_median(self, close_idx: DeviceArray, out: DeviceArray) -> DeviceArray:
        self.ctx.call("fmk_comp_bar_median_dev", self.amount.p, C.c_int(self.amount_is_f64), c_i64(self.n),
                      close_idx.p, c_i64(close_idx.n), out.p)
        return out

    def bar_trade_size(self, close_idx: DeviceArray, theta, theta_mult: float = 5.0) -> Dict[str, np.ndarray]:
        """comp_bar_trade_size_features (base.py:549-612) -> host float32 arrays keyed like the reference's
        DataFrame columns."""
        nb = close_idx.n - 1
        th = DeviceArray.from_host(self.ctx, np.ascontiguousarray(theta, dtype=np.float64))
        keys = ("mean_size_rel", "size_95_rel", "pct_block", "size_gini")
        out = {k: DeviceArray(self.ctx, nb, np.float32) for k in keys}
        self.ctx.call("fmk_comp_bar_trade_size_dev", self.amount.p, C.c_int(self.amount_is_f64), c_i64(self.n), th.p,
                      close_idx.p, c_i64(close_idx.n), c_f64(theta_mult), *[out[k].p for k in keys])
        return {k: v.to_host() for k, v in out.items()}

    def bar_directional(self, close_idx: DeviceArray) -> Tuple[Dict[str, DeviceArray], DeviceArray]:
        """comp_bar_directional_features (base.py:409-546); second value: device count of bars without a
        signed tick (the reference raises ZeroDivisionError for those)."""
        nb = close_idx.n - 1
        out = {k: DeviceArray(self.ctx, nb, dt) for k, dt in DIRECTIONAL_FIELDS}
        st = DirectionalOut(**{k: out[k].ptr for k in out})
        nz = DeviceArray(self.ctx, 1, np.int64)
        nz.zero()
        self.ctx.call("fmk_comp_bar_directional_dev", self.price.p, self.amount.p, C.c_int(self.amount_is_f64),
                      c_i64(self.n), close_idx.p, c_i64(close_idx.n), self.side.p, C.byref(st), nz.p)
        return out, nz

    def bar_microstructure(self, close_idx: DeviceArray) -> Dict[str, DeviceArray]:
        """comp_bar_microstructure_features on device-resident columns: the eight float64 columns stay in HBM."""
        if self.side is None:
            raise ValueError("the microstructure features need the side column of the trades")
        nb = max(close_idx.n - 1, 0)
        out = {k: DeviceArray(self.ctx, nb, dt) for k, dt in MICROSTRUCTURE_FIELDS}
        st = MicrostructureOut(**{k: out[k].ptr for k in out})
        self.ctx.call("fmk_comp_bar_microstructure_dev", self.price.p, self.amount.p, C.c_int(self.amount_is_f64),
                      c_i64(self.n), close_idx.p, c_i64(close_idx.n), self.side.p, C.byref(st))
        return out

    def bar_footprints(self, close_idx: DeviceArray, lows: DeviceArray, highs: DeviceArray,
                       price_tick_size: float, imbalance_factor: float = 3.0):
        """comp_bar_footprints (base.py:615-850) in CSR form -> (level_offsets, flat, per_bar, n_bad)."""
        nb = close_idx.n - 1
        off = DeviceArray(self.ctx, nb + 1, np.int64)
        tot, mx = c_i64(), c_i64()
        self.ctx.call("fmk_comp_bar_footprints_size_dev", lows.p, highs.p, c_i64(nb), c_f64(price_tick_size),
                      off.p, C.byref(tot), C.byref(mx))
        flat = {k: DeviceArray(self.ctx, tot.value, dt) for k, dt in FOOTPRINT_FLAT_FIELDS}
        bar = {k: DeviceArray(self.ctx, nb, dt) for k, dt in FOOTPRINT_BAR_FIELDS}
        st = FootprintOut(**{k: v.ptr for k, v in {**flat, **bar}.items()})
        bad = DeviceArray(self.ctx, 1, np.int64)
        bad.zero()
        self.ctx.call("fmk_comp_bar_footprints_fill_dev", self.price.p, self.amount.p,
                      C.c_int(self.amount_is_f64), c_i64(self.n), close_idx.p, c_i64(close_idx.n), self.side.p,
                      c_f64(price_tick_size), lows.p, c_f64(imbalance_factor), off.p, c_i64(mx.value),
                      C.byref(st), bad.p)
        return off, flat, bar, bad

    def bars_fused(self, close_idx: DeviceArray, price_tick_size: float, imbalance_factor: float = 3.0,
                   want_median: bool = True):
        """cfg 4: build_ohlcv + build_directional_features + build_footprints semantics in two passes over the ticks
        (13 B/tick each: OHLCV + order-flow in one kernel, then the footprints, whose sweep also takes the median trade size).

        -> (ohlcv, directional, n_zero_div, level_offsets, flat, per_bar, n_bad), all device-resident."""
        nb = close_idx.n - 1
        o = self.alloc_ohlcv(max(nb, 0), want_median)
        med = o["median_trade_size"].p if want_median else None
        off = DeviceArray(self.ctx, nb + 1, np.int64)
        tot, mx = c_i64(), c_i64()
        d = {k: DeviceArray(self.ctx, nb, dt) for k, dt in DIRECTIONAL_FIELDS}
        dst = DirectionalOut(**{k: d[k].ptr for k in d})
        cnts = DeviceArray(self.ctx, 2, np.int64)
        cnts.zero()
        # pass 1: OHLCV and the order-flow features from ONE read of price / amount / side, then the level counts.  The median
        # trade size is left to pass 2 when the library says so (float32 amounts, 600..2048-tick bars): 26 B/tick in all
        deferred = C.c_int(0)
        self.ctx.call("fmk_bars_flow_size_defer_dev", self.price.p, self.amount.p, C.c_int(self.amount_is_f64), c_i64(self.n),
                      close_idx.p, c_i64(close_idx.n), self.side.p, c_f64(price_tick_size), o["open"].p, o["high"].p,
                      o["low"].p, o["close"].p, o["volume"].p, o["vwap"].p, o["trades"].p, med, C.byref(dst),
                      cnts.view(0, 1).p, off.p, C.byref(tot), C.byref(mx), C.byref(deferred))
        flat = {k: DeviceArray(self.ctx, tot.value, dt) for k, dt in FOOTPRINT_FLAT_FIELDS}
        bar = {k: DeviceArray(self.ctx, nb, dt) for k, dt in FOOTPRINT_BAR_FIELDS}
        fst = FootprintOut(**{k: v.ptr for k, v in {**flat, **bar}.items()})
        # pass 2: the footprints (+ the median of the amounts each wave has just swept)
        self.ctx.call("fmk_comp_bar_footprints_fill_median_dev", self.price.p, self.amount.p, C.c_int(self.amount_is_f64),
                      c_i64(self.n), close_idx.p, c_i64(close_idx.n), self.side.p, c_f64(price_tick_size), o["low"].p,
                      c_f64(imbalance_factor), off.p, c_i64(mx.value), C.byref(fst), cnts.view(1, 1).p,
                      med if deferred.value else None)
        return o, d, cnts.view(0, 1), off, flat, bar, cnts.view(1, 1)

    # ------------------------------------------------------------------ tick-level features
    def lagged_returns(self, window_sec: float, is_log: bool, close: Optional[DeviceArray] = None) -> DeviceArray:
        out = DeviceArray(self.ctx, self.n, np.float64)
        self.ctx.call("fmk_comp_lagged_returns_dev", self.ts.p, (close or self.price).p, c_i64(self.n),
                      c_f64(window_sec), C.c_int(bool(is_log)), out.p)
        return out

    def ewmst(self, y: DeviceArray, half_life: float, sigma_floor: float = 1e-12, mean0: bool = False) -> DeviceArray:
        out = DeviceArray(self.ctx, self.n, np.float64)
        self.ctx.call("fmk_ewmst_dev", self.ts.p, y.p, c_i64(self.n), c_f64(half_life), c_f64(sigma_floor),
                      C.c_int(bool(mean0)), out.p)
        return out

    def ewms(self, y: DeviceArray, span: int) -> DeviceArray:
        out = DeviceArray(self.ctx, y.n, np.float64)
        self.ctx.call("fmk_ewms_dev", y.p, c_i64(y.n), c_i64(int(span)), out.p)
        return out

    def realized_vol(self, r: DeviceArray, window: int, is_sample: bool) -> DeviceArray:
        out = DeviceArray(self.ctx, r.n, np.float64)
        self.ctx.call("fmk_realized_vol_dev", r.p, c_i64(r.n), c_i64(int(window)), C.c_int(bool(is_sample)), out.p)
        return out

    # ------------------------------------------------------------------ series features: one `resident` call per row of
    # feature/series_ops.py, which checks the arguments, the dtype and the lengths before the context is looked at
    # rolling-window moments (csrc/fmk_rolling.hip)
    def sma(self, y: DeviceArray, window: int) -> DeviceArray:
        """sma (feature/core/ma.py:46-62) of a resident float64 series."""
        return resident(self.ctx, OPS["sma"], (y,), window)

    def zscore(self, y: DeviceArray, window: int, ddof: int = 0) -> DeviceArray:
        """comp_zscore (feature/core/utils.py:67-90) of a resident float64 series; ValueError when window - ddof <= 0."""
        return resident(self.ctx, OPS["zscore"], (y,), window, ddof)

    def rolling_variance(self, y: DeviceArray, window: int, ddof: int = 1, min_periods: int = 1) -> DeviceArray:
        """rolling_variance_nb (feature/core/volatility.py:440-478) of a resident float64 series."""
        return resident(self.ctx, OPS["rolling_variance"], (y,), window, ddof, min_periods)

    def variance_ratio_1_4(self, window: int = 32, ddof: int = 0, ret_type: str = "log",
                           series: Optional[DeviceArray] = None) -> DeviceArray:
        """variance_ratio_1_4_core (feature/core/volatility.py:481-540) on a resident float64 series (default: the price column)."""
        return resident(self.ctx, OPS["variance_ratio_1_4"], (self.price if series is None else series,), window, ddof, ret_type == "log")

    # windowed order statistics (csrc/fmk_order.hip)
    def burst_ratio(self, y: DeviceArray, window: int) -> DeviceArray:
        """comp_burst_ratio (feature/core/utils.py:92-108) of a resident float64 series: y / its rolling median."""
        return resident(self.ctx, OPS["burst_ratio"], (y,), window)

    def roc(self, y: DeviceArray, period: int) -> DeviceArray:
        """roc (feature/core/momentum.py:6-22) of a resident float64 series."""
        return resident(self.ctx, OPS["roc"], (y,), period)

    def pct_change(self, y: DeviceArray, periods: int) -> DeviceArray:
        """pct_change (feature/core/utils.py:110-124) of a resident float64 series."""
        return resident(self.ctx, OPS["pct_change"], (y,), periods)

    def stoch_k(self, close: DeviceArray, low: DeviceArray, high: DeviceArray, length: int) -> DeviceArray:
        """stoch_k (feature/core/momentum.py:68-112) of three resident float64 series of one length."""
        return resident(self.ctx, OPS["stoch_k"], (close, low, high), length)

    # recursive indicators (csrc/fmk_recur.hip)
    def ewma(self, y: DeviceArray, span) -> DeviceArray:
        """ewma (feature/core/ma.py:6-43) of a resident float64 series."""
        return resident(self.ctx, OPS["ewma"], (y,), span)

    def rsi_wilder(self, close: DeviceArray, window: int) -> DeviceArray:
        """rsi_wilder (feature/core/momentum.py:25-65) of a resident float64 series."""
        return resident(self.ctx, OPS["rsi_wilder"], (close,), window)

    def true_range(self, high: DeviceArray, low: DeviceArray, close: DeviceArray) -> DeviceArray:
        """true_range (feature/core/volatility.py:222-253) of three resident float64 series of one length."""
        return resident(self.ctx, OPS["true_range"], (high, low, close))

    def atr(self, high: DeviceArray, low: DeviceArray, close: DeviceArray, window: int, ema_based: bool = False,
            normalize: bool = False) -> DeviceArray:
        """atr (feature/core/volatility.py:352-437) of three resident float64 series of one length."""
        return resident(self.ctx, OPS["atr"], (high, low, close), window, ema_based, normalize)

    def adx(self, high: DeviceArray, low: DeviceArray, close: DeviceArray, length: int = 14) -> DeviceArray:
        """adx_core (feature/core/trend.py:8-96) of three resident float64 series of one length."""
        return resident(self.ctx, OPS["adx"], (high, low, close), length)

    # running-sum indicators (csrc/fmk_runsum.hip)
    def bollinger_percent_b(self, y: DeviceArray, window: int, num_std: float = 2.0) -> DeviceArray:
        """bollinger_percent_b (feature/core/volatility.py:289-338) of a resident float64 series."""
        return resident(self.ctx, OPS["bollinger_percent_b"], (y,), window, num_std)

    def vwap_distance(self, close: DeviceArray, volume: DeviceArray, n_periods: int, is_log: bool = False) -> DeviceArray:
        """vwap_distance (feature/core/reversion.py:9-56) of two resident float64 series of one length."""
        return resident(self.ctx, OPS["vwap_distance"], (close, volume), n_periods, is_log)

    def parkinson_range(self, high: DeviceArray, low: DeviceArray) -> DeviceArray:
        """parkinson_range (feature/core/volatility.py:341-349) of two resident float64 series of one length."""
        return resident(self.ctx, OPS["parkinson_range"], (high, low))

    def flow_acceleration(self, volumes: DeviceArray, window: int, recent_periods: int) -> DeviceArray:
        """comp_flow_acceleration (feature/core/volume.py:572-607) of a resident float64 series."""
        return resident(self.ctx, OPS["flow_acceleration"], (volumes,), window, recent_periods)

    def vpin(self, volume_buy: DeviceArray, volume_sell: DeviceArray, window: int) -> DeviceArray:
        """vpin (feature/core/volume.py:610-641) of two resident float64 series of one length -> a float32 array."""
        return resident(self.ctx, OPS["vpin"], (volume_buy, volume_sell), window)

    # rolling price-volume correlation (csrc/fmk_corr.hip)
    def price_volume_corr(self, price: DeviceArray, volume: DeviceArray, window: int) -> DeviceArray:
        """rolling_price_volume_correlation (feature/core/correlation.py:10-111) of two resident float64 series of one length."""
        return resident(self.ctx, OPS["price_volume_corr"], (price, volume), window)

    # window statistics (csrc/fmk_shape.hip)
    def kurtosis(self, y: DeviceArray, window: int) -> DeviceArray:
        """rolling_kurtosis (feature/core/shape.py; reference transforms.py:900-933) of a resident float64 series."""
        return resident(self.ctx, OPS["rolling_kurtosis"], (y,), window)

    def trend_slope(self, y: DeviceArray, window: int) -> DeviceArray:
        """trend_slope (feature/core/shape.py; reference transforms.py:936-988) of a resident float64 price series, in degrees."""
        return resident(self.ctx, OPS["trend_slope"], (y,), window)

    def hurst_exponent(self, y: DeviceArray, window: int) -> DeviceArray:
        """hurst_exponent (feature/core/shape.py; reference transforms.py:1341-1397) of a resident float64 series; ValueError when
        window < 9."""
        return resident(self.ctx, OPS["hurst_exponent"], (y,), window)

    def bipower_variation(self, y: DeviceArray, window: int) -> DeviceArray:
        """bipower_variation (feature/core/shape.py; reference transforms.py:1551-1602) of a resident float64 series."""
        return resident(self.ctx, OPS["bipower_variation"], (y,), window)

    # approximate entropy (csrc/fmk_entropy.hip)
    def approximate_entropy(self, y: DeviceArray, window: int, m: int = 2, tolerance: float = 0.2) -> DeviceArray:
        """approximate_entropy (feature/core/entropy.py; reference transforms.py:1400-1457) of a resident float64 series; ValueError
        for the arguments that function refuses."""
        return resident(self.ctx, OPS["approximate_entropy"], (y,), window, m, tolerance)

    # the causal FIR filter and fractional differentiation (csrc/fmk_fir.hip); the weights are host numbers
    def fir(self, y: DeviceArray, weights) -> DeviceArray:
        """fir (feature/core/fracdiff.py) of a resident float64 series: out[t] = sum_k weights[k] * y[t-k], one fused multiply-add
        per tap, oldest first; ValueError for the weights that function refuses."""
        return fracdiff.resident(self.ctx, y, weights)

    def frac_diff(self, y: DeviceArray, d: float, threshold: float = 1e-5) -> DeviceArray:
        """frac_diff_ffd (feature/core/fracdiff.py) of a resident float64 series: the fixed-width window fractional
        differentiation of order d; ValueError for a d or a threshold that frac_diff_weights refuses."""
        return fracdiff.resident(self.ctx, y, fracdiff.frac_diff_weights(d, threshold))

    # the encoding and the entropies of an encoded series (csrc/fmk_lz.hip); the edges are host numbers, a message is a uint8 array
    def encode(self, y: DeviceArray, edges) -> DeviceArray:
        """encode (feature/core/lz.py) of a resident float64 series -> a uint8 array of codes: the edges at or below each element,
        255 for a NaN; ValueError for the edges that function refuses."""
        return lz.resident(self.ctx, "encode", y, edges)

    def plugin_entropy(self, codes: DeviceArray, window: int, word: int = 1, alphabet: int = 2) -> DeviceArray:
        """plugin_entropy (feature/core/lz.py) of a resident uint8 message, in bits per symbol; ValueError for the arguments that
        function refuses."""
        return lz.resident(self.ctx, "plugin_entropy", codes, window, word, alphabet)

    def match_lengths(self, codes: DeviceArray, lookback: int) -> DeviceArray:
        """match_lengths (feature/core/lz.py) of a resident uint8 message -> a uint16 array."""
        return lz.resident(self.ctx, "match_lengths", codes, lookback)

    def kontoyiannis_entropy(self, codes: DeviceArray, window: int, lookback: int) -> DeviceArray:
        """kontoyiannis_entropy (feature/core/lz.py) of a resident uint8 message, in bits per symbol; ValueError for the arguments
        that function refuses."""
        return lz.resident(self.ctx, "kontoyiannis_entropy", codes, window, lookback)

    # the bar clock, run lengths and the opening range (csrc/fmk_clock.hip).  ts=None: the tape's own stamps; a DeviceArray of bar
    # stamps (int64 nanoseconds, e.g. from gather_ts) may be given instead
    def bar_duration(self, periods: int = 1, ts: Optional[DeviceArray] = None) -> DeviceArray:
        """Seconds between row i and row i - periods (reference transforms.py:1511-1548), NaN where there is no such row."""
        return clock.resident(self.ctx, clock.CLOCK_OPS["bar_duration"], (self.ts if ts is None else ts,), int(periods))[0]

    def bar_duration_ewma(self, span=20, ts: Optional[DeviceArray] = None) -> DeviceArray:
        """ewma of the bar durations, NaN at row 0 (reference transforms.py:1460-1508); ValueError when span < 1."""
        span = clock.rule_span(span)
        return clock.resident(self.ctx, clock.CLOCK_OPS["bar_duration_ewma"], (self.ts if ts is None else ts,), span)[0]

    def bar_rate(self, window_sec: float, ts: Optional[DeviceArray] = None) -> DeviceArray:
        """Rows per hour over the closed window of window_sec seconds that ends at each row (reference transforms.py:1210-1270);
        ValueError for a window below one nanosecond."""
        w = clock.window_ns(window_sec)
        return clock.resident(self.ctx, clock.CLOCK_OPS["bar_rate"], (self.ts if ts is None else ts,), float(window_sec), w)[0]

    def dir_run_len(self, y: DeviceArray) -> DeviceArray:
        """The length of the run of equal signs each row of a resident float64 series ends (reference transforms.py:1605-1664) -> an
        int8 array."""
        return clock.resident(self.ctx, clock.CLOCK_OPS["dir_run_len"], (y,))[0]

    def orb_break(self, high: DeviceArray, low: DeviceArray, close: DeviceArray, ts: Optional[DeviceArray] = None):
        """Opening-range breakouts per UTC day (reference transforms.py:1122-1207) of three resident float64 series -> (orb_long,
        orb_short), two uint8 arrays.  Strictly increasing stamps."""
        return clock.resident(self.ctx, clock.CLOCK_OPS["orb_break"], (self.ts if ts is None else ts, high, low, close),
                              unequal=clock.ORB_RESIDENT_SHAPE_MESSAGE)

    # ------------------------------------------------------------------ event sampling
    def cusum_filter(self, threshold, series: Optional[DeviceArray] = None) -> DeviceArray:
        """cusum_filter (sampling/filters.py:7-70) on a resident float64 series (default: the price column) -> int64 event indices
        on the device, as `triple_barrier` takes them.  `threshold`: a float, or a DeviceArray with one value per element."""
        x = self.price if series is None else series
        if x.n <= 1:
            raise ValueError("Input time series must have at least 2 elements.")
        if isinstance(threshold, DeviceArray):
            if threshold.n != 1 and threshold.n != x.n:
                raise ValueError("Threshold array must either contain 1 const. element or len(raw_time_series) elements.")
            thr = threshold
        else:
            thr = DeviceArray.from_host(self.ctx, np.array([threshold], dtype=np.float64))
        # one call when the guess holds (an event per 64 ticks or fewer); otherwise the count it reports sizes the second
        m = c_i64()
        out = DeviceArray(self.ctx, max(1024, x.n // 64), np.int64)
        args = (x.p, c_i64(x.n), thr.p, c_i64(thr.n))
        if self.ctx.call("fmk_cusum_filter_dev", *args, out.p, c_i64(out.n), C.byref(m), None, allow=(_ffi.E_CAPACITY,)) != _ffi.OK:
            out = DeviceArray(self.ctx, m.value, np.int64)
            self.ctx.call("fmk_cusum_filter_dev", *args, out.p, c_i64(out.n), C.byref(m), None)
        if m.value == out.n:
            return out
        ev = DeviceArray(self.ctx, m.value, np.int64)                  # an array of its own: `out` is released with this frame
        if m.value:
            self.ctx.call("fmk_d2d", ev.p, out.p, C.c_size_t(ev.nbytes))
        return ev

    # ------------------------------------------------------------------ structural breaks
    def cusum_test_rolling(self, window_size: int = 1000, warmup_period: int = 30, series: Optional[DeviceArray] = None):
        """cusum_test_rolling (feature/core/structural_break/cusum.py:179-274) on a resident float64 series (default: the price
        column) -> (up, down, crit_up, crit_down), four resident float64 arrays.  ValueError when a price is <= 0."""
        if warmup_period < 2:
            raise ValueError("warmup_period must be at least 2.")
        x = self.price if series is None else series
        if x.dtype != np.float64:
            raise TypeError(f"cusum_test_rolling: the series must be float64, not {x.dtype}")
        out = tuple(DeviceArray(self.ctx, x.n, np.float64) for _ in range(4))
        if x.n:
            self.ctx.call("fmk_cusum_test_rolling_dev", x.p, c_i64(x.n), c_i64(max(0, int(window_size))), c_i64(int(warmup_period)),
                          *[o.p for o in out])
        return out

    def sadf(self, min_len: int, max_len: Optional[int] = None, lags: int = 1, trend: str = "c", step: int = 1,
             end_idx: Optional[DeviceArray] = None, series: Optional[DeviceArray] = None):
        """sadf (feature/core/structural_break/adf.py) on a resident float64 series (default: the price
        column; pass log prices for the book's test) -> (stat float64, start int64, n_skipped): the supremum ADF statistic of every
        end point, the first row of the window that attains it (-1 without one) and a device int64 counting the end points without
        a usable window.  end_idx: an int64 DeviceArray of end points, as `cusum_filter` returns its events; None: every element.
        max_len None: all history.  ValueError for the arguments that function refuses."""
        return adf.resident(self.ctx, self.price if series is None else series, end_idx, min_len, max_len, lags, trend, step)

    def adf_rolling(self, window: int, lags: int = 1, trend: str = "c", series: Optional[DeviceArray] = None) -> DeviceArray:
        """adf_rolling (feature/core/structural_break/adf.py) on a resident float64 series (default: the price column): the ADF
        statistic of the `window` rows that end at every element."""
        return adf.resident(self.ctx, self.price if series is None else series, None, window, window, lags, trend, 1)[0]

    # ------------------------------------------------------------------ labels and sample weights
    def triple_barrier(self, event_idx: DeviceArray, targets: DeviceArray, horizontal_barriers, vertical_barrier: float,
                       min_close_time_sec: float, side: Optional[DeviceArray] = None, min_ret: float = 0.0):
        """triple_barrier (label/tbm.py:11-158) on the resident tape; events, targets and sides are DeviceArrays (int64, float64,
        int8).  -> (labels int8, touch_idx int64, returns float64, max_rb_ratios float64, n_skipped): n_skipped is a device
        int64 counting the events whose window holds no later tick (label 0, NaN, touch_idx = event_idx)."""
        if targets.n != event_idx.n:
            raise ValueError("The lengths of event_idxs and targets must match.")
        if side is not None and side.n != event_idx.n:
            raise ValueError("The length of event_idxs must match the length of side.")
        ne = event_idx.n
        bottom, top = horizontal_barriers
        out = (DeviceArray(self.ctx, ne, np.int8), DeviceArray(self.ctx, ne, np.int64), DeviceArray(self.ctx, ne, np.float64),
               DeviceArray(self.ctx, ne, np.float64))
        skipped = DeviceArray(self.ctx, 1, np.int64)
        skipped.zero()
        self.ctx.call("fmk_triple_barrier_dev", self.ts.p, self.price.p, c_i64(self.n), event_idx.p, targets.p,
                      None if side is None else side.p, c_i64(ne), c_f64(bottom), c_f64(top), c_f64(vertical_barrier),
                      c_f64(min_close_time_sec), c_f64(min_ret), out[0].p, out[1].p, out[2].p, out[3].p, skipped.p)
        return out + (skipped,)

    def trend_scanning(self, event_idx: DeviceArray, min_len: int, max_len: int, step: int = 1,
                       series: Optional[DeviceArray] = None):
        """trend_scanning (label/trend_scanning.py) on a resident float64 series (default: the price column);
        events are an int64 DeviceArray, as `cusum_filter` returns them.  -> (labels int8, t_value float64, touch_idx int64,
        ret float64, n_skipped): n_skipped is a device int64 counting the events whose longest span runs past the end of the series
        or all of whose spans hold a NaN (label 0, NaN, touch_idx = event_idx).  touch_idx is what `label_concurrency` and
        `label_weights` take."""
        from .label.trend_scanning import check_arguments
        y = self.price if series is None else series
        if y.dtype != np.float64:
            raise TypeError(f"trend_scanning: the series must be float64, not {y.dtype}")
        if event_idx.dtype != np.int64:
            raise TypeError(f"trend_scanning: the event indices must be int64, not {event_idx.dtype}")
        min_len, max_len, step = check_arguments(y.n, None, min_len, max_len, step)
        ne = event_idx.n
        out = (DeviceArray(self.ctx, ne, np.int8), DeviceArray(self.ctx, ne, np.float64), DeviceArray(self.ctx, ne, np.int64),
               DeviceArray(self.ctx, ne, np.float64))
        skipped = DeviceArray(self.ctx, 1, np.int64)
        skipped.zero()
        self.ctx.call("fmk_trend_scanning_dev", y.p, c_i64(y.n), event_idx.p, c_i64(ne), c_i64(min_len), c_i64(max_len),
                      c_i64(step), out[0].p, out[1].p, out[2].p, out[3].p, skipped.p)
        return out + (skipped,)

    def label_concurrency(self, event_idx: DeviceArray, touch_idx: DeviceArray) -> DeviceArray:
        """The concurrency column of average_uniqueness (label/weights.py:31-38): int16 per tick."""
        if touch_idx.n != event_idx.n:
            raise ValueError("Timestamps and lookahead indices must have the same length.")
        out = DeviceArray(self.ctx, self.n, np.int16)
        self.ctx.call("fmk_label_concurrency_dev", event_idx.p, touch_idx.p, c_i64(event_idx.n), c_i64(self.n), out.p)
        return out

    def label_weights(self, event_idx: DeviceArray, touch_idx: DeviceArray, concurrency: DeviceArray,
                      want_attribution: bool = True) -> Tuple[DeviceArray, Optional[DeviceArray]]:
        """average uniqueness and (not normalised) return attribution of the events from one pass over price + concurrency
        (label/weights.py:41-47, 76-94) -> (avg_uniqueness, return_attribution or None)."""
        ne = event_idx.n
        avg = DeviceArray(self.ctx, ne, np.float64)
        att = DeviceArray(self.ctx, ne, np.float64) if want_attribution else None
        self.ctx.call("fmk_label_weights_dev", self.price.p, concurrency.p, c_i64(self.n), event_idx.p, touch_idx.p, c_i64(ne),
                      avg.p, None if att is None else att.p)
        return avg, att

    def sequential_bootstrap(self, event_idx: DeviceArray, touch_idx: DeviceArray, n_draws: Optional[int] = None, n_runs: int = 1,
                             seed: int = 0, return_uniqueness: bool = False):
        """sequential_bootstrap (label/bootstrap.py) on resident spans, as `triple_barrier` and
        `trend_scanning` return them, on this tape's axis -> draws, a flat run-major int64 DeviceArray of n_runs * n_draws positions
        in the event arrays; with return_uniqueness also the int64 DeviceArray of each drawn event's average uniqueness when it was
        drawn, in units of 2^-30.  The library reads the two index arrays back for the host-side compression of the axis (16 bytes
        per event, nothing of the tape), so the call waits for the stream."""
        from .label.bootstrap import check_arguments
        if touch_idx.n != event_idx.n:
            raise ValueError("sequential_bootstrap: event_idxs and touch_idxs must have the same length.")
        if event_idx.dtype != np.int64 or touch_idx.dtype != np.int64:
            raise TypeError("sequential_bootstrap: the event and touch indices must be int64")
        if event_idx.n < 1:
            raise ValueError("sequential_bootstrap: n_events must be between 1 and 2^31 - 1.")
        n_draws, n_runs, seed, dpl = check_arguments(event_idx.n, n_draws, n_runs, seed, None)
        draws = DeviceArray(self.ctx, n_runs * n_draws, np.int64)
        q = DeviceArray(self.ctx, n_runs * n_draws, np.int64) if return_uniqueness else None
        self.ctx.call("fmk_sequential_bootstrap_dev", event_idx.p, touch_idx.p, c_i64(event_idx.n), c_i64(self.n), c_i64(n_draws),
                      c_i64(n_runs), C.c_uint64(seed), None, c_i64(dpl), draws.p, None if q is None else q.p)
        return (draws, q) if return_uniqueness else draws

    def _bet_events(self, what: str, event_idx: DeviceArray, touch_idx: DeviceArray, per_event: DeviceArray, dtype, name: str):
        if touch_idx.n != event_idx.n or per_event.n != event_idx.n:
            raise ValueError(f"{what}: event_idxs, touch_idxs and {name} must have the same length.")
        if event_idx.dtype != np.int64 or touch_idx.dtype != np.int64:
            raise TypeError(f"{what}: the event and touch indices must be int64")
        if per_event.dtype != dtype:
            raise TypeError(f"{what}: {name} must be {np.dtype(dtype)}, not {per_event.dtype}")
        if event_idx.n < 1:
            raise ValueError(f"{what}: n_events must be between 1 and 2^31 - 1.")

    def bet_size_path(self, event_idx: DeviceArray, touch_idx: DeviceArray, signal: DeviceArray, step: float = 0.0,
                      return_count: bool = False):
        """bet_size_path (label/betsize.py) on resident spans, as `triple_barrier` and `trend_scanning` return
        them, and a resident float64 signal per event -> the float64 position per tick of this tape: the average of the signals of
        the events open on event_idx <= t < touch_idx, discretised when step > 0; with return_count also the int16 number of open
        events.  ValueError for what the library counts on the device: a span outside the tape, a signal that is NaN or outside
        [-1, 1], more than 32767 events open on one tick."""
        from .label.betsize import check_step
        self._bet_events("bet_size_path", event_idx, touch_idx, signal, np.float64, "signal")
        step = check_step("bet_size_path", step)
        value = DeviceArray(self.ctx, self.n, np.float64)
        count = DeviceArray(self.ctx, self.n, np.int16) if return_count else None
        self.ctx.call("fmk_bet_size_path_dev", event_idx.p, touch_idx.p, signal.p, c_i64(event_idx.n), c_i64(self.n), c_f64(step),
                      value.p, None if count is None else count.p)
        return (value, count) if return_count else value

    def bet_size_at(self, event_idx: DeviceArray, touch_idx: DeviceArray, signal: DeviceArray, at_idx: Optional[DeviceArray] = None,
                    step: float = 0.0) -> DeviceArray:
        """The path of `bet_size_path` at the ticks of an int64 DeviceArray (None: each event's own tick); the path is a temporary
        of the call.  ValueError also for an index outside the tape."""
        from .label.betsize import check_step
        self._bet_events("bet_size_at", event_idx, touch_idx, signal, np.float64, "signal")
        step = check_step("bet_size_at", step)
        at = event_idx if at_idx is None else at_idx
        if at.dtype != np.int64:
            raise TypeError("bet_size_at: the indices must be int64")
        out = DeviceArray(self.ctx, at.n, np.float64)
        self.ctx.call("fmk_bet_size_at_dev", event_idx.p, touch_idx.p, signal.p, c_i64(event_idx.n), c_i64(self.n), c_f64(step),
                      at.p, c_i64(at.n), out.p)
        return out

    def bet_size_budget(self, event_idx: DeviceArray, touch_idx: DeviceArray, side: DeviceArray):
        """bet_size_budget (label/betsize.py) on resident spans and a resident int8 side per event -> (m float64 per tick of this
        tape, max2): max2 is a device int64 pair, the largest number of concurrent long and short bets."""
        self._bet_events("bet_size_budget", event_idx, touch_idx, side, np.int8, "side")
        m, max2 = DeviceArray(self.ctx, self.n, np.float64), DeviceArray(self.ctx, 2, np.int64)
        self.ctx.call("fmk_bet_size_budget_dev", event_idx.p, touch_idx.p, side.p, c_i64(event_idx.n), c_i64(self.n), m.p, max2.p)
        return m, max2


def to_host(d: Dict[str, DeviceArray]) -> Dict[str, np.ndarray]:
    return {k: v.to_host() for k, v in d.items()}
