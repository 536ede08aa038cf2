"""merge_split_trades, comp_trade_side_vector (csrc/fmk_preprocess.hip, csrc/fmk_scan.h) and the resampling of bar frames
(csrc/fmk_resample.hip) on the MI355X on the hand-built cases of tests/_preprocess_ref.py: the second 1024-tile trip of the two
one-block scans, moves and heads at thread, wave, row and tile edges, a tile without a head and tiles of heads only, follower sums
across tile edges, the head-relative 1e-8 rule and the 1e-12 epsilon hit exactly, NaN / inf / -0.0 prices and sizes, float32
absorption, timestamps at the int64 ends, what the raw ABI refuses; for the resampling more groups than one launch has waves, groups
of 1 .. 4097 rows in the four dtype combinations, the three paths of the weighted median, first / last in a later chunk, the Kahan
sums' edges.  The resident (`_dev`) entries run with every output prefilled with a sentinel: what must be written is, and nothing
else.  Every output is compared on dtype, length and every element (NaN at the same places); no tolerance anywhere.
tests/test_preprocess_host.py holds the expectations (restatement, C oracle) to the recording of the untouched reference."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _preprocess_ref as H

pytestmark = pytest.mark.gpu

SV_TILE, MG_TILE, TRIP, TRIP_N = H.SV_TILE, H.MG_TILE, H.TRIP, H.TRIP_N
GUARD = 64
I8_SENTINEL, I64_SENTINEL, F64_SENTINEL, F32_SENTINEL = np.int8(77), np.int64(0x5A5A5A5A5A5A5A5A), np.float64(-7.5e300), np.float32(-7.5e33)
c_i64 = C.c_int64


def _ctx():
    from finmlkit_amd import _ffi
    return _ffi.default_context()


def _raw(ctx, fn, *a):
    from finmlkit_amd import _ffi
    rc = getattr(_ffi.lib(), fn)(ctx.handle, *a)
    return rc, _ffi.lib().fmk_last_error(ctx.handle).decode(errors="replace")


def _up(ctx, a):
    from finmlkit_amd._ffi import DeviceArray
    return DeviceArray.from_host(ctx, a)


# ---------------------------------------------------------------------------------------------- tick rule
def _tick_dev(ctx, px):
    """fmk_comp_trade_side_vector_dev on a resident copy; the output is prefilled with 77 and 64 elements longer than n."""
    n = len(px)
    d_p, d_o = _up(ctx, px), _up(ctx, np.full(n + GUARD, I8_SENTINEL, np.int8))
    rc, msg = _raw(ctx, "fmk_comp_trade_side_vector_dev", d_p.p, c_i64(n), d_o.p)
    got = d_o.to_host()
    d_p.free()
    d_o.free()
    assert rc == 0, (rc, msg)
    assert (got[n:] == I8_SENTINEL).all(), "the guard behind the output was written"
    return got[:n]


@pytest.mark.parametrize("name", [n for n in H.TICK_CASES if n in H.LARGE])
def test_tick_rule_second_trip(orc, name):
    """More than 1024 tile aggregates: k_side_scan_tiles carries `run` into its second trip, across whole tiles of zero aggregate on
    both sides of the edge (m <= 0: the last tile of the first trip, the edge from below)."""
    px = H.inputs(name)
    want = orc.comp_trade_side_vector(px)                         # (held to the recording by tests/test_preprocess_host.py)
    info = H.check_structure(name, want)
    n = H.same(_tick_dev(_ctx(), px), want, name + " (_dev)")
    _counts.record(f"preprocess_edges/tick/{name}", cases=1, outputs_compared=n, **info)


def test_tick_rule_small_cases():
    """Placement of the only move (a thread's eight elements, the wave edge at 8 * 64, the tile edge, the last element), its mirror
    image, the epsilon hit exactly and by one ulp more on both signs at the first element of tile 1, NaN / inf / -0.0, n = 1, 2."""
    from finmlkit_amd.bar.utils import comp_trade_side_vector
    ctx = _ctx()
    n = 0
    for name in H.SMALL_TICK:
        px, want = H.inputs(name), H.expected(name)
        H.check_structure(name, want)
        n += H.same(_tick_dev(ctx, px), want, name + " (_dev)")
        n += H.same(comp_trade_side_vector(px), want, name + " (bar.utils)")
    _counts.record("preprocess_edges/tick/small", cases=len(H.SMALL_TICK), outputs_compared=n)


def test_tick_rule_refusals():
    from finmlkit_amd import _ffi
    ctx = _ctx()
    for n in (0, -1, -(2 ** 40)):
        for fn in ("fmk_comp_trade_side_vector_dev", "fmk_comp_trade_side_vector"):
            rc, msg = _raw(ctx, fn, None, c_i64(n), None)
            assert rc == _ffi.E_ARG and "empty input" in msg, (fn, n, rc, msg)
    px = H.inputs("tick.n2.up")
    H.same(_tick_dev(ctx, px), H.expected("tick.n2.up"), "a good call after the refusals")
    _counts.record("preprocess_edges/tick/refused", calls=6)


# ---------------------------------------------------------------------------------------------- merge
MERGE_SENTINELS = ((np.int64, I64_SENTINEL), (np.float64, F64_SENTINEL), (np.float32, F32_SENTINEL), (np.int8, I8_SENTINEL))


class _Merge:
    """One input resident on the device; count() is the count-only phase (null outputs), fill() the fill phase into outputs of
    `n` elements prefilled with sentinels."""

    def __init__(self, ctx, ts, px, am, ibm):
        self.ctx, self.n = ctx, len(ts)
        self.ins = [_up(ctx, ts), _up(ctx, px), _up(ctx, am)]
        self.flag = None if ibm is None else _up(ctx, np.ascontiguousarray(ibm, dtype=np.uint8))
        self.outs = [_up(ctx, np.full(self.n, s, dt)) for dt, s in MERGE_SENTINELS]

    def call(self, outs, side, capacity):
        m = c_i64(-1)
        rc, msg = _raw(self.ctx, "fmk_merge_split_trades_dev", *[d.p for d in self.ins], None if self.flag is None else self.flag.p,
                       c_i64(self.n), *[None if not outs else d.p for d in self.outs[:3]], self.outs[3].p if side else None,
                       c_i64(capacity), C.byref(m))
        return rc, msg, m.value

    def count(self):
        return self.call(False, False, 0)

    def read(self):
        return [d.to_host() for d in self.outs]

    def free(self):
        for d in self.ins + self.outs + ([self.flag] if self.flag is not None else []):
            d.free()


def _merge_dev(ctx, name, ts, px, am, ibm, want):
    """Count-only phase, then the fill phase at capacity n: the two counts agree, outputs [0, m) equal the expectation, [m, n) still
    hold the sentinel, and the side buffer is left alone when no flag is given (null is passed for it).  -> elements compared"""
    mg = _Merge(ctx, ts, px, am, ibm)
    try:
        rc, msg, m1 = mg.count()
        assert rc == 0, (name, rc, msg)
        rc, msg, m2 = mg.call(True, ibm is not None, mg.n)
        assert rc == 0, (name, rc, msg)
        got = mg.read()
    finally:
        mg.free()
    m = len(want[0])
    assert m1 == m2 == m, (name, m1, m2, m)
    n = 0
    for k, g, w, (dt, s) in zip(H.MERGE_KEYS, got, want, MERGE_SENTINELS):
        if k == "side" and ibm is None:
            assert (g == s).all(), f"{name}: side output touched without a flag array"
            continue
        n += H.same(g[:m], w, f"{name} (_dev) {k}")
        assert (g[m:] == s).all(), f"{name}: {k} written past the {m} merged trades"
    return n


def _both_flavours(ctx, name, via_utils):
    from finmlkit_amd.bar.utils import merge_split_trades
    ts, px, am, ibm = H.inputs(name)
    n = 0
    for flag in (ibm, None):
        want = H.expected(name, flag is not None)
        n += _merge_dev(ctx, f"{name} flag={flag is not None}", ts, px, am, flag, want)
        if via_utils:
            for k, g, w in zip(H.MERGE_KEYS, merge_split_trades(ts, px, am, flag), want):
                n += H.same(g, w, f"{name} flag={flag is not None} (bar.utils) {k}")
    return n


def test_merge_second_trip(orc):
    """n = 1024 tiles + 2049: k_scan_tile_scan carries its running total into a second trip; tiles 1023 and 1024 both hold heads,
    and a 2052-trade run of one timestamp crosses the trip edge and the tile edge behind it.  Against the C oracle elementwise."""
    ctx = _ctx()
    name = "merge.trip"
    ts, px, am, ibm = H.inputs(name)
    wants = [orc.merge_split_trades(ts, px, am, ibm), orc.merge_split_trades(ts, px, am, None)]
    info = H.check_structure(name, *wants)
    n = sum(_merge_dev(ctx, f"{name} flag={flag is not None}", ts, px, am, flag, want) for flag, want in zip((ibm, None), wants))
    _counts.record("preprocess_edges/merge/trip", cases=2, outputs_compared=n, merged=len(wants[0][0]), merged_noflag=len(wants[1][0]), **info)


GEOMETRY = ("merge.run_edges", "merge.nohead", "merge.all_heads", "merge.one_trade", "merge.emit_edges")
VALUES = tuple(n for n in H.SMALL_MERGE if n not in GEOMETRY)


@pytest.mark.parametrize("name", GEOMETRY)
def test_merge_geometry(name):
    """A run across two tile edges with a middle tile of its heads only; a tile without a head under a follower sum that crosses its
    edges; a tile of heads only and 4097 ticks of one trade; heads at the emit's row and wave edges, their slots asserted."""
    H.check_structure(name, H.expected(name), H.expected(name, False))
    n = _both_flavours(_ctx(), name, via_utils=True)
    _counts.record(f"preprocess_edges/merge/{name}", cases=4, outputs_compared=n)


def test_merge_thresholds_odd_values_flags_timestamps():
    """The head-relative drift chain across a tile edge, a price difference of exactly 1e-8 and one ulp less, NaN / inf / -0.0
    prices and the a-b-a pattern inside one timestamp, absorbed, NaN, inf and -0.0f sizes, flags that flip inside a timestamp and
    flags all set, timestamps at both int64 ends, negative, and equal but not adjacent."""
    ctx = _ctx()
    n = 0
    for name in VALUES:
        H.check_structure(name, H.expected(name), H.expected(name, False))
        n += _both_flavours(ctx, name, via_utils=True)
    # -0.0f alone keeps its sign (array_equal does not tell the zeros apart)
    ts, px, am, ibm = H.inputs("merge.amount.negzero")
    from finmlkit_amd.bar.utils import merge_split_trades
    assert np.signbit(merge_split_trades(ts, px, am, ibm)[2][:2]).all()
    _counts.record("preprocess_edges/merge/values", cases=4 * len(VALUES), outputs_compared=n)


def test_merge_refusals_through_the_raw_abi():
    from finmlkit_amd import _ffi
    ctx = _ctx()
    name = "merge.emit_edges"
    ts, px, am, ibm = H.inputs(name)
    want = H.expected(name)
    m = len(want[0])
    mg = _Merge(ctx, ts, px, am, ibm)
    try:
        rc, msg, got_m = mg.call(True, True, m - 1)               # one slot short: refused, the count reported, nothing written
        assert rc == _ffi.E_CAPACITY and got_m == m and str(m) in msg, (rc, msg, got_m)
        for g, (dt, s) in zip(mg.read(), MERGE_SENTINELS):
            assert (g == s).all(), "an output was written by a refused call"
        rc, msg, got_m = mg.call(True, True, m)                   # exactly enough, on the same context right after
        assert rc == 0 and got_m == m, (rc, msg)
        for k, g, w in zip(H.MERGE_KEYS, mg.read(), want):
            H.same(g[:m], w, f"capacity m: {k}")
    finally:
        mg.free()
    mg = _Merge(ctx, ts, px, am, None)
    try:
        rc, msg, got_m = mg.call(True, True, mg.n)                # a side output without a flag array
        assert rc == _ffi.E_ARG and "is_buyer_maker" in msg, (rc, msg)
        for g, (dt, s) in zip(mg.read(), MERGE_SENTINELS):
            assert (g == s).all(), "an output was written by a refused call"
    finally:
        mg.free()
    for n in (0, -3):
        for fn in ("fmk_merge_split_trades_dev", "fmk_merge_split_trades"):
            rc, msg = _raw(ctx, fn, None, None, None, None, c_i64(n), None, None, None, None, c_i64(0), None)
            assert rc == _ffi.E_ARG and "empty input" in msg, (fn, n, rc, msg)
    _counts.record("preprocess_edges/merge/refused", calls=7)


# ---------------------------------------------------------------------------------------------- resampling
RS_SENTINELS = (F64_SENTINEL,) * 4 + (None, I64_SENTINEL, F32_SENTINEL, F32_SENTINEL, np.uint8(77))


def _n_cu(ctx):
    v = C.c_int64()
    ctx.call("fmk_diag_n_cu", C.byref(v))
    return int(v.value)


def _resample_dev(ctx, name):
    """fmk_resample_bars_dev on resident columns; every output is prefilled with a sentinel and 64 elements longer than the groups:
    every group's element is written (also -7.5e33 or 77 is no answer of any case), and the guard stays.  -> outputs"""
    seg, cols = H.rs_inputs(name)
    G = len(seg) - 1
    vol, vw = cols[4], cols[6]
    ins = [_up(ctx, a) for a in (seg,) + cols]
    sent = [np.full(G + GUARD, (vol.dtype.type(-7.5e33) if s is None else s), w.dtype) for s, w in zip(RS_SENTINELS, H.rs_expected(name))]
    outs = [_up(ctx, a) for a in sent]
    d_seg, d_o, d_h, d_l, d_c, d_vol, d_tr, d_vw, d_med = ins
    rc, msg = _raw(ctx, "fmk_resample_bars_dev", d_seg.p, c_i64(G), d_o.p, d_h.p, d_l.p, d_c.p, d_vol.p, C.c_int(vol.dtype == np.float64),
                   d_tr.p, d_vw.p, C.c_int(vw.dtype == np.float64), d_med.p, *[o.p for o in outs])
    ctx.sync()
    got = [o.to_host() for o in outs]
    for d in ins + outs:
        d.free()
    assert rc == 0, (name, rc, msg)
    for k, g, s in zip(H.RS_OUT, got, sent):
        assert (g[G:] == s[G:]).all(), f"{name}: the guard behind {k} was written"
    return [g[:G] for g in got]


def _resample_frame(name, want):
    """bar.io.resample_bars on the case as a frame: the reference's columns and dtypes, the groups without an open dropped."""
    from finmlkit_amd.bar.io import resample_bars
    df, timeframe = H.rs_frame(name)
    got = resample_bars(df, timeframe)
    keep = want[8] == 1
    assert list(got.columns) == list(H.RS_COLS) and len(got) == keep.sum()
    np.testing.assert_array_equal(got.index.values.astype("datetime64[ns]").astype(np.int64) // (86_400 * 10 ** 9), np.flatnonzero(keep))
    return sum(H.same(got[k].values, w[keep], f"{name} (bar.io) {k}") for k, w in zip(H.RS_COLS, want))


def _resample_case(ctx, name, want, frame=True):
    n = sum(H.same(g, w, f"{name} (_dev) {k}") for k, g, w in zip(H.RS_OUT, _resample_dev(ctx, name), want))
    return n + (_resample_frame(name, want) if frame else 0)


def test_resample_more_groups_than_waves(orc):
    """70 000 groups of 1 .. 3 rows: the launch is capped at n_cu * 32 workgroups of four waves, so past 128 * n_cu groups a wave
    takes a second group (g += nwaves).  Against the C oracle elementwise, the last group included."""
    ctx = _ctx()
    name = "resample.grid"
    seg, cols = H.rs_inputs(name)
    n_cu = _n_cu(ctx)
    assert 0 < 128 * n_cu < len(seg) - 1 == H.GRID_GROUPS
    want = orc.resample_bars(seg, *cols)                          # (held to the recording by tests/test_preprocess_host.py)
    H.rs_check_structure(name, want)
    n = _resample_case(ctx, name, want)
    _counts.record("preprocess_edges/resample/grid", groups=len(seg) - 1, n_cu=n_cu, waves=128 * n_cu, outputs_compared=n)


def test_resample_group_sizes_in_the_four_dtype_combinations():
    """Groups of 1, 63, 64, 65, 128, 129 and 4097 rows in one call: the wave-wide median path up to 64 rows, the bisection past it,
    whole and partial 64-row chunks; volume float32 / float64 x vwap float32 / float64."""
    ctx = _ctx()
    seen, n = set(), 0
    for combo in H.COMBOS:
        name = f"resample.sizes.{combo}"
        want = H.rs_expected(name)
        H.rs_check_structure(name, want)
        cols = H.rs_inputs(name)[1]
        seen.add((cols[4].dtype.name, cols[6].dtype.name, want[4].dtype.name))
        n += _resample_case(ctx, name, want)
    assert seen == {(v, w, v) for v in ("float32", "float64") for w in ("float32", "float64")}
    _counts.record("preprocess_edges/resample/sizes", cases=len(H.COMBOS), outputs_compared=n)


def test_resample_weighted_median_first_last_and_sums():
    """Zero total trades, a cumulative weight equal to the cutoff, a cutoff inside a run of equal sizes, NaN medians with the
    majority, all-NaN, +-inf and -0.0 medians, each at 40, 64, 65 and 130 rows; first open / last close in the second chunk, a group
    without any open between two valid ones, an all-NaN high; float32 / float64 absorption that Kahan recovers, an infinity (the
    compensation reset), NaN volume or vwap rows, a volume sum of zero."""
    ctx = _ctx()
    names = ["resample.median", "resample.firstlast"] + [f"resample.sums.{c}" for c in H.COMBOS]
    n = 0
    for name in names:
        want = H.rs_expected(name)
        H.rs_check_structure(name, want)
        n += _resample_case(ctx, name, want)
    _counts.record("preprocess_edges/resample/edges", cases=len(names), outputs_compared=n)


def test_resample_no_groups():
    """n_groups 0 is not an error in either flavour and writes nothing."""
    ctx = _ctx()
    for fn, extra in (("fmk_resample_bars_dev", ()), ("fmk_resample_bars", (c_i64(0),))):
        rc, msg = _raw(ctx, fn, None, c_i64(0), *extra, None, None, None, None, None, C.c_int(0), None, None, C.c_int(1), None,
                       *([None] * 9))
        assert rc == 0, (fn, rc, msg)
    _counts.record("preprocess_edges/resample/no_groups", calls=2)
