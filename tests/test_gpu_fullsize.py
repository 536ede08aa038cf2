"""GPU, BASELINE.json sizes (1e9 ticks per GPU): ALL-bar parity with the threaded oracle, size-independent properties, prefix parity.

`test_all_bars_*` compare EVERY bar of the 1e9-tick run with the C oracle, whose per-bar loops run as OpenMP parallel-for over bars
on the GPU box's host cores (ORC_THREADS; ~2e8 ticks/s on 256 cores, so cfg 2 and cfg 4 take seconds each; the columns are copied
back from the device -- the device generator equals orc.synth bit for bit, tests/test_gpu_core.py).  When host memory is short the
comparison covers the longest prefix that fits.  The older tests below check the same runs through
  * causality / prefix parity: every bar that closes inside the first P ticks must equal the oracle's bar
    computed from those P ticks alone (bars depend only on their own ticks; threshold-bar closes only on
    earlier ticks) -- the full-size run is compared with the oracle on the prefix, bit for bit;
  * conservation laws over ALL bars (trade counts, exact dyadic volumes across bar granularities,
    footprint rows vs bar totals), ordering and envelope invariants.
FMK_FULLSIZE_TICKS overrides the size (default 1e9; reduced automatically if HBM is short); `<n>:prefix` lets a host that
cannot hold all columns compare a prefix (host_cols)."""
import os

import numpy as np
import pytest

from tests import _golden as G
from tests._counts import record

pytestmark = pytest.mark.gpu

PREFIX = 3_000_000


@pytest.fixture(scope="module")
def big():
    from finmlkit_amd import _ffi, engine
    ctx = _ffi.default_context()
    n = int(float(os.environ.get("FMK_FULLSIZE_TICKS", "1e9").split(":")[0]))
    free, _ = ctx.mem_info()
    n = min(n, int((free - (8 << 30)) // 60))           # columns + footprint / threshold scratch head-room
    t = engine.DeviceTrades.synth(n, seed=42, ctx=ctx)
    return engine, t, n


@pytest.fixture(scope="module")
def prefix(orc):
    return orc.synth(42, 0, PREFIX)


def test_time_bars_full_size(big, prefix, orc):
    engine, t, n = big
    ts, px, am, sd = prefix
    clock, ci = t.time_bar_index(60.0)
    o = engine.to_host(t.bar_ohlcv(ci))
    cih, clk = ci.to_host(), clock.to_host()
    nb = len(cih) - 1
    # --- structure
    assert np.all(np.diff(clk) == 60_000_000_000) and np.all(np.diff(cih) >= 0) and cih[-1] == n - 1
    assert o["trades"].sum() == cih[-1] - cih[0] and np.array_equal(o["trades"], np.diff(cih))
    # --- envelopes
    assert np.all(o["high"] >= np.maximum(o["open"], o["close"])) and np.all(o["low"] <= np.minimum(o["open"], o["close"]))
    nz = o["trades"] > 0
    assert np.all((o["vwap"][nz] >= o["low"][nz] - 1e-9) & (o["vwap"][nz] <= o["high"][nz] + 1e-9))
    assert np.all(o["median_trade_size"][nz] >= 2.0 ** -10) and np.all(o["median_trade_size"][nz] <= 4.0)
    # --- conservation across granularities.  Dyadic amounts (multiples of 2^-10): a float32 bar volume is
    #     exact while the bar holds < 2^24 quanta, i.e. for 1-minute and 5-minute bars (not for daily ones).
    _, ci_5m = t.time_bar_index(300.0)
    o_5m = engine.to_host(t.bar_ohlcv(ci_5m, want_median=False))
    assert o["volume"].astype(np.float64).sum() == o_5m["volume"].astype(np.float64).sum()
    _, ci_day = t.time_bar_index(86400.0)            # long bars: generic streaming kernel
    o_day = engine.to_host(t.bar_ohlcv(ci_day, want_median=True))
    assert o_day["trades"].sum() == o["trades"].sum() == o_5m["trades"].sum()
    assert o["high"].max() == o_day["high"].max() == o_5m["high"].max()
    assert o["low"].min() == o_day["low"].min()
    np.testing.assert_allclose(o_day["volume"].astype(np.float64).sum(), o["volume"].astype(np.float64).sum(), rtol=1e-6)
    assert np.all((o_day["median_trade_size"] > 1.9) & (o_day["median_trade_size"] < 2.1))   # uniform on (0, 4]
    # --- prefix parity: bars closing inside the first PREFIX ticks == oracle on those ticks alone
    oclk, oci = orc._time_bar_indexer(ts, 60.0)
    k = int(np.searchsorted(cih, PREFIX - 1, side="left")) - 1        # bars fully inside the prefix
    assert k > 1000
    np.testing.assert_array_equal(cih[:k + 1], oci[:k + 1])
    want = orc.comp_bar_ohlcv(px, am, oci[:k + 1])
    for key, w in zip(["open", "high", "low", "close", "volume", "vwap", "trades", "median_trade_size"], want):
        if key == "vwap":
            G.assert_f64_close(o[key][:k], w, rtol=1e-9, what="vwap")
        else:
            np.testing.assert_array_equal(o[key][:k], w, err_msg=key)


def test_directional_and_footprints_full_size(big, prefix, orc):
    engine, t, n = big
    ts, px, am, sd = prefix
    _, ci = t.time_bar_index(60.0)
    cih = ci.to_host()
    o = t.bar_ohlcv(ci, want_median=False)
    d, nz = t.bar_directional(ci)
    d = engine.to_host(d)
    assert int(nz.to_host()[0]) == 0
    trades = np.diff(cih)
    assert np.array_equal(d["ticks_buy"] + d["ticks_sell"], trades)                     # every tick is signed
    vol = o["volume"].to_host().astype(np.float64)
    assert np.array_equal(d["volume_buy"].astype(np.float64) + d["volume_sell"].astype(np.float64), vol)   # exact dyadic
    assert np.all(d["cum_ticks_max"] >= d["cum_ticks_min"]) and np.all(np.abs(d["cum_ticks_max"]) <= trades)
    off, flat, bar, bad = t.bar_footprints(ci, o["low"], o["high"], 0.01, 3.0)
    assert int(bad.to_host()[0]) == 0
    offh = off.to_host()
    bt, st = flat["buy_ticks"].to_host(), flat["sell_ticks"].to_host()
    bv, sv = flat["buy_volumes"].to_host(), flat["sell_volumes"].to_host()
    seg = np.add.reduceat
    starts = offh[:-1]
    assert np.array_equal(seg(bt.astype(np.int64), starts), d["ticks_buy"])            # rows vs bar totals
    assert np.array_equal(seg(st.astype(np.int64), starts), d["ticks_sell"])
    assert np.array_equal(seg(bv.astype(np.float64), starts), d["volume_buy"].astype(np.float64))
    assert np.array_equal(seg(sv.astype(np.float64), starts), d["volume_sell"].astype(np.float64))
    lv = flat["price_levels"].to_host()
    lows = np.rint(o["low"].to_host() / 0.01).astype(np.int64)
    highs = np.rint(o["high"].to_host() / 0.01).astype(np.int64)
    assert np.array_equal(lv[starts], lows) and np.array_equal(lv[offh[1:] - 1], highs)
    g = bar["vp_gini"].to_host()
    assert np.all((g >= 0) & (g < 1))
    # --- prefix parity
    _, oci = orc._time_bar_indexer(ts, 60.0)
    k = int(np.searchsorted(cih, PREFIX - 1, side="left")) - 1
    want = orc.comp_bar_directional_features(px, am, oci[:k + 1], sd)
    for key, w in zip(G.DIR_KEYS, want):
        # bar 0 starts at tick 0: its spread terms use the reference's wrap-around tick prices[-1], which is
        # the LAST tick of whatever array is passed (1e9 ticks here, the prefix in the oracle) -> skip bar 0
        np.testing.assert_array_equal(d[key][1:k], w[1:], err_msg=key)          # float32 columns bit-identical too
    oo = orc.comp_bar_ohlcv(px, am, oci[:k + 1], want_median=False)
    woff, wflat, wbar = orc.comp_bar_footprints_csr(px, am, oci[:k + 1], sd, 0.01, oo[2], oo[1], 3.0)
    np.testing.assert_array_equal(offh[:k + 1], woff)
    for key in G.FP_LIST_KEYS:
        np.testing.assert_array_equal(flat[key].to_host()[:woff[-1]].astype(wflat[key].dtype), wflat[key], err_msg=key)
    for key in ("buy_imbalances_sum", "sell_imbalances_sum", "cot_price_levels", "imb_max_run_signed", "vp_gini"):
        np.testing.assert_array_equal(bar[key].to_host()[:k], wbar[key], err_msg=key)


def test_cfg1_reference_vectors_at_full_size(big):
    """BASELINE cfg 1 + cfg 2 tied together: the first bars of the 10^9-tick HIP run against the vectors the REFERENCE's
    own `TimeBarKit(60 s).build_ohlcv()` produced from the first 10^7 ticks of the same stream (oracle/gen_cfg1.py,
    tests/golden/cfg1_reference_timebars.npz) -- directly, no oracle in between.  All bars but the reference run's last
    (which closes on that run's final, partial minute) consist of the same ticks in both runs.  Indices, counts, OHLC,
    median and the float32 volume bit-exact; vwap <= 1e-9 relative (tree-ordered float64 sum)."""
    engine, t, n = big
    d = G.load("cfg1_reference_timebars")
    assert n >= int(d["n_ohlcv"])
    clock, ci = t.time_bar_index(60.0)
    k = len(d["close_indices"]) - 2                                      # complete bars of the 10^7-tick run: 8330
    assert k == 8330
    np.testing.assert_array_equal(ci.view(0, k + 1).to_host(), d["close_indices"][:k + 1])
    np.testing.assert_array_equal(clock.view(0, k + 1).to_host(), d["close_ts"][:k + 1])
    o = t.bar_ohlcv(ci)
    for key in ("open", "high", "low", "close", "volume", "trades", "median_trade_size"):
        got, want = o[key].view(0, k).to_host(), d["ohlcv_col_" + key][:k]
        assert got.dtype == want.dtype, key
        np.testing.assert_array_equal(got, want, err_msg=key)
    G.assert_f64_close(o["vwap"].view(0, k).to_host(), d["ohlcv_col_vwap"][:k], rtol=1e-9, what="vwap")
    # order-flow + footprints (the reference's build_directional_features / build_footprints on the first 10^6 ticks)
    kf = len(d["flow_close_indices"]) - 2
    cif = ci.view(0, kf + 1)
    dd, nz = t.bar_directional(cif)
    for name in (str(c) for c in d["dir_columns"]):
        mine = {"cum_volume_min": "cum_volumes_min", "cum_volume_max": "cum_volumes_max"}.get(name, name)
        got, want = dd[mine].to_host(), d["dir_col_" + name][:kf]
        if name in ("mean_spread", "max_spread"):                       # bar 0: wrap-around tick prices[-1]
            got, want = got[1:], want[1:]
        assert got.dtype == want.dtype, name
        np.testing.assert_array_equal(got, want, err_msg=name)
    off, flat, bar, bad = t.bar_footprints(cif, o["low"].view(0, kf), o["high"].view(0, kf), 0.01, 3.0)
    assert int(bad.to_host()[0]) == 0
    offh = off.to_host()
    np.testing.assert_array_equal(np.diff(offh), d["fp_n_levels"][:kf])
    nl = int(offh[-1])
    for key in G.FP_LIST_KEYS:
        want = d["fp_" + key][:nl]
        np.testing.assert_array_equal(flat[key].to_host().astype(want.dtype), want, err_msg=key)
    for key in ("buy_imbalances_sum", "sell_imbalances_sum", "cot_price_levels", "imb_max_run_signed", "vp_gini"):
        np.testing.assert_array_equal(bar[key].to_host(), d["fp_" + key][:kf], err_msg=key)
    np.testing.assert_allclose(bar["vp_skew"].to_host(), d["fp_vp_skew"][:kf], atol=1e-6)


def test_threshold_bars_full_size(big, prefix, orc):
    engine, t, n = big
    ts, px, am, sd = prefix
    vthr = 1728.5                     # ~864 ticks per bar (median daily volume / 2000 of this stream)
    dthr = vthr * 10_000.0
    # Both in the library's DEFAULT (exact) mode.  Volume bars: fragile decisions are settled by replaying their bar.  Dollar
    # bars: ~230 of the 1.16e6 closes fall inside the rounding drift of the reference's float64 running sum (which never
    # resets); the exact tier (csrc/fmk_dollar_exact.hip) reconstructs that running sum's state at every bar start and
    # replays the ~0.3 % of the bars that need it -- n_uncertified comes back 0 at GPU speed (the serial walk took 15-22 s).
    _threshold_bars_full_size(engine, t, n, px, am, orc, vthr, dthr, ("volume", "dollar"))
    # the closed form alone (fast mode) still reports its count, and on this stream none of the reported decisions differs
    t.ctx.set_fast_threshold(True)
    try:
        fast = t.dollar_bar_index(dthr).to_host()
        assert t.last_uncertified > 0 or n < 10**8
    finally:
        t.ctx.set_fast_threshold(False)
    exact = t.dollar_bar_index(dthr).to_host()
    assert t.last_uncertified == 0 and len(exact) == len(fast)
    print(f"dollar bars at {n:.3g} ticks: {int((exact != fast).sum())} closes differ between the exact tier and the closed form")


def test_cfg3_reference_vectors(big, monkeypatch):
    """cfg 3 against vectors the REFERENCE's own sequential indexers made (oracle/gen_cfg1.py): the closes of the 10^9-tick HIP
    run that fall inside the first 10^7 ticks (threshold bars are causal), and the lognormal float64 tape in full -- default exact
    mode, and the dollar tape once more forced through the exact tier with a wide margin (most bars replayed)."""
    engine, t, n = big
    d = G.load("cfg1_reference_timebars")
    m = int(d["n_ohlcv"])
    assert n >= m
    for kind, thr, key in (("volume", float(d["cfg3_vthr"]), "cfg3_volume_close_indices"),
                           ("dollar", float(d["cfg3_dthr"]), "cfg3_dollar_close_indices")):
        ci = (t.volume_bar_index(thr) if kind == "volume" else t.dollar_bar_index(thr)).to_host()
        assert t.last_uncertified == 0
        k = int(np.searchsorted(ci, m, side="left"))
        np.testing.assert_array_equal(ci[:k], d[key], err_msg=kind)
    lam, lpx = G.lognormal_tape(d)
    tape = engine.DeviceTrades.from_numpy(np.arange(len(lam), dtype=np.int64), lpx, lam)
    np.testing.assert_array_equal(tape.volume_bar_index(float(d["cfg3_logn_vthr"])).to_host(), d["cfg3_logn_volume_close_indices"])
    np.testing.assert_array_equal(tape.dollar_bar_index(float(d["cfg3_logn_dthr"])).to_host(), d["cfg3_logn_dollar_close_indices"])
    monkeypatch.setenv("FMK_DL_FORCE_EXACT_TIER", "1")
    monkeypatch.setenv("FMK_DL_MARGIN_SCALE", "1e6")
    np.testing.assert_array_equal(tape.dollar_bar_index(float(d["cfg3_logn_dthr"])).to_host(), d["cfg3_logn_dollar_close_indices"])
    assert tape.last_uncertified == 0


def _threshold_bars_full_size(engine, t, n, px, am, orc, vthr, dthr, kinds):
    for kind in kinds:
        ci = (t.volume_bar_index(vthr) if kind == "volume" else t.dollar_bar_index(dthr)).to_host()
        want = orc._volume_bar_indexer(am, vthr) if kind == "volume" else orc._dollar_bar_indexer(px, am, dthr)
        assert ci[0] == 0 and np.all(np.diff(ci) > 0) and ci[-1] < n
        # causal: the closes inside the prefix are exactly the oracle's closes on the prefix
        k = int(np.searchsorted(ci, PREFIX, side="left"))
        np.testing.assert_array_equal(ci[:k], want, err_msg=kind)
        assert t.last_uncertified == 0
        if kind == "volume":
            o = engine.to_host(t.bar_ohlcv(engine.DeviceArray.from_host(t.ctx, ci), want_median=False))
            v = o["volume"].astype(np.float64)
            assert np.all(v >= vthr - 4.0) and np.all(v < vthr + 4.0)       # reset bars: thr <= vol(+tick 0 rule) < thr + max tick


def test_cusum_and_volume_profile_full_size(big, prefix, orc, monkeypatch):
    """The "next" rows at 1e9 ticks: CUSUM closes are causal (prefix parity with the sequential oracle on the same
    sigma) and, with thresholds reached every ~200 ticks, come from the one-pass form (csrc/fmk_cusum_onepass.h) and equal the
    fixed point's over the whole stream; the rolling volume profile satisfies its ordering invariants on 8e5 bars and equals
    the oracle on a prefix."""
    import ctypes as C
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64
    engine, t, n = big
    ts, px, am, sd = prefix
    r = t.lagged_returns(5.0, True)
    sg = t.ewmst(r, 60.0)
    del r
    sigma_prefix = sg.view(0, PREFIX).to_host()
    m, rounds = c_i64(), c_i64()
    t.ctx.call("fmk_cusum_bar_indexer_dev", t.ts.p, t.price.p, sg.p, c_i64(n), c_f64(1e-5), c_f64(2.0), None, c_i64(0),
               C.byref(m), C.byref(rounds))
    out = DeviceArray(t.ctx, m.value, np.int64)
    t.ctx.call("fmk_cusum_bar_indexer_dev", t.ts.p, t.price.p, sg.p, c_i64(n), c_f64(1e-5), c_f64(2.0), out.p,
               c_i64(m.value), C.byref(m), C.byref(rounds))
    ci = out.to_host()
    used, launches, pending, chunks = (c_i64() for _ in range(4))
    _ffi.lib().fmk_diag_cusum_onepass(C.byref(used), C.byref(launches), C.byref(pending), C.byref(chunks))
    if n >= 100_000_000:
        assert used.value == 1 and launches.value <= 8, (used.value, launches.value, pending.value, chunks.value)
    monkeypatch.setenv("FMK_CUSUM_ONEPASS", "0")                     # the fixed point on chunk-transposed copies (rounds 1-4)
    m2 = c_i64()
    t.ctx.call("fmk_cusum_bar_indexer_dev", t.ts.p, t.price.p, sg.p, c_i64(n), c_f64(1e-5), c_f64(2.0), out.p,
               c_i64(out.n), C.byref(m2), C.byref(rounds))
    _ffi.lib().fmk_diag_cusum_onepass(C.byref(used), None, None, None)
    assert used.value == 0 and m2.value == m.value
    np.testing.assert_array_equal(out.to_host(), ci)
    monkeypatch.delenv("FMK_CUSUM_ONEPASS")
    del sg, out
    assert rounds.value <= 16 and np.all(np.diff(ci) > 0) and ci[-1] < n
    want = orc._cusum_bar_indexer(ts, px, sigma_prefix, 1e-5, 2.0)
    k = int(np.searchsorted(ci, PREFIX - 1, side="left"))           # the tick PREFIX-1 has no successor in the prefix run
    assert k > 1000
    np.testing.assert_array_equal(ci[:k], want[:k])
    # ---- rolling volume profile over all one-minute bars
    clock, cid = t.time_bar_index(60.0)
    o, d, nz, off, flat, bar, bad = t.bars_fused(cid, 0.01, 3.0, want_median=False)
    nb = cid.n - 1
    bts = clock.view(1, nb)
    window_ns = 1800 * 10**9
    first = int(np.searchsorted(bts.to_host(), int(bts.view(0, 1).to_host()[0]) + window_ns))
    outs = [DeviceArray(t.ctx, nb, np.int32) for _ in range(3)] + [DeviceArray(t.ctx, nb, np.float32)]
    t.ctx.call("fmk_volume_profile_rolling_dev", bts.p, o["high"].p, o["low"].p, off.p, flat["price_levels"].p,
               flat["buy_volumes"].p, flat["sell_volumes"].p, c_i64(nb), c_i64(first), c_i64(window_ns), c_i64(27),
               c_f64(0.01), c_f64(68.34), *[x.p for x in outs])
    poc, hva, lva, pct = (x.to_host() for x in outs)
    assert np.all(poc[:first] == 0) and np.all(poc[first:] > 0)
    assert np.all(lva[first:] <= poc[first:]) and np.all(poc[first:] <= hva[first:])
    assert np.all((pct >= 0) & (pct <= 1))
    kb = 2000                                                          # oracle on the first 2000 bars (causal windows)
    offh = off.view(0, kb + 1).to_host()
    nl = int(offh[-1])
    w = orc.volume_profile_rolling(bts.view(0, kb).to_host(), o["high"].view(0, kb).to_host(), o["low"].view(0, kb).to_host(),
                                   offh, flat["price_levels"].view(0, nl).to_host(), flat["buy_volumes"].view(0, nl).to_host(),
                                   flat["sell_volumes"].view(0, nl).to_host(), 1800.0, 27, 0.01, 68.34)
    for g, ww, name in zip((poc, hva, lva, pct), w, ("poc", "hva", "lva", "pct")):
        np.testing.assert_array_equal(g[:kb], ww, err_msg=name)


def test_cusum_default_floor_chain_walk_equals_fixed_point(big, prefix, orc, monkeypatch):
    """CUSUMBarKit's default sigma_floor (5e-4; kit.py:147) on the 1e9-tick tape: a close per ~2.4e5 ticks, served by the
    chain walk of fmk_cusum_chain.hip.  Its closes are those of the fixed point (the reference's loop operation for
    operation: 0.3 s here) at two floors, and on the prefix those of the sequential oracle."""
    import ctypes as C
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray, c_f64, c_i64
    engine, t, n = big
    ts, px, am, sd = prefix
    r = t.lagged_returns(5.0, True)
    sg = t.ewmst(r, 60.0)
    del r
    out = DeviceArray(t.ctx, 1 << 20, np.int64)
    m, rounds, tier, opened, status = c_i64(), c_i64(), c_i64(), c_i64(), c_i64()

    def run(floor):
        t.ctx.call("fmk_cusum_bar_indexer_dev", t.ts.p, t.price.p, sg.p, c_i64(n), c_f64(floor), c_f64(2.0), out.p,
                   c_i64(out.n), C.byref(m), C.byref(rounds))
        _ffi.lib().fmk_diag_cusum_last(C.byref(tier), C.byref(opened), C.byref(status))
        return out.view(0, m.value).to_host().copy(), tier.value

    for floor in (5e-4, 3e-4):
        monkeypatch.setenv("FMK_CUSUM_CHAIN", "1")
        got, used = run(floor)
        if n >= 100_000_000:
            assert used == 1, "the chain walk should serve this regime"
        monkeypatch.setenv("FMK_CUSUM_CHAIN", "0")
        want, used0 = run(floor)
        assert used0 == 0
        np.testing.assert_array_equal(got, want)
        assert len(got) > n // 1_000_000
    sigma_prefix = sg.view(0, PREFIX).to_host()
    seq = orc._cusum_bar_indexer(ts, px, sigma_prefix, 3e-4, 2.0)
    k = int(np.searchsorted(got, PREFIX - 1, side="left"))
    assert k > 10
    np.testing.assert_array_equal(got[:k], seq[:k])


def test_one_second_bars_full_size(big, prefix, orc):
    """TimeBarKit(1 s) -- the reference's other caller (io.py:484) -- at 1e9 ticks: 5e7 bars of ~20 ticks.  The library takes its
    lane-per-bar schedules here on its own (k_bar_ohlcv_lanes, k_bar_dir_lanes, k_bar_footprints_lanes + the wave kernels for the
    bars they list); the outputs satisfy the row-sum identities over all bars and equal the oracle on the prefix, bit for bit."""
    engine, t, n = big
    ts, px, am, sd = prefix
    _, ci = t.time_bar_index(1.0)
    cih = ci.to_host()
    o = t.bar_ohlcv(ci)
    d, nz = t.bar_directional(ci)
    d = engine.to_host(d)
    trades = np.diff(cih)
    assert int(nz.to_host()[0]) == int((trades == 0).sum())               # empty seconds: no signed tick
    assert np.array_equal(d["ticks_buy"] + d["ticks_sell"], trades)
    assert np.array_equal(o["trades"].to_host(), trades)
    off, flat, bar, bad = t.bar_footprints(ci, o["low"], o["high"], 0.01, 3.0)
    assert int(bad.to_host()[0]) == 0
    offh = off.to_host()
    starts = offh[:-1]
    has = np.diff(offh) > 0
    bt = np.add.reduceat(flat["buy_ticks"].to_host().astype(np.int64), np.minimum(starts, offh[-1] - 1))
    assert np.array_equal(bt[has], d["ticks_buy"][has])
    # --- prefix parity with the oracle
    _, oci = orc._time_bar_indexer(ts, 1.0)
    k = int(np.searchsorted(cih, PREFIX - 1, side="left")) - 1
    assert k > 100_000
    oo = orc.comp_bar_ohlcv(px, am, oci[:k + 1])
    for key, w in zip(G.OHLCV_KEYS, oo):
        got = o[{"median": "median_trade_size"}.get(key, key)].to_host()[:k]
        if key == "vwap":
            G.assert_f64_close(got, w, what="vwap")
        else:
            np.testing.assert_array_equal(got, w, err_msg=key)
    want = orc.comp_bar_directional_features(px, am, oci[:k + 1], sd, raise_on_zero_div=False)
    for key, w in zip(G.DIR_KEYS, want):
        np.testing.assert_array_equal(d[key][1:k], w[1:], err_msg=key)    # bar 0: the wrap-around tick differs (see above)
    woff, wflat, wbar = orc.comp_bar_footprints_csr(px, am, oci[:k + 1], sd, 0.01, oo[2], oo[1], 3.0)
    np.testing.assert_array_equal(offh[:k + 1], woff)
    for key in G.FP_LIST_KEYS:
        np.testing.assert_array_equal(flat[key].view(0, int(woff[-1])).to_host().astype(wflat[key].dtype), wflat[key], err_msg=key)
    for key in ("buy_imbalances_sum", "sell_imbalances_sum", "cot_price_levels", "imb_max_run_signed", "vp_gini"):
        np.testing.assert_array_equal(bar[key].view(0, k).to_host(), wbar[key], err_msg=key)


def test_cfg4_first_half_lane_schedule_full_size(big, prefix, orc):
    """cfg 4 at 1e9 ticks, 1-minute bars: bars_fused takes k_bar_dir_lanes<OHLC> + the median-only kernel on its own.  Its OHLCV
    equals build_ohlcv's (vwap to 1e-9: the lane adds in the reference's tick order, the wave kernel as a tree), its order-flow
    columns the standalone reducer's, and everything the oracle's on the prefix."""
    engine, t, n = big
    ts, px, am, sd = prefix
    _, ci = t.time_bar_index(60.0)
    cih = ci.to_host()
    o, d, nz, off, flat, bar, bad = t.bars_fused(ci, 0.01, 3.0)
    o, d = engine.to_host(o), engine.to_host(d)
    o2 = engine.to_host(t.bar_ohlcv(ci))
    for k in o2:
        if k == "vwap":
            G.assert_f64_close(o[k], o2[k], what="vwap fused vs build_ohlcv")
        else:
            np.testing.assert_array_equal(o[k], o2[k], err_msg=k)
    d2, _ = t.bar_directional(ci)
    for k, v in engine.to_host(d2).items():
        np.testing.assert_array_equal(d[k], v, err_msg=k)
    _, oci = orc._time_bar_indexer(ts, 60.0)
    k = int(np.searchsorted(cih, PREFIX - 1, side="left")) - 1
    want = orc.comp_bar_ohlcv(px, am, oci[:k + 1])
    for key, w in zip(["open", "high", "low", "close", "volume", "vwap", "trades", "median_trade_size"], want):
        if key == "vwap":
            G.assert_f64_close(o[key][:k], w, what="vwap")
        else:
            np.testing.assert_array_equal(o[key][:k], w, err_msg=key)


# ---------------------------------------------------------------------------------------------------------------------------
# every bar of the full-size run against the threaded oracle (VERDICT r2 next #2a)
# ---------------------------------------------------------------------------------------------------------------------------
def _mem_available_bytes():
    try:
        with open("/proc/meminfo") as fh:
            for ln in fh:
                if ln.startswith("MemAvailable:"):
                    return int(ln.split()[1]) * 1024
    except OSError:
        pass
    return 16 << 30


@pytest.fixture(scope="module")
def host_cols(big):
    """The device columns on the host: ALL n ticks.  A host too small for columns + oracle outputs + HIP outputs (~60 B/tick all
    told, in a third of the available memory) FAILS the all-bars tests instead of silently comparing a prefix; FMK_FULLSIZE_TICKS=<n>:prefix
    (developer boxes) brings the prefix comparison back, and gpu_parity_counts.json says how much was compared either way."""
    engine, t, n = big
    m = min(n, int(_mem_available_bytes() / 3 // 60))
    if m < n and not os.environ.get("FMK_FULLSIZE_TICKS", "").endswith(":prefix"):
        pytest.fail(f"host memory holds {m:.3g} of the {n:.3g} ticks: the all-bars tests would compare a prefix only "
                    "(FMK_FULLSIZE_TICKS=<n>:prefix to allow that)")
    cores = len(os.sched_getaffinity(0))
    os.environ["ORC_THREADS"] = str(cores)
    cols = tuple(None if c is None else c.view(0, m).to_host() for c in (t.ts, t.price, t.amount, t.side))
    yield cols, m
    os.environ.pop("ORC_THREADS", None)


def _bars_inside(cih, m, n):
    """Number of leading bars whose ticks all lie inside the first m ticks (all of them when m == n)."""
    return len(cih) - 1 if m == n else int(np.searchsorted(cih, m - 1, side="left")) - 1


def test_all_bars_cfg2_against_threaded_oracle(big, host_cols, orc):
    import time
    engine, t, n = big
    (ts, px, am, sd), m = host_cols
    clock, ci = t.time_bar_index(60.0)
    cih, clk = ci.to_host(), clock.to_host()
    t0 = time.perf_counter()
    oclk, oci = orc._time_bar_indexer(ts, 60.0)
    k = _bars_inside(cih, m, n)
    assert k > 1000 and (m < n or k == len(oci) - 1)
    np.testing.assert_array_equal(cih[:k + 1], oci[:k + 1])
    np.testing.assert_array_equal(clk[:k + 1], oclk[:k + 1])
    want = orc.comp_bar_ohlcv(px, am, oci[:k + 1])
    dt = time.perf_counter() - t0
    o = engine.to_host(t.bar_ohlcv(ci))
    for key, w in zip(["open", "high", "low", "close", "volume", "vwap", "trades", "median_trade_size"], want):
        assert o[key].dtype == w.dtype, key
        if key == "vwap":
            G.assert_f64_close(o[key][:k], w, rtol=1e-9, what="vwap")
        else:
            np.testing.assert_array_equal(o[key][:k], w, err_msg=key)
    print(f"cfg 2: {k} of {len(cih) - 1} bars ({m:.3g} of {n:.3g} ticks) equal the oracle's; oracle {dt:.1f} s on "
          f"{os.environ['ORC_THREADS']} threads")
    record("cfg2_time_bars_ohlcv_median", ticks_compared=m, ticks_total=n, bars_compared=k, bars_total=len(cih) - 1,
           edges_compared=k + 1)
    # cfg 3 on the same columns: the reference's sequential loops (one thread, ~1 ns/tick) against the exact default mode
    vthr, dthr = 1728.5, 17_285_000.0
    for kind, got, w in (("volume", t.volume_bar_index(vthr).to_host(), orc._volume_bar_indexer(am, vthr)),
                         ("dollar", t.dollar_bar_index(dthr).to_host(), orc._dollar_bar_indexer(px, am, dthr))):
        kk = len(got) if m == n else int(np.searchsorted(got, m, side="left"))
        np.testing.assert_array_equal(got[:kk], w[:kk] if m == n else w, err_msg=kind)
        assert m < n or len(got) == len(w)
        print(f"cfg 3 {kind}: {kk} closes equal the sequential loop's")
        record(f"cfg3_{kind}_bar_closes", ticks_compared=m, ticks_total=n, closes_compared=kk, closes_total=len(got))


def test_all_bars_cfg4_against_threaded_oracle(big, host_cols, orc):
    # the bench tape's one-minute bars (~1 200 ticks, dyadic sizes) take the one pass with the unit histogram by default
    _cfg4_all_bars(big, host_cols, orc, 60.0, expect_mode=1)


@pytest.mark.parametrize("interval", [3600.0, 86400.0])
def test_all_long_bars_cfg4_against_threaded_oracle(big, host_cols, orc, interval):
    """... and on hourly / daily bars: the workgroup-per-bar schedules (order flow with its tick-order redo, footprints on one LDS
    histogram, OHLCV + sample-bracket median) on ALL bars of the full-size run."""
    _cfg4_all_bars(big, host_cols, orc, interval)


@pytest.mark.parametrize("interval", [60.0, 3600.0])
def test_all_bars_cfg4_full_mantissa_sizes_against_threaded_oracle(big, host_cols, orc, interval):
    """... and with FULL-MANTISSA float32 sizes (what real trade sizes are): every footprint bar then takes the tick-ordered path and
    the order-flow sums sit in the float32 tie zone far more often -- all bars of the full-size run again."""
    import ctypes as C
    engine, t, n = big
    from finmlkit_amd._ffi import DeviceArray, c_i64
    am2 = DeviceArray(t.ctx, n, np.float32)
    t.ctx.call("fmk_diag_fill_amounts_dev", C.c_uint64(42), c_i64(n), am2.p)
    t2 = engine.DeviceTrades(t.ctx, t.ts, t.price, am2, t.side)
    (ts, px, am, sd), m = host_cols
    # (one-minute bars: a mean below 1 250 ticks, where the one pass without the unit histogram does not pay -- the two-pass schedules)
    _cfg4_all_bars((engine, t2, n), ((ts, px, am2.view(0, m).to_host(), sd), m), orc, interval, tag="full_mantissa_sizes",
                   expect_mode=0 if interval == 60.0 else None)


def test_all_bars_cfg4_lognormal_full_mantissa_against_threaded_oracle(big, host_cols, orc):
    """... and the primary cfg 4 figure of bench.py: bars of lognormal length (mean 1 200 ticks, sigma 1: what real one-minute bars look
    like) on full-mantissa sizes -- the length census sends it to the two-pass schedules (sorted lanes, comp_bar_ohlcv's size classes,
    the long-bar kernels); all bars of the full-size run again."""
    import ctypes as C
    engine, t, n = big
    from finmlkit_amd._ffi import DeviceArray, c_i64
    am2 = DeviceArray(t.ctx, n, np.float32)
    t.ctx.call("fmk_diag_fill_amounts_dev", C.c_uint64(42), c_i64(n), am2.p)
    t2 = engine.DeviceTrades(t.ctx, t.ts, t.price, am2, t.side)
    rng = np.random.default_rng(7)                        # bench.py's bar lengths (seed 7), rebuilt here
    lens = np.maximum(1, rng.lognormal(np.log(1200.0) - 0.5, 1.0, int(n / 1200 * 1.3)).astype(np.int64))
    cih = np.concatenate([[-1], np.cumsum(lens) - 1])
    cih = cih[cih <= n - 1].astype(np.int64)
    (ts, px, am, sd), m = host_cols
    _cfg4_all_bars((engine, t2, n), ((ts, px, am2.view(0, m).to_host(), sd), m), orc, None, tag="full_mantissa_sizes",
                   ci=DeviceArray.from_host(t.ctx, cih), count_key="cfg4_full_mantissa_sizes_lognormal_bars", expect_mode=0)


def _cfg4_all_bars(big, host_cols, orc, interval, tag="dyadic_sizes", ci=None, count_key=None, expect_mode=None):
    """cfg 4 on all bars of the full-size run: time bars of `interval` seconds, or the close indices `ci` (a DeviceArray), recorded as
    `count_key`; expect_mode: the schedule the sizing call must take (fmk_diag_fused_mode)."""
    import time
    from tests.test_gpu_fused import fused_mode
    engine, t, n = big
    (ts, px, am, sd), m = host_cols
    if ci is None:
        _, ci = t.time_bar_index(interval)
    cih = ci.to_host()
    k = _bars_inside(cih, m, n)
    oci = cih[:k + 1]
    o, d, nz, off, flat, bar, bad = t.bars_fused(ci, 0.01, 3.0, want_median=True)
    mode = fused_mode(t.ctx)
    assert int(bad.to_host()[0]) == 0 and int(nz.to_host()[0]) == 0
    if expect_mode is not None:
        assert mode[0] == expect_mode, f"cfg 4 took schedule {mode[0]}, expected {expect_mode}"
        assert mode[1] == (expect_mode == 1)      # the fill consumed the staged rows exactly when the one pass staged them
    t0 = time.perf_counter()
    want_d = orc.comp_bar_directional_features(px, am, oci, sd)
    oo = orc.comp_bar_ohlcv(px, am, oci, want_median=True)
    woff, wflat, wbar = orc.comp_bar_footprints_csr(px, am, oci, sd, 0.01, oo[2], oo[1], 3.0)
    dt = time.perf_counter() - t0
    lo = 0 if m == n else 1        # bar 0's spread uses prices[-1] = the last tick of the array passed (base.py:485-500)
    for key, w in zip(G.DIR_KEYS, want_d):
        got = d[key].to_host()
        assert got.dtype == w.dtype, key
        a = lo if key in ("mean_spread", "max_spread") else 0
        np.testing.assert_array_equal(got[a:k], w[a:], err_msg=key)
    for key, w in zip(["open", "high", "low", "close", "volume", "vwap", "trades", "median_trade_size"], oo):
        got = o[key].to_host()
        if key == "vwap":
            G.assert_f64_close(got[:k], w, rtol=1e-9, what="vwap")
        else:
            np.testing.assert_array_equal(got[:k], w, err_msg=key)
    offh = off.to_host()
    np.testing.assert_array_equal(offh[:k + 1], woff)
    nl = int(woff[-1])
    for key in G.FP_LIST_KEYS:
        np.testing.assert_array_equal(flat[key].view(0, nl).to_host().astype(wflat[key].dtype), wflat[key], err_msg=key)
    for key in ("buy_imbalances_sum", "sell_imbalances_sum", "cot_price_levels", "imb_max_run_signed", "vp_gini"):
        np.testing.assert_array_equal(bar[key].to_host()[:k], wbar[key], err_msg=key)
    np.testing.assert_allclose(bar["vp_skew"].to_host()[:k], wbar["vp_skew"], atol=1e-6)
    count_key = count_key or f"cfg4_{tag}_{interval:.0f}s_bars"
    print(f"{count_key}: {k} bars, {nl} footprint levels equal the oracle's; oracle {dt:.1f} s")
    record(count_key, ticks_compared=m, ticks_total=n, bars_compared=k, bars_total=len(cih) - 1,
           footprint_levels_compared=nl)


@pytest.mark.parametrize("interval", [60.0, 150.0, 600.0, 1200.0, 1500.0, 3600.0])
def test_all_bars_trade_size_against_threaded_oracle(big, host_cols, orc, interval):
    """comp_bar_trade_size_features of ALL bars at full size against the oracle (its bar loop on all host cores): 1-minute bars (one
    wave reading the bar once), 150-second bars (one wave with five tree levels / two waves), 10-minute bars (eight waves on two of
    np.sum's chunks), 20- and 25-minute bars (sixteen waves on three / four chunks, or the sub-tree workgroup where the last chunk does
    not fit), hourly bars (the sub-tree workgroup, sample-bracket percentile) -- every column bit for bit."""
    import time
    engine, t, n = big
    (ts, px, am, sd), m = host_cols
    _, ci = t.time_bar_index(interval)
    cih = ci.to_host()
    k = _bars_inside(cih, m, n)
    assert k >= 100
    theta_d = t.bar_ohlcv(ci)["median_trade_size"]
    theta = theta_d.to_host()
    got = t.bar_trade_size(ci, theta, 5.0)
    t0 = time.perf_counter()
    want = orc.comp_bar_trade_size_features(am, theta[:k], cih[:k + 1], 5.0)
    dt = time.perf_counter() - t0
    for key, w in zip(["mean_size_rel", "size_95_rel", "pct_block", "size_gini"], want):
        np.testing.assert_array_equal(got[key][:k], w, err_msg=f"{key} interval {interval}")
    print(f"trade size, {interval:.0f} s bars: {k} bars equal the oracle's; oracle {dt:.1f} s")
    record(f"trade_size_{interval:.0f}s_bars", ticks_compared=m, ticks_total=n, bars_compared=k, bars_total=len(cih) - 1)
