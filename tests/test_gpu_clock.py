"""The bar-clock, run-length and opening-range features on the MI355X -- bar_duration, bar_duration_ewma, bar_rate, dir_run_len,
orb_break (csrc/fmk_clock.hip, csrc/fmk_lasthead.h) -- against the untouched reference's recorded outputs (tests/golden/clock.npz,
tools/gen_clock_golden.py) and, on seeded tapes, against the NumPy restatement that the generator held against the reference
(tests/_clock_ref.py).  The host-pointer entries, the `_dev` entries, the `DeviceTrades` methods, the transforms and the transforms
under `Compose`.

Bit for bit: bar_duration, bar_rate, dir_run_len, orb_break.  bar_duration_ewma: its NaN exactly and within 1e-9 relative, the
project's contract for recurrence scans (the restatement itself lies within 1.8e-15 of pandas: clock.json, dew_ref_dev).  The host
and the `_dev` flavour of every feature give identical bits.  The sizes come from the kernels' own constants (clock.geometry())."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from tests import _clock_ref as H
from tests import _counts
from tests.test_clock_host import MANIFEST, expected, product

pytestmark = pytest.mark.gpu

HOST = {"dur": "bar_duration", "dew": "bar_duration_ewma", "rate": "bar_rate", "run": "dir_run_len", "orb": "orb_break"}
WORST = {"dew": 0.0}


def geo():
    return product().geometry()


def check(fn, got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype == np.uint8 and w.dtype == np.bool_:
            g = g.view(np.bool_)
        if H.EXACT[fn]:
            if not H.same_bits(g, w):
                bad = np.flatnonzero(~((g == w) | ((g != g) & (w != w)))) if g.shape == w.shape else "shape"
                raise AssertionError((what, k, g.dtype, w.dtype, bad[:5], g[bad[:3]], w[bad[:3]]))
        else:
            dev = H.dew_deviation(g, w)
            print(f"deviation {fn} {what}: {dev}")
            assert dev is not None, (what, "NaN positions")
            if dev > WORST["dew"]:
                WORST["dew"] = dev
                _counts.record("clock/max_deviation/dew", value=repr(dev), bound=repr(H.DEW_BOUND), case=what)
            assert dev <= H.DEW_BOUND, (what, dev)


def c_values(fn, args):
    P = product()
    if fn == "dur":
        return (int(args[0]),)
    if fn == "dew":
        return (P.rule_span(args[0]),)
    if fn == "rate":
        return (float(args[0]), P.window_ns(args[0]))
    return ()


def host_call(fn, inputs, args):
    out = getattr(product(), HOST[fn])(*inputs, *args)
    return out if isinstance(out, tuple) else (out,)


def dev_call(fn, inputs, args):
    """The `_dev` entry on resident copies of the inputs -> host arrays."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    P = product()
    ctx = _ffi.default_context()
    dev = [DeviceArray.from_host(ctx, a) for a in inputs]
    outs = P.resident(ctx, P.CLOCK_OPS[HOST[fn]], dev, *c_values(fn, args), unequal="unequal")
    return tuple(o.to_host() for o in outs)


def both(fn, inputs, args, want, what):
    """Host-pointer entry and `_dev` entry against `want`, and against each other in every bit."""
    h, d = host_call(fn, inputs, args), dev_call(fn, inputs, args)
    check(fn, h, want, what + " (host)")
    check(fn, d, want, what + " (_dev)")
    for a, b in zip(h, d):
        assert a.tobytes() == b.tobytes(), (what, "host and _dev differ")


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_fixture_replay(name):
    c = MANIFEST[name]
    both(c["fn"], H.generate(c["source"]), c["args"], expected(name), name)
    _counts.record(f"clock/fixture/{name}", outputs_compared=2 * c["n"])


# ---------------------------------------------------------------------------------------------- seeded tapes against the restatement
def _sizes():
    g = geo()
    t = g["scan_tile"]
    return (0, 1, 2, 3, 4, 5, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1, 3 * t + 77)


@pytest.mark.parametrize("fn", H.FUNCTIONS)
def test_seeded_tapes_at_the_edge_lengths(fn):
    compared = 0
    for k, n in enumerate(_sizes()):
        if fn == "run":
            inputs, args = H.returns(n, 3100 + k), []
        elif fn == "orb":
            inputs, args = (H.orb_walk(n, 3200 + k) if n else (np.empty(0, np.int64), np.empty(0), np.empty(0), np.empty(0))), []
        else:
            inputs = H.stamps(n, 3300 + k, 0.3)
            args = {"dur": [2], "dew": [7], "rate": [2.5]}[fn]
        both(fn, inputs, args, H.call(fn, inputs, args), f"{fn} n={n}")
        compared += n
    _counts.record(f"clock/seeded/{fn}", outputs_compared=2 * compared)


def test_a_second_trip_of_the_aggregate_scan():
    """More tiles than one trip of the scans' second launch takes, with a head whose reach crosses the trip: one run of equal signs
    and one day over the whole series, and the recurrence."""
    n = H.second_trip_length(geo())
    x = np.full(n, 0.5)
    both("run", (x,), [], H.call("run", (x,), []), "run: one run over two trips")
    (y,) = H.returns(n, 3401, 0.002, 0.0005)                          # long runs, a few of them over several tiles
    both("run", (y,), [], H.call("run", (y,), []), "run: long runs over two trips")
    tape = H.orb_tape([[19_950, 0, n, 100_000_000]], 3402)            # one day: the only head is row 0
    want = H.call("orb", tape, [])
    assert want[0].any() and want[1].any()
    both("orb", tape, [], want, "orb: one day over two trips")
    walk = H.orb_walk(n, 3403, -60_000)                               # some 120 000 days around 1970
    both("orb", walk, [], H.call("orb", walk, []), "orb: a walk over two trips")
    (ts,) = H.stamps(n, 3404)
    both("dew", (ts,), [20], H.call("dew", (ts,), [20]), "dew over two trips")
    both("dew", (ts,), [2000], H.call("dew", (ts,), [2000]), "dew span 2000 over two trips")
    _counts.record("clock/second_trip", n=n)


def test_bar_rate_windows_on_both_sides_of_the_stage():
    """Random windows from one microsecond to thirty minutes on a tape with duplicate stamps: slices that fit the LDS stage, slices
    that do not, and tiles of either kind in one call."""
    g = geo()
    n = 6 * g["rate_tile"] + 41
    (ts,) = H.stamps(n, 3500, 0.25)
    for w in (1e-6, 1e-3, 0.4, 30.0, float(g["rate_stage"] - g["rate_tile"]), 1800.0):
        want = H.call("rate", (ts,), [w])
        both("rate", (ts,), [w], want, f"rate w={w}")
    lb = np.searchsorted(ts, ts - H.window_ns(1800.0), side="left")
    first = np.arange(0, n, g["rate_tile"])
    spans = np.minimum(first + g["rate_tile"], n) - lb[first]         # rows a tile has to see: staged when they fit
    assert (spans > g["rate_stage"]).any() and (spans <= g["rate_stage"]).any()
    (reg,) = H.regular(n, H.SECOND)
    for k in (g["rate_stage"] - g["rate_tile"] - 1, g["rate_stage"] - g["rate_tile"], g["rate_stage"] - g["rate_tile"] + 1):
        both("rate", (reg,), [float(k)], H.call("rate", (reg,), [float(k)]), f"rate regular k={k}")


def test_bar_duration_periods():
    (ts,) = H.stamps(700, 3600, 0.2)
    for p in (1, 3, 0, -2, 700, 701, -699, -700, 2**40, -(2**62)):
        both("dur", (ts,), [p], (H.bar_duration(ts, p),), f"dur periods={p}")


def test_outputs_at_odd_addresses():
    """Views that start 1 .. 7 bytes past an 8-byte boundary: the scans store their int8 / uint8 outputs byte by byte there."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    n = 2 * geo()["scan_tile"] + 19
    (x,) = H.returns(n, 3700)
    tape = H.orb_walk(n, 3701)
    dx = DeviceArray.from_host(ctx, x)
    dt = [DeviceArray.from_host(ctx, a) for a in tape]
    for off in (1, 3, 7):
        buf = DeviceArray.from_host(ctx, np.full(n + 16, 77, np.int8))
        ctx.call("fmk_dir_run_len_dev", dx.p, C.c_int64(n), buf.view(off, n).p)
        got = buf.to_host()
        assert H.same_bits(got[off:off + n], H.dir_run_len(x)) and (got[:off] == 77).all() and (got[off + n:] == 77).all()
        a, b = (DeviceArray.from_host(ctx, np.full(n + 16, 77, np.uint8)) for _ in range(2))
        ctx.call("fmk_orb_break_dev", *(d.p for d in dt), C.c_int64(n), a.view(off, n).p, b.view(8 - off, n).p)
        lg, sh = H.orb_break(*tape)
        ga, gb = a.to_host(), b.to_host()
        assert H.same_bits(ga[off:off + n].view(np.bool_), lg) and H.same_bits(gb[8 - off:8 - off + n].view(np.bool_), sh)
        assert (ga[:off] == 77).all() and (ga[off + n:] == 77).all() and (gb[:8 - off] == 77).all() and (gb[8 - off + n:] == 77).all()


def test_refusals_through_the_raw_abi():
    from finmlkit_amd import _ffi
    ctx, lib = _ffi.default_context(), _ffi.lib()
    i64, f64 = C.c_int64, C.c_double
    big = i64(1 << 31)
    calls = {"fmk_bar_duration": lambda n: (None, n, i64(1), None), "fmk_bar_duration_ewma": lambda n: (None, n, f64(20.0), None),
             "fmk_bar_rate": lambda n: (None, n, f64(5.0), i64(5 * H.SECOND), None), "fmk_dir_run_len": lambda n: (None, n, None),
             "fmk_orb_break": lambda n: (None, None, None, None, n, None, None)}
    for entry, args in calls.items():
        for name in (entry, entry + "_dev"):                         # refused before any pointer is looked at
            assert getattr(lib, name)(ctx.handle, *args(big)) == _ffi.E_ARG, name
            assert getattr(lib, name)(ctx.handle, *args(i64(0))) == _ffi.OK, name
    for name in ("fmk_bar_duration_ewma", "fmk_bar_duration_ewma_dev"):
        assert getattr(lib, name)(ctx.handle, None, i64(10), f64(0.5), None) == _ffi.E_ARG
        assert "span size" in lib.fmk_last_error(ctx.handle).decode()
    for name in ("fmk_bar_rate", "fmk_bar_rate_dev"):
        assert getattr(lib, name)(ctx.handle, None, i64(10), f64(0.0), i64(0), None) == _ffi.E_ARG
        assert lib.fmk_last_error(ctx.handle).decode() == product().BAR_RATE_WINDOW_MESSAGE


# ---------------------------------------------------------------------------------------------- DeviceTrades, transforms, Compose
def test_device_trades_methods():
    from finmlkit_amd import engine
    from finmlkit_amd._ffi import DeviceArray
    n = geo()["scan_tile"] + 333
    tape = H.orb_walk(n, 3800)
    ts, high, low, close = tape
    t = engine.DeviceTrades.from_numpy(ts, close, np.ones(n, np.float32))
    check("dur", (t.bar_duration().to_host(),), (H.bar_duration(ts, 1),), "DeviceTrades.bar_duration")
    check("dur", (t.bar_duration(3).to_host(),), (H.bar_duration(ts, 3),), "DeviceTrades.bar_duration(3)")
    check("dew", (t.bar_duration_ewma().to_host(),), (H.bar_duration_ewma(ts, 20),), "DeviceTrades.bar_duration_ewma")
    check("rate", (t.bar_rate(3600.0).to_host(),), (H.bar_rate(ts, 3600.0),), "DeviceTrades.bar_rate")
    (x,) = H.returns(n, 3801)
    r = t.dir_run_len(DeviceArray.from_host(t.ctx, x))
    assert r.dtype == np.int8
    check("run", (r.to_host(),), (H.dir_run_len(x),), "DeviceTrades.dir_run_len")
    lg, sh = t.orb_break(DeviceArray.from_host(t.ctx, high), DeviceArray.from_host(t.ctx, low), t.price)
    assert lg.dtype == sh.dtype == np.uint8
    check("orb", (lg.to_host(), sh.to_host()), H.orb_break(*tape), "DeviceTrades.orb_break")
    # bar stamps of its own instead of the tape's
    (bars,) = H.stamps(500, 3802)
    db = DeviceArray.from_host(t.ctx, bars)
    check("dur", (t.bar_duration(2, ts=db).to_host(),), (H.bar_duration(bars, 2),), "bar_duration(ts=)")
    check("dew", (t.bar_duration_ewma(5, ts=db).to_host(),), (H.bar_duration_ewma(bars, 5),), "bar_duration_ewma(ts=)")
    check("rate", (t.bar_rate(1.5, ts=db).to_host(),), (H.bar_rate(bars, 1.5),), "bar_rate(ts=)")
    empty = DeviceArray(t.ctx, 0, np.int64, dptr=0)
    assert t.bar_duration(ts=empty).n == 0 and t.bar_rate(5.0, ts=empty).n == 0 and t.bar_duration_ewma(ts=empty).n == 0


def test_transforms_on_frames():
    from finmlkit_amd.feature import transforms as T
    n = geo()["scan_tile"] + 91
    tape = H.orb_walk(n, 3900)
    ts, high, low, close = tape
    (x,) = H.returns(n, 3901)
    frame = pd.DataFrame({"high": high, "low": low, "close": close, "ret1": x}, index=pd.DatetimeIndex(ts))
    for backend in ("nb", "pd"):
        s = T.BarDuration(2)(frame, backend=backend)
        assert s.name == "dur_2bar" and s.index.equals(frame.index)
        check("dur", (s.values,), (H.bar_duration(ts, 2),), "BarDuration")
        s = T.BarDurationEWMA(9)(frame, backend=backend)
        assert s.name == "dur_ewma9"
        check("dew", (s.values,), (H.bar_duration_ewma(ts, 9),), "BarDurationEWMA")
        s = T.BarRate(pd.Timedelta(hours=6))(frame, backend=backend)
        assert s.name == "bars_per_hour"
        check("rate", (s.values,), (H.bar_rate(ts, 21600.0),), "BarRate")
        s = T.DirRunLen()(frame, backend=backend)
        assert s.name == "ret1_dir_run_len" and s.dtype == np.int8
        check("run", (s.values,), (H.dir_run_len(x),), "DirRunLen")
        lg, sh = T.ORBBreak()(frame, backend=backend)
        assert (lg.name, sh.name) == ("orb_long", "orb_short") and lg.dtype == sh.dtype == np.bool_ and lg.index.equals(frame.index)
        check("orb", (lg.values, sh.values), H.orb_break(*tape), "ORBBreak")


def _prices_for(x):
    """A price path on a regular one-second clock whose one-second returns carry the signs of x (x[0] has no return)."""
    step = np.where(np.isnan(x), 0.0, np.sign(x))
    level = np.cumsum(step)
    px = 100.0 * (1.0 + 2.0**-10) ** level
    px[np.isnan(x)] = np.nan
    return px


@pytest.mark.parametrize("name", sorted(k for k in MANIFEST if k.startswith("run.") and MANIFEST[k]["n"] > 1))
def test_dir_run_len_cases_under_compose_after_return_t(name):
    """The run-length cases once more as Compose(ReturnT, DirRunLen): the returns stay on the device.  The expected run lengths are
    the restatement's on the returns the package's own comp_lagged_returns gives; the signs of the case survive the detour."""
    from finmlkit_amd.feature import transforms as T
    from finmlkit_amd.feature.core.utils import comp_lagged_returns
    (x,) = H.generate(MANIFEST[name]["source"])
    n = len(x)
    px = _prices_for(x)
    (ts,) = H.regular(n, H.SECOND)
    frame = pd.DataFrame({"price": px}, index=pd.DatetimeIndex(ts))
    chain = T.Compose(T.ReturnT(pd.Timedelta(seconds=1), input_col="price"), T.DirRunLen("ret1.0s"))
    got = chain(frame)
    assert got.name == "price_ret1.0s_dir_run_len" and got.dtype == np.int8
    ret = comp_lagged_returns(ts, px, 1.0, False)
    plain = np.isfinite(px[1:]) & np.isfinite(px[:-1])
    assert np.array_equal(np.sign(ret[1:][plain]), np.sign(x[1:][plain]))
    check("run", (got.values,), (H.dir_run_len(ret),), name + " under Compose")


def test_clock_transforms_under_compose():
    from finmlkit_amd.feature import transforms as T
    from finmlkit_amd.feature.core.ma import sma
    n = geo()["scan_tile"] + 57
    (ts,) = H.stamps(n, 4000, 0.2)
    close = np.linspace(100.0, 101.0, n)
    frame = pd.DataFrame({"close": close}, index=pd.DatetimeIndex(ts))
    s = T.Compose(T.SMA(3, "close"), T.BarDuration(2, "sma3"))(frame)
    assert s.name == "close_sma3_dur_2bar"
    check("dur", (s.values,), (H.bar_duration(ts, 2),), "Compose(SMA, BarDuration)")
    s = T.Compose(T.SMA(3, "close"), T.BarDurationEWMA(20, "sma3"))(frame)
    assert s.name == "close_sma3_dur_ewma20"
    check("dew", (s.values,), (H.bar_duration_ewma(ts, 20),), "Compose(SMA, BarDurationEWMA)")
    s = T.Compose(T.BarRate(pd.Timedelta(seconds=90)), T.SMA(4, "rate_1.5m"))(frame)
    assert s.name == "close_rate_1.5m_sma4"
    check("dur", (s.values,), (sma(H.bar_rate(ts, 90.0), 4),), "Compose(BarRate, SMA)")
    s = T.Compose(T.BarDuration(), T.DirRunLen("dur_1bar"))(frame)                 # zero durations are zeros, the first is NaN
    assert s.name == "close_dur_1bar_dir_run_len"
    check("run", (s.values,), (H.dir_run_len(H.bar_duration(ts, 1)),), "Compose(BarDuration, DirRunLen)")
