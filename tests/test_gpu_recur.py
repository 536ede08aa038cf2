"""The recursive indicators on the MI355X -- ewma, rsi_wilder, true_range, atr, adx_core (csrc/fmk_recur.hip) -- against the untouched
reference's recorded outputs (tests/golden/recur.npz) and the sequential restatement of tests/_recur_ref.py.

Bit for bit (np.array_equal, equal_nan=True): true_range, atr in SMA mode with and without normalize, every output before a seed
index, where any output is NaN, and where adx_core is exactly 0.0.  Within BOUND: ewma, rsi_wilder, atr in EMA mode and adx_core from
their seed on, where the state that enters a thread's eight elements is composed from tile aggregates instead of stepped.  The
contract's ceiling is 1e-9 relative (ewma, atr) and 1e-7 absolute on the 0-100 scale (rsi_wilder, adx_core); BOUND is the largest
deviation measured on the MI355X over every case of this file x 16, rounded up to a power of ten (DESIGN.md 7e holds the
figures).  Every comparison goes through close(), which also keeps the largest deviation per function and reports it with the
parity counts.  The inputs hold no infinities and no long loss-free runs: both are outside the contract."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _counts
from tests import _recur_ref as H
from tests.test_recur_host import MANIFEST, OK_CASES, REFUSED, case_input, expected, product

pytestmark = pytest.mark.gpu

THREADS = 256                        # lanes per workgroup (csrc/fmk_recur.hip: RC_THREADS)
ITEMS = 8                            # consecutive elements per lane (RC_ITEMS)
TILE = THREADS * ITEMS               # elements per workgroup of the scan's first and third launch (RC_TILE)
AGG_UNIT = 256                       # tile aggregates per trip of the aggregate scan (RC_AGG_UNIT)
SMA_TILE = 1024                      # atr, SMA mode: outputs per workgroup of the window walk (ATR_TILE)
ENTRY = {"ewma": "fmk_ewma", "rsi": "fmk_rsi_wilder", "tr": "fmk_true_range", "atr": "fmk_atr", "adx": "fmk_adx"}
WINDOWS = (1, 2, 3, 14, 100)
# measured on the MI355X over all cases below: ewma 4.4e-15 and atr (EMA) 7.1e-14 relative, rsi_wilder 2.0e-13 and
# adx_core 8.8e-14 absolute; each x 16, rounded up to a power of ten
BOUND = {"ewma": 1e-13, "atr": 1e-11, "rsi": 1e-11, "adx": 1e-11}
RELATIVE = {"ewma": True, "atr": True, "rsi": False, "adx": False}
SENTINEL = 12345.678
WORST = {}


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert np.array_equal(got, want, equal_nan=True), (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def close(fn, got, want, what, exact=False):
    """NaN positions and adx's zeros exactly; the rest bit for bit (`exact`: true_range, the SMA mode) or within BOUND[fn]: the
    absolute deviation (rsi, adx) at every element that is a number, the relative one (ewma, atr) at every one that is not 0.0."""
    got, want = np.asarray(got), np.asarray(want)
    if exact or fn == "tr":
        return equal(got, want, what)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(np.isnan(got) != np.isnan(want))[0]
    assert len(bad) == 0, (what, "NaN positions", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    assert not np.isinf(got).any() and not np.isinf(want).any(), what
    if fn == "adx":
        bad = np.nonzero((got == 0) != (want == 0))[0]
        assert len(bad) == 0, (what, "zeros", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    ok = ~np.isnan(want)
    if RELATIVE[fn]:                               # where the expected value is 0.0 there is no quotient: zero, or within the bound of it
        zero = ok & (want == 0)
        bad = np.nonzero(zero & (np.abs(got) > BOUND[fn]))[0]
        assert len(bad) == 0, (what, "expected 0.0", len(bad), bad[:5], got[bad[:3]])
        ok &= ~zero
    if not ok.any():
        return
    dev = np.abs(got[ok] - want[ok])
    if RELATIVE[fn]:
        dev = dev / np.abs(want[ok])
    worst = float(dev.max())
    if worst > WORST.get(fn, (0.0, ""))[0]:
        WORST[fn] = (worst, what)
        _counts.record(f"recur/max_deviation/{fn}", value=repr(worst), relative=RELATIVE[fn], bound=repr(BOUND[fn]), case=what)
    print(f"deviation {fn} {what}: {worst:.3e}")
    assert worst <= BOUND[fn], (what, worst, BOUND[fn], int(np.nonzero(ok)[0][dev.argmax()]))


def is_exact(fn, args):
    return fn == "tr" or (fn == "atr" and not args[1])


def dev_call(fn, inputs, args, ctx=None, prefill=None, resident=None):
    """The `_dev` entry of `fn` on resident copies of the inputs -> host array.  prefill: what the output buffer holds before the
    call, so that an element the kernels do not write shows.  resident: DeviceArrays (or views) to use instead of uploading."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = ctx or _ffi.default_context()
    n = len(inputs[0]) if resident is None else resident[0].n
    dev = resident or [DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=np.float64)) for a in inputs]
    out = DeviceArray(ctx, n, np.float64) if prefill is None else DeviceArray.from_host(ctx, np.full(n, prefill, np.float64))
    ctx.call(ENTRY[fn] + "_dev", *(d.p for d in dev), C.c_int64(n), *c_args(fn, args), out.p)
    return out.to_host()


def c_args(fn, args):
    if fn == "ewma":
        return (C.c_double(float(args[0])),)
    if fn == "atr":
        return (C.c_int64(int(args[0])), C.c_int(bool(args[1])), C.c_int(bool(args[2])))
    return tuple(C.c_int64(int(a)) for a in args)


def seed_index(fn, args):
    """The first index whose output carries a value."""
    return {"ewma": lambda: 0, "rsi": lambda: args[0], "tr": lambda: 0, "atr": lambda: args[0] - 1, "adx": lambda: 2 * args[0] - 1}[fn]()


@pytest.fixture(scope="module")
def series():
    """A grid walk and an OHLC walk as (high, low, close), shared by the tests below (never written to); both resident as well."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    n = 3 * TILE + 300
    made = (H.grid_walk(n, 801),) + H.hlc_walk(n, 802)
    assert all(np.isfinite(a).all() for a in made)
    assert H.longest_loss_free_run(made[0]) * 20 < math.log(1e-300) / math.log(0.5)
    for a in made:
        a.setflags(write=False)
    ctx = _ffi.default_context()
    return made, [DeviceArray.from_host(ctx, a) for a in made]


def inputs_of(fn, made, n):
    """The last n elements of the shared series: another phase of the series at every size."""
    full = made[:1] if fn in ("ewma", "rsi") else made[1:]
    return tuple(a[len(a) - n:] for a in full)


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay(name):
    c, ins = MANIFEST[name], case_input(name)
    fn, args = c["fn"], c["args"]
    close(fn, H.call(fn, ins, args, mod=product()), expected(name), name + " (python)", is_exact(fn, args))
    if c["n"]:
        close(fn, dev_call(fn, ins, args, prefill=SENTINEL), expected(name), name + " (_dev)", is_exact(fn, args))
    _counts.record(f"recur/fixture/{name}", outputs_compared=2 * c["n"], finite=c["finite"])


@pytest.mark.parametrize("name", [k for k in REFUSED if "unequal" not in k])
def test_refused_arguments_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    c, ins = MANIFEST[name], case_input(name)
    fn, args = c["fn"], c["args"]
    ctx, lib = _ffi.default_context(), _ffi.lib()
    with pytest.raises(ValueError) as e:
        dev_call(fn, ins, args)
    assert c["message"] in str(e.value)
    n = len(ins[0])
    out = np.zeros(n)
    rc = getattr(lib, ENTRY[fn])(ctx.handle, *(_ffi.ptr(a) for a in ins), C.c_int64(n), *c_args(fn, args), _ffi.ptr(out))
    assert rc == _ffi.E_ARG
    rc = getattr(lib, ENTRY[fn] + "_dev")(ctx.handle, *(None for _ in ins), C.c_int64(n), *c_args(fn, args), None)
    assert rc == _ffi.E_ARG                      # refused before any pointer is looked at


def test_a_series_of_two_to_the_31_is_refused():
    from finmlkit_amd import _ffi
    ctx, lib = _ffi.default_context(), _ffi.lib()
    for fn, nin, args in (("ewma", 1, [5]), ("rsi", 1, [5]), ("tr", 3, []), ("atr", 3, [5, True, False]), ("adx", 3, [5])):
        for entry in (ENTRY[fn] + "_dev", ENTRY[fn]):      # the host-pointer flavour too: nothing is uploaded first
            rc = getattr(lib, entry)(ctx.handle, *(None for _ in range(nin)), C.c_int64(1 << 31), *c_args(fn, args), None)
            assert rc == _ffi.E_ARG, entry


# ---------------------------------------------------------------------------------------------- geometry
GEOMETRY = [("ewma", [w]) for w in WINDOWS] + [("rsi", [w]) for w in WINDOWS] + [("atr", [w, True, False]) for w in WINDOWS] + \
    [("atr", [w, False, True]) for w in WINDOWS] + [("adx", [w]) for w in WINDOWS] + [("atr", [14, True, True]), ("tr", [])]


@pytest.mark.parametrize("fn,args", GEOMETRY, ids=lambda v: v if isinstance(v, str) else "-".join(str(a) for a in v))
def test_geometry(series, fn, args):
    """Lengths seed + m around the lane's eight elements and the tile, through the Python functions on the last n elements of one
    series; and every length below the seed that differs: all NaN, or all zero for adx_core."""
    made, _ = series
    seed = seed_index(fn, args)
    tile = SMA_TILE if is_exact(fn, args) and fn == "atr" else TILE
    lengths = sorted({seed + m for m in (0, 1, 7, 8, 9, tile - 1, tile, tile + 1, 2 * tile + 1)} | {max(seed - 1, 1), max(seed // 2, 1)})
    compared = 0
    for n in lengths:
        ins = inputs_of(fn, made, n)
        want = H.call(fn, ins, args)
        if n <= seed:
            assert (want == 0).all() if fn == "adx" else np.isnan(want).all()
        elif fn != "rsi" or args[0] >= 14:         # (a short window without a loss gives NaN)
            assert np.isfinite(want[seed:]).all()
        close(fn, H.call(fn, ins, args, mod=product()), want, f"{fn} {args} n={n}", is_exact(fn, args))
        compared += n
    _counts.record(f"recur/geometry/{fn}_{'_'.join(str(a) for a in args)}", outputs_compared=compared)


@pytest.mark.parametrize("fn,args", [("ewma", [14]), ("rsi", [14]), ("atr", [14, True, False]), ("adx", [14])],
                         ids=("ewma", "rsi", "atr_ema", "adx"))
def test_second_trip_of_the_aggregate_scan(fn, args):
    """One tile aggregate more than a trip of the aggregate scan takes, and a few elements: the carried map crosses trips."""
    n = AGG_UNIT * TILE + TILE + 9
    assert -(-n // TILE) == AGG_UNIT + 2 and n < 1 << 20
    # (moves of 5 cents at most: half a million larger ones reach the generators' floor of 1.00 and stay there)
    ins = (H.grid_walk(n, 803, 5),) if fn in ("ewma", "rsi") else H.hlc_walk(n, 804, 5, 30)
    assert all(a.min() > 10.0 for a in ins)
    assert all(np.isfinite(a).all() for a in ins)
    if fn == "rsi":
        assert H.longest_loss_free_run(ins[0]) * 20 < math.log(1e-300) / math.log(13 / 14)
    want = H.call(fn, ins, args)
    assert np.isfinite(want[seed_index(fn, args):]).all()
    close(fn, dev_call(fn, ins, args, prefill=SENTINEL), want, f"{fn} {args} n={n} (second trip)")
    _counts.record(f"recur/second_trip/{fn}", outputs_compared=n)


# ---------------------------------------------------------------------------------------------- seed placement
SEEDS = [("rsi", [w]) for w in (TILE - 1, TILE, TILE + 1)] + [("atr", [w, True, False]) for w in (TILE - 1, TILE, TILE + 1)] + \
    [("atr", [w, False, False]) for w in (SMA_TILE - 1, SMA_TILE, SMA_TILE + 1)] + \
    [("adx", [length]) for length in (TILE // 2, TILE // 2 + 1, TILE - 1, TILE)]


@pytest.mark.parametrize("fn,args", SEEDS, ids=lambda v: v if isinstance(v, str) else "-".join(str(a) for a in v))
def test_seed_at_a_tile_edge(series, fn, args):
    """The seed index in the last element of a tile and in the first of the next (adx_core: 2 L - 1 = TILE - 1 and TILE + 1, and
    the seed of the sums at TILE - 1 and TILE), on resident views of the shared series with a prefilled output."""
    made, resident = series
    seed = seed_index(fn, args)
    n = seed + TILE + 9
    full = resident[:1] if fn == "rsi" else resident[1:]
    views = [d.view(d.n - n, n) for d in full]
    ins = inputs_of(fn, made, n)
    want = H.call(fn, ins, args)
    assert np.isfinite(want[seed:]).all() and (fn == "adx" or np.isnan(want[:seed]).all())
    close(fn, dev_call(fn, None, args, prefill=SENTINEL, resident=views), want, f"{fn} {args} n={n} (seed edge)", is_exact(fn, args))
    _counts.record(f"recur/seed_edge/{fn}_{args[0]}", outputs_compared=n)


# ---------------------------------------------------------------------------------------------- NaN, positions compared exactly
@pytest.mark.parametrize("at", (TILE - 1, TILE, 2 * TILE - 8, 2 * TILE - 9))
def test_a_nan_poisons_ewma_and_the_ema_mode_for_good(series, at):
    made, _ = series
    n = 2 * TILE + 100
    (y,) = (a.copy() for a in inputs_of("ewma", made, n))
    y[at] = np.nan
    want = H.ewma(y, 14)
    assert np.isfinite(want[:at]).all() and np.isnan(want[at:]).all()
    close("ewma", dev_call("ewma", (y,), [14], prefill=SENTINEL), want, f"ewma NaN at {at}")
    for col in range(3):                           # high, low: the bar's true range; close: the next bar's
        ins = [a.copy() for a in inputs_of("atr", made, n)]
        ins[col][at] = np.nan
        first = at + (col == 2)
        for norm in (False, True):
            want = H.atr(*ins, 14, True, norm)
            assert np.isfinite(want[13:first]).all() and np.isnan(want[first:]).all()
            close("atr", dev_call("atr", tuple(ins), [14, True, norm], prefill=SENTINEL), want, f"atr ema NaN in column {col} at {at}")


def test_rsi_nan_rules(series):
    made, _ = series
    n = 2 * TILE + 100
    for w, at in ((14, 0), (14, 14), (TILE + 5, TILE - 1), (TILE + 5, TILE)):       # inside the first window: NaN everywhere
        (c,) = (a.copy() for a in inputs_of("rsi", made, n))
        c[at] = np.nan
        want = H.rsi_wilder(c, w)
        assert np.isnan(want).all()
        close("rsi", dev_call("rsi", (c,), [w], prefill=SENTINEL), want, f"rsi w={w} NaN at {at} (seed window)")
    for at in (15, TILE - 1, TILE, TILE + 1):                                      # after it: finite around the NaN
        (c,) = (a.copy() for a in inputs_of("rsi", made, n))
        c[at] = np.nan
        want = H.rsi_wilder(c, 14)
        assert np.isnan(want[:14]).all() and np.isfinite(want[14:]).all()
        close("rsi", dev_call("rsi", (c,), [14], prefill=SENTINEL), want, f"rsi NaN at {at} (after the seed)")


@pytest.mark.parametrize("window", (1, 2, 3, 14, 100))
def test_sma_mode_nan_runs_across_a_tile_edge(series, window):
    """NaN runs shorter and longer than the window across the edge of the walk's tile, and the NaN at bar 2."""
    made, _ = series
    n = 2 * SMA_TILE + window + 50
    edge = window - 1 + SMA_TILE                   # the first output of the second workgroup
    for run in (max(1, window // 2), window + 3):
        for start in (edge - run // 2 - 1, edge - run, edge):
            h, lo, c = (a.copy() for a in inputs_of("atr", made, n))
            h[start:start + run] = np.nan
            c[5] = np.nan
            lo[2] = h[2] = c[2] = np.nan
            for norm in (False, True):
                want = H.atr(h, lo, c, window, False, norm)
                assert np.isnan(want[window - 1:]).sum() >= (run > window) and np.isfinite(want).sum() > n // 2
                equal(dev_call("atr", (h, lo, c), [window, False, norm], prefill=SENTINEL), want, f"atr sma w={window} run={run} at {start}")
    equal(dev_call("tr", (h, lo, c), [], prefill=SENTINEL), H.true_range(h, lo, c), "true_range with NaN")


def test_adx_nan_rules(series):
    made, _ = series
    n = TILE + 500
    for at in (9, 13, 20, TILE - 1, TILE):             # in the seed window of the sums (bars 1 .. 14): zero everywhere
        ins = [a.copy() for a in inputs_of("adx", made, n)]
        ins[at % 3][at] = np.nan
        want = H.adx_core(*ins, 14)
        assert (want == 0).all() == (at < 14) and np.isfinite(want).all()
        close("adx", dev_call("adx", tuple(ins), [14], prefill=SENTINEL), want, f"adx NaN at {at}")


# ---------------------------------------------------------------------------------------------- every element is written
@pytest.mark.parametrize("fn,args", [("ewma", [3]), ("rsi", [300]), ("tr", []), ("atr", [300, True, False]), ("atr", [300, False, False]),
                                     ("atr", [0, True, False]), ("adx", [5]), ("adx", [700]), ("adx", [5000])],
                         ids=lambda v: v if isinstance(v, str) else "-".join(str(a) for a in v))
def test_no_element_is_left_unwritten(series, fn, args):
    """A prefilled output buffer: the NaN head, adx_core's zeros before its seed and a series shorter than the seed all come from
    the kernels."""
    made, _ = series
    for n in (1, 7, TILE - 1, TILE + 1, 2 * TILE + 3):
        ins = inputs_of(fn, made, n)
        got = dev_call(fn, ins, args, prefill=SENTINEL)
        assert not (got == SENTINEL).any(), (fn, args, n)
        close(fn, got, H.call(fn, ins, args), f"{fn} {args} n={n} (prefilled)", is_exact(fn, args))


# ---------------------------------------------------------------------------------------------- transforms, Compose, DeviceTrades
def test_transforms_on_a_small_frame():
    import pandas as pd

    from finmlkit_amd.feature.transforms import ADX, ATR, EWMA, RSIWilder
    n = 500
    h, lo, c = H.hlc_walk(n, 810)
    idx = pd.date_range("2024-01-01", periods=n, freq="min")
    frame = pd.DataFrame({"high": h, "low": lo, "close": c}, index=idx)
    for backend in ("nb", "pd"):
        for t, fn, args, ins in ((RSIWilder(14), "rsi", [14], (c,)), (ATR(14), "atr", [14, False, False], (h, lo, c)),
                                 (ATR(14, True, True), "atr", [14, True, True], (h, lo, c)), (ADX(14), "adx", [14], (h, lo, c))):
            s = t(frame, backend=backend)
            assert s.name == t.output_name and s.index.equals(idx)
            close(fn, s.values, H.call(fn, ins, args), f"{type(t).__name__} {backend}", is_exact(fn, args))
    e = EWMA(10, "close")
    s = e(frame)
    assert s.name == "close_ewma10"
    close("ewma", s.values, H.ewma(c, 10), "EWMA nb")
    p = e(frame, backend="pd")                     # pandas' own ewm: the same weights, another evaluation order
    assert p.name == "close_ewma10"
    np.testing.assert_allclose(p.values, H.ewma(c, 10), rtol=1e-12)
    swapped = ATR(14, input_cols=["low", "high", "close"])(frame)      # the columns go to (high, low, close) in the order given
    equal(swapped.values, H.atr(lo, h, c, 14), "ATR with the columns swapped")


def test_compose_chains_on_the_device():
    import pandas as pd

    from finmlkit_amd.feature.core.utils import comp_lagged_returns, pct_change
    from finmlkit_amd.feature.transforms import EWMA, Compose, PctChange, ReturnT, RSIWilder
    n = 3000
    c = H.grid_walk(n, 811)
    idx = pd.date_range("2024-01-01", periods=n, freq="s")
    frame = pd.DataFrame({"close": c}, index=idx)
    chain = Compose(ReturnT(pd.Timedelta(seconds=5), input_col="close"), EWMA(10, "ret5.0s"))
    got = chain(frame)
    assert got.name == "close_ret5.0s_ewma10"
    ret = comp_lagged_returns(idx.values.astype(np.int64), c, 5.0, False)
    close("ewma", got.values, H.ewma(ret, 10), "Compose(ReturnT, EWMA)")           # NaN from the first return on, as the reference
    chain = Compose(PctChange(1, "close"), RSIWilder(14, "pctc1"))
    got = chain(frame)
    assert got.name == "close_pctc1_rsiw14"
    close("rsi", got.values, H.rsi_wilder(pct_change(c, 1), 14), "Compose(PctChange, RSIWilder)")
    # a chain whose outputs are numbers: on the device path it is the two kernels on the same data, so it equals the two functions
    # called one after the other in every bit; those are held against the reference by the tests above
    chain = Compose(EWMA(5, "close"), RSIWilder(14, "ewma5"))
    got = chain(frame)
    assert got.name == "close_ewma5_rsiw14"
    P = product()
    smooth = P.ewma(c, 5)
    want = P.rsi_wilder(smooth, 14)
    assert np.isfinite(want[14:]).all() and len(set(want[14:])) > n // 2
    equal(got.values, want, "Compose(EWMA, RSIWilder)")
    close("ewma", smooth, H.ewma(c, 5), "Compose(EWMA, RSIWilder): the first step")
    close("rsi", want, H.rsi_wilder(smooth, 14), "Compose(EWMA, RSIWilder): the second step on the first's output")


def test_device_trades_methods():
    from finmlkit_amd import _ffi, engine
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    n = TILE + 77
    h, lo, c = H.hlc_walk(n, 812)
    t = engine.DeviceTrades.synth(16, seed=1, ctx=ctx)
    dh, dl, dc = (DeviceArray.from_host(ctx, a) for a in (h, lo, c))
    for got, fn, args, ins in ((t.ewma(dc, 14), "ewma", [14], (c,)), (t.rsi_wilder(dc, 14), "rsi", [14], (c,)),
                               (t.true_range(dh, dl, dc), "tr", [], (h, lo, c)), (t.atr(dh, dl, dc, 14), "atr", [14, False, False], (h, lo, c)),
                               (t.atr(dh, dl, dc, 14, True, True), "atr", [14, True, True], (h, lo, c)),
                               (t.adx(dh, dl, dc, 14), "adx", [14], (h, lo, c)), (t.adx(dh, dl, dc), "adx", [14], (h, lo, c))):
        assert isinstance(got, DeviceArray) and got.n == n and got.dtype == np.float64
        close(fn, got.to_host(), H.call(fn, ins, args), f"DeviceTrades {fn} {args}", is_exact(fn, args))
    empty = DeviceArray(ctx, 0, np.float64)
    assert t.ewma(empty, 3).n == 0 and t.adx(empty, empty, empty).n == 0
