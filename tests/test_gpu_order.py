"""The windowed order statistics on the MI355X -- comp_burst_ratio, stoch_k, roc, pct_change (csrc/fmk_order.hip) -- bit-equal
(np.array_equal, equal_nan=True) to the untouched reference's recorded outputs (tests/golden/order_stats.npz) and to the plain
restatement of tests/_order_ref.py.  There is no tolerance: a median, a minimum and a maximum are selections, and what follows them
is one or two IEEE operations in the reference's order.  Signed and infinite values, planted elements, NaN-saturated spans and the
second trip of the grid-stride loops: tests/test_gpu_order_edges.py."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _order_ref as H
from tests.test_order_host import MANIFEST, OK_CASES, REFUSED, VALUE_CLASS_CASES, case_input, expected, product

pytestmark = pytest.mark.gpu

BLOCK = 256                          # lanes per workgroup (csrc/fmk_order.hip: ORD_BLOCK)
TILE = 1024                          # sorted path: outputs per workgroup (ORD_TILE = ORD_BLOCK * ORD_OPL)
SPAN_MAX = 4096                      # sorted path: entries in LDS (ORD_SPAN_MAX)
SORT_WINDOW_MAX = SPAN_MAX - TILE + 1    # the largest window of the sorted path (ORD_SORT_WINDOW_MAX); the next takes the bisection
WALK_TILE = BLOCK                    # walk kernels (bisection, %K): outputs per workgroup (ORD_WALK_TILE)
SLAB = 4096                          # walk kernels: LDS elements per staging (csrc/fmk_window.h: FMK_SLAB_MAX)
ONE_SLAB_WINDOW = SLAB - WALK_TILE + 1   # walk kernels: the longest window whose full tile reads one slab
ENTRY = {"burst": "fmk_burst_ratio", "stoch": "fmk_stoch_k", "roc": "fmk_roc", "pct": "fmk_pct_change"}


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert np.array_equal(got, want, equal_nan=True), (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def equal_bits(got, want, what):
    """equal(), and where both are zero they have the same sign (burst ratio, roc and pct_change: the reference decides it)."""
    equal(got, want, what)
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero((got == 0) & (want == 0) & (np.signbit(got) != np.signbit(want)))[0]
    assert len(bad) == 0, (what, "the sign of a zero", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def dev_call(fn, inputs, arg, ctx=None, prefill=None):
    """The `_dev` entry of `fn` on resident copies of the inputs -> host array.  prefill: what the output buffer holds before the
    call, so that an element the kernels do not write shows."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = ctx or _ffi.default_context()
    ins = inputs if isinstance(inputs, tuple) else (inputs,)
    n = len(ins[0])
    dev = [DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=np.float64)) for a in ins]
    out = DeviceArray(ctx, n, np.float64) if prefill is None else DeviceArray.from_host(ctx, np.full(n, prefill, np.float64))
    ctx.call(ENTRY[fn] + "_dev", *(d.p for d in dev), C.c_int64(n), C.c_int64(arg), out.p)
    return out.to_host()


@pytest.fixture(scope="module")
def series():
    """The tie-heavy sizes, a grid walk and an OHLC walk, shared by the tests below (never written to)."""
    n = 6000
    made = (H.tie_sizes(n, 701), H.grid_walk(n, 702)) + H.ohlc_walk(n, 703)
    for a in made:
        a.setflags(write=False)
    return made


@pytest.fixture(scope="module")
def long_series():
    """The same kinds of series for the windows of two slabs and more."""
    n = 13_000
    made = (H.tie_sizes(n, 711), H.grid_walk(n, 712)) + H.ohlc_walk(n, 713)
    for a in made:
        a.setflags(write=False)
    return made


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", [k for k in OK_CASES if k not in VALUE_CLASS_CASES])      # those: tests/test_gpu_order_edges.py
def test_fixture_replay(name):
    c, ins = MANIFEST[name], case_input(name)
    equal(H.call(c["fn"], ins, c["arg"], mod=product()), expected(name), name + " (python)")
    equal(dev_call(c["fn"], ins, c["arg"]), expected(name), name + " (_dev)")
    _counts.record(f"order/fixture/{name}", outputs_compared=2 * c["n"], finite=c["finite"])


@pytest.mark.parametrize("name", [k for k in REFUSED if k != "refused.stoch_unequal"])
def test_refused_arguments_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    c, ins = MANIFEST[name], case_input(name)
    ctx = _ffi.default_context()
    with pytest.raises(ValueError) as e:
        dev_call(c["fn"], ins, c["arg"])
    assert c["message"] in str(e.value)
    # the status itself, from the host-pointer and the device flavour
    ins = ins if isinstance(ins, tuple) else (ins,)
    n = len(ins[0])
    out = np.zeros(n)
    lib = _ffi.lib()
    rc = getattr(lib, ENTRY[c["fn"]])(ctx.handle, *(_ffi.ptr(a) for a in ins), C.c_int64(n), C.c_int64(c["arg"]), _ffi.ptr(out))
    assert rc == _ffi.E_ARG
    rc = getattr(lib, ENTRY[c["fn"]] + "_dev")(ctx.handle, *(None for _ in ins), C.c_int64(n), C.c_int64(c["arg"]), None)
    assert rc == _ffi.E_ARG                      # refused before any pointer is looked at


def test_a_series_of_two_to_the_31_is_refused():
    from finmlkit_amd import _ffi
    ctx, lib = _ffi.default_context(), _ffi.lib()
    for fn, nin in (("burst", 1), ("stoch", 3), ("roc", 1), ("pct", 1)):
        rc = getattr(lib, ENTRY[fn] + "_dev")(ctx.handle, *(None for _ in range(nin)), C.c_int64(1 << 31), C.c_int64(5), None)
        assert rc == _ffi.E_ARG, fn


# ---------------------------------------------------------------------------------------------- geometry
def _lengths(window, tile):
    return sorted({window} | {window - 1 + m for m in (tile - 1, tile, tile + 1, 2 * tile + 1)})


# the rolling median: wave edges, the tile of the sorted path +-1, its largest window (both parities below it), the first windows of
# the bisection (both parities), a window of 1.2 times that, and where the bisection's walk takes a second slab
BURST_WINDOWS = [(w, TILE) for w in (1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, SORT_WINDOW_MAX - 1, SORT_WINDOW_MAX)]
BURST_WINDOWS += [(w, WALK_TILE) for w in (SORT_WINDOW_MAX + 1, SORT_WINDOW_MAX + 2, 3687, 3688, ONE_SLAB_WINDOW, ONE_SLAB_WINDOW + 1)]


# three slabs (the middle one lies wholly inside every lane's window), and a full tile's span of exactly two slabs and one more
LONG_WINDOWS = (2 * SLAB - WALK_TILE + 1, 2 * SLAB - WALK_TILE + 2, 8500, 8501)
BURST_WINDOWS += [(w, WALK_TILE) for w in LONG_WINDOWS]


@pytest.mark.parametrize("window,tile", BURST_WINDOWS)
def test_burst_ratio_geometry(series, long_series, window, tile):
    ties, walk = (long_series if window in LONG_WINDOWS else series)[:2]
    P = product()
    compared = 0
    for n in _lengths(window, tile):
        for name, full in (("ties", ties), ("walk", walk)):
            x = full[len(full) - n:]                             # the last n elements: another phase of the series at every size
            want = H.comp_burst_ratio(x, window)
            assert np.isfinite(want[window - 1:]).all()
            equal_bits(P.comp_burst_ratio(x, window), want, f"burst {name} n={n} w={window}")
            compared += n
    _counts.record(f"order/geometry/burst_w{window}", outputs_compared=compared)


# %K: the same edges for the walk kernel's tile and slab
STOCH_LENGTHS = (1, 2, 3, 63, 64, 65, WALK_TILE - 1, WALK_TILE, WALK_TILE + 1, ONE_SLAB_WINDOW, ONE_SLAB_WINDOW + 1, SLAB + 1)
STOCH_LENGTHS += LONG_WINDOWS[:3] + (12289,)                     # two slabs exactly, one element more, three slabs, four


@pytest.mark.parametrize("length", STOCH_LENGTHS)
def test_stoch_k_geometry(series, long_series, length):
    close, low, high = (long_series if length > SLAB + 1 else series)[2:]
    P = product()
    compared = 0
    for n in _lengths(length, WALK_TILE):
        c, lo, hi = (a[len(a) - n:] for a in (close, low, high))
        want = H.stoch_k(c, lo, hi, length)
        equal(P.stoch_k(c, lo, hi, length), want, f"stoch n={n} l={length}")
        if length > 1:
            assert np.isfinite(want[length - 1:]).all()
        compared += n
    _counts.record(f"order/geometry/stoch_l{length}", outputs_compared=compared)


def test_roc_and_pct_change_geometry(series):
    ties, walk = series[:2]
    P = product()
    compared = 0
    for n in (1, BLOCK - 1, BLOCK + 1, 5999):
        for lag in sorted({0, 1, 63, n - 1, n, n + 5}):
            for x in (walk[:n], ties[:n]):
                equal(P.roc(x, lag), H.roc(x, lag), f"roc n={n} p={lag}")
                equal(P.pct_change(x, lag), H.pct_change(x, lag), f"pct n={n} p={lag}")
                compared += 2 * n
    _counts.record("order/geometry/lagged", outputs_compared=compared)


# ---------------------------------------------------------------------------------------------- NaN runs, flat stretches
def test_burst_ratio_nan_runs_across_a_tile_edge(series):
    ties, walk = series[:2]
    P = product()
    n = 3 * TILE
    for window in (20, 21):
        edge = window - 1 + TILE                                 # the first output of the second tile
        for base in (ties, walk):
            x = np.array(base[:n])
            x[edge - 3:edge + 3] = np.nan                        # shorter than the window, over the edge
            x[edge + TILE - 25:edge + TILE + 15] = np.nan        # longer, over the next edge
            x[edge - window] = np.nan                            # leaves the window exactly at the edge
            x[100] = -np.nan                                     # a NaN with the sign bit set
            want = H.comp_burst_ratio(x, window)
            equal(P.comp_burst_ratio(x, window), want, f"burst w={window}")
            assert np.isnan(want[edge - 1]) and np.isnan(want[edge - 3:edge + 2 + window]).all()
            assert np.isnan(want[edge + TILE - 25:edge + TILE + 14 + window]).all() and np.isfinite(want[edge + TILE + 40:]).all()
            assert np.isnan(want[100:100 + window]).all() and np.isfinite(want[100 + window:edge - window]).all()
    # the bisection path: a window of the first size it takes, a NaN that leaves exactly at its tile edge
    window = SORT_WINDOW_MAX + 1
    edge = window - 1 + WALK_TILE
    x = np.array(ties[:window + 2 * WALK_TILE])
    x[edge - window] = np.nan
    x[edge + 40:edge + 43] = np.nan
    want = H.comp_burst_ratio(x, window)
    equal(P.comp_burst_ratio(x, window), want, "burst, bisection")
    assert np.isnan(want[edge - 1]) and np.isfinite(want[edge:edge + 40]).all() and np.isnan(want[edge + 40:]).all()
    _counts.record("order/nan_runs/burst", outputs_compared=4 * n + len(x))


def test_stoch_k_nan_runs_and_flat_stretch_across_a_tile_edge(series):
    close, low, high = series[2:]
    P = product()
    length, n = 20, 4 * WALK_TILE
    edge = length - 1 + WALK_TILE
    for which in ("low", "high", "both"):
        c, lo, hi = (np.array(a[:n]) for a in (close, low, high))
        for a in {"low": (lo,), "high": (hi,), "both": (lo, hi)}[which]:
            a[edge - 3:edge + 3] = np.nan                        # shorter than the window, over the edge
            a[edge + WALK_TILE - 25:edge + WALK_TILE + 15] = np.nan      # longer, over the next edge
            a[edge - length] = np.nan                            # leaves the window exactly at the edge
        want = H.stoch_k(c, lo, hi, length)
        equal(P.stoch_k(c, lo, hi, length), want, f"stoch NaN in {which}")
        assert np.isnan(want[edge - 1]) and np.isnan(want[edge - 3:edge + 2 + length]).all()
        assert np.isfinite(want[edge + 2 + length:edge + WALK_TILE - 25]).all() and np.isfinite(want[edge + WALK_TILE + 40:]).all()
    # equal low and high over a stretch that crosses the edge: hi == lo gives NaN on both sides
    c, lo, hi = (np.array(a[:n]) for a in (close, low, high))
    lo[edge - 40:edge + 40] = hi[edge - 40:edge + 40] = c[edge - 40:edge + 40] = 101.25
    want = H.stoch_k(c, lo, hi, length)
    equal(P.stoch_k(c, lo, hi, length), want, "stoch flat")
    flat = list(range(edge - 40 + length - 1, edge + 40))
    assert list(np.nonzero(np.isnan(want[length - 1:]))[0] + length - 1) == flat and flat[0] < edge < flat[-1]
    _counts.record("order/nan_runs/stoch", outputs_compared=4 * n)


# ---------------------------------------------------------------------------------------------- transforms and the resident flow
def test_transforms_and_compose(series):
    import pandas as pd
    from finmlkit_amd.feature.core.utils import comp_lagged_returns
    from finmlkit_amd.feature.transforms import ROC, BurstRatio, Compose, PctChange, ReturnT, StochK
    ties, walk, close, low, high = series
    n = 5000
    frame = pd.DataFrame({"amount": np.array(ties[:n]), "px": np.array(walk[:n]), "close": np.array(close[:n]),
                          "low": np.array(low[:n]), "high": np.array(high[:n])},
                         index=pd.date_range("2024-01-01", periods=n, freq="1s"))
    am, px = frame["amount"].values, frame["px"].values
    # the reference's StochK hands (high, low, close) to stoch_k(close, low, high): its output is what the transform gives
    swapped = H.stoch_k(frame["high"].values, frame["low"].values, frame["close"].values, 14)
    assert not np.array_equal(swapped, H.stoch_k(frame["close"].values, frame["low"].values, frame["high"].values, 14), equal_nan=True)
    for tr, want in ((BurstRatio(50, "amount"), H.comp_burst_ratio(am, 50)), (BurstRatio(7, "px"), H.comp_burst_ratio(px, 7)),
                     (ROC(5, input_col="px"), H.roc(px, 5)), (ROC(1), H.roc(frame["close"].values, 1)),
                     (PctChange(3, input_col="amount"), H.pct_change(am, 3)), (StochK(), swapped),
                     (StochK(5, ["close", "low", "high"]), H.stoch_k(frame["close"].values, frame["low"].values, frame["high"].values, 5))):
        for backend in ("nb", "pd"):
            s = tr(frame, backend=backend)
            assert s.index.equals(frame.index)
            if isinstance(tr, PctChange) and backend == "pd":    # pandas' own pct_change, under the input column's name
                assert s.name == "amount"
                equal(s.values, frame["amount"].pct_change(3).values, "pctc3 (pd)")
                continue
            assert s.name == tr.output_name
            equal(s.values, want, f"{tr.output_name} ({backend})")
    chain = Compose(PctChange(3, "amount"), BurstRatio(50, "pctc3"))
    s = chain(frame)                                             # the device-resident path: PctChange._dev -> BurstRatio._dev
    assert s.name == chain.output_name == "amount_pctc3_burst50" and s.index.equals(frame.index)
    want = H.comp_burst_ratio(H.pct_change(am, 3), 50)
    equal(s.values, want, chain.output_name)
    assert np.isnan(want[:52]).all() and np.isfinite(want[52:]).sum() > 100
    ret = ReturnT(pd.Timedelta(seconds=5), is_log=True, input_col="px")
    lagged = comp_lagged_returns(frame.index.values.astype(np.int64), px, 5.0, True)
    chain = Compose(ret, BurstRatio(64, "ret"))
    s = chain(frame)
    assert s.name == chain.output_name == "px_ret5.0s_burst64"
    want = H.comp_burst_ratio(lagged, 64)
    equal(s.values, want, chain.output_name)
    assert np.isnan(want[:68]).all() and np.isfinite(want[68:]).sum() > 100
    with pytest.raises(ValueError, match="window must be at least 1"):
        Compose(ret, BurstRatio(0, "ret"))(frame)
    _counts.record("order/transforms", outputs_compared=16 * n)


def test_device_trades_methods(series):
    from finmlkit_amd import engine
    from finmlkit_amd._ffi import DeviceArray
    ties, walk, close, low, high = series
    n = 6000
    t = engine.DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), np.array(walk[:n]), np.ones(n, np.float32))
    d = {k: DeviceArray.from_host(t.ctx, np.array(a[:n])) for k, a in (("ties", ties), ("close", close), ("low", low), ("high", high))}
    f32 = DeviceArray.from_host(t.ctx, np.array(ties[:n], dtype=np.float32))
    for fn in (lambda: t.burst_ratio(f32, 5), lambda: t.roc(f32, 5), lambda: t.pct_change(f32, 5),
               lambda: t.stoch_k(d["close"], f32, d["high"], 5)):
        with pytest.raises(TypeError, match="float64"):
            fn()
    got = {"burst": t.burst_ratio(d["ties"], 100), "burst_price": t.burst_ratio(t.price, 51), "roc": t.roc(t.price, 10),
           "pct": t.pct_change(d["ties"], 4), "stoch": t.stoch_k(d["close"], d["low"], d["high"], 14)}
    want = {"burst": H.comp_burst_ratio(ties[:n], 100), "burst_price": H.comp_burst_ratio(walk[:n], 51), "roc": H.roc(walk[:n], 10),
            "pct": H.pct_change(ties[:n], 4), "stoch": H.stoch_k(close[:n], low[:n], high[:n], 14)}
    for k, g in got.items():
        assert isinstance(g, DeviceArray) and g.dtype == np.float64 and g.n == n, k
        equal(g.to_host(), want[k], k)                           # the results come down once, for the comparison
    _counts.record("order/resident", outputs_compared=len(got) * n)
