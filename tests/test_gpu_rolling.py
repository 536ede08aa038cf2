"""The rolling-window moments on the MI355X -- sma, comp_zscore, rolling_variance_nb, variance_ratio_1_4_core (csrc/fmk_rolling.hip)
-- bit-equal (np.array_equal, equal_nan=True) to the reference's recorded outputs (tests/golden/rolling_stats.npz) and to the plain
restatement of tests/_rolling_ref.py.  There is no tolerance: every operation is an IEEE addition, subtraction, product, quotient or
square root in the reference's order, or the host's log."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _rolling_ref as H
from tests.test_rolling_host import MANIFEST, OK_CASES, REFUSED, case_input, expected, product

pytestmark = pytest.mark.gpu

BLOCK = 256                          # lanes per workgroup (csrc/fmk_rolling.hip: ROLL_BLOCK)
TILE = 1024                          # outputs per workgroup (ROLL_TILE = ROLL_BLOCK * ROLL_OPL)
SLAB = 4096                          # LDS elements per staging (csrc/fmk_window.h: FMK_SLAB_MAX)
ONE_SLAB_WINDOW = SLAB - TILE + 1    # the longest window whose full tile reads one slab (window - 1 + ROLL_TILE <= FMK_SLAB_MAX)


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert np.array_equal(got, want, equal_nan=True), (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def dev_call(fn, x, window, ddof=None, min_periods=None, ret_type=None, ctx=None):
    """The `_dev` entry of `fn` on a resident copy of x -> host array."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = ctx or _ffi.default_context()
    n = len(x)
    d_x, out = DeviceArray.from_host(ctx, np.ascontiguousarray(x, dtype=np.float64)), DeviceArray(ctx, n, np.float64)
    i64 = C.c_int64
    if fn == "sma":
        ctx.call("fmk_sma_dev", d_x.p, i64(n), i64(window), out.p)
    elif fn == "zscore":
        ctx.call("fmk_zscore_dev", d_x.p, i64(n), i64(window), i64(ddof), out.p)
    elif fn == "variance":
        ctx.call("fmk_rolling_variance_dev", d_x.p, i64(n), i64(window), i64(ddof), i64(min_periods), out.p)
    else:
        ctx.call("fmk_variance_ratio_1_4_dev", d_x.p, i64(n), i64(window), i64(ddof), C.c_int(ret_type == "log"), out.p)
    return out.to_host()


@pytest.fixture(scope="module")
def series():
    """One seeded walk and its log returns, shared by the tests below (never written to)."""
    n = 20_001
    px, ret = H.grid_walk(n, 901), H.walk_returns(n, 902)
    px.setflags(write=False)
    ret.setflags(write=False)
    return px, ret


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay(name):
    c, x = MANIFEST[name], case_input(name)
    args = (c["fn"], x, c["window"], c.get("ddof"), c.get("min_periods"), c.get("ret_type"))
    equal(H.call(*args, mod=product()), expected(name), name + " (python)")
    equal(dev_call(*args), expected(name), name + " (_dev)")
    _counts.record(f"rolling/fixture/{name}", outputs_compared=2 * c["n"], finite=c["finite"])


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    c, x = MANIFEST[name], case_input(name)
    ctx = _ffi.default_context()
    args = (c["fn"], x, c["window"], c.get("ddof"), c.get("min_periods"), c.get("ret_type"))
    with pytest.raises(ValueError) as e:
        dev_call(*args)
    assert c["message"] in str(e.value)
    # the status itself, from the device and the host-pointer flavour
    out = np.zeros(len(x))
    tail = {"sma": (), "zscore": (C.c_int64(c.get("ddof", 0)),), "variance": (C.c_int64(1), C.c_int64(1)),
            "ratio": (C.c_int64(0), C.c_int(1))}[c["fn"]]
    entry = {"sma": "fmk_sma", "zscore": "fmk_zscore", "variance": "fmk_rolling_variance", "ratio": "fmk_variance_ratio_1_4"}[c["fn"]]
    lib = _ffi.lib()
    rc = getattr(lib, entry)(ctx.handle, _ffi.ptr(x), C.c_int64(len(x)), C.c_int64(c["window"]), *tail, _ffi.ptr(out))
    assert rc == _ffi.E_ARG
    rc = getattr(lib, entry + "_dev")(ctx.handle, None, C.c_int64(len(x)), C.c_int64(c["window"]), *tail, None)
    assert rc == _ffi.E_ARG                      # refused before any pointer is looked at


# ---------------------------------------------------------------------------------------------- geometry
def _outputs(window, counts):
    return [(window - 1 + m, window) for m in counts]


GEOMETRY = []
for _w in (1, 2, 63, 64, 65):                                  # wave edges; n at one tile +-1 and two tiles +-1 of outputs
    GEOMETRY += _outputs(_w, (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1))
for _w in (BLOCK - 1, BLOCK + 1, TILE - 1, TILE + 1):          # a lane's outputs are ROLL_BLOCK apart; the tile size
    GEOMETRY += _outputs(_w, (TILE + 1, 2 * TILE + 1))
for _w in (ONE_SLAB_WINDOW - 1, ONE_SLAB_WINDOW, ONE_SLAB_WINDOW + 1, SLAB - 1, SLAB, SLAB + 1):
    GEOMETRY += _outputs(_w, (TILE + 1,))                      # where a second slab begins; a window of one slab +-1
GEOMETRY += _outputs(4915, (5, 2 * TILE + 1))                  # a window of 1.2 slabs
GEOMETRY += [(20_001, 65), (20_001, TILE + 1), (64, 65), (1, 1)]
# a full tile's span of exactly two slabs and of one element more; three slabs (the middle one lies wholly inside every window); four
for _w in (2 * SLAB - TILE + 1, 2 * SLAB - TILE + 2, 8500, 12289):
    GEOMETRY += _outputs(_w, (TILE + 1,))


@pytest.mark.parametrize("n,window", GEOMETRY)
def test_geometry(series, n, window):
    px, ret = series
    P = product()
    off = len(px) - n                                           # the last n elements: another phase of the walk at every size
    x, r = px[off:], ret[off:]
    ddof = window % 2 if window > 1 else 0
    rt = "log" if window % 2 else "simple"
    equal(P.sma(x, window), H.sma(x, window), f"sma n={n} w={window}")
    equal(P.comp_zscore(r, window, ddof), H.comp_zscore(r, window, ddof), f"zscore n={n} w={window}")
    equal(P.rolling_variance_nb(r, window, ddof, 1), H.rolling_variance_nb(r, window, ddof, 1), f"variance n={n} w={window}")
    # the ratio's series start four elements earlier where there are any, so that its first tile is full as well
    xr = px[max(0, off - 4):]
    want = H.variance_ratio_1_4_core(xr, window, ddof, rt)
    equal(P.variance_ratio_1_4_core(xr, window, ddof, rt), want, f"ratio n={len(xr)} w={window}")
    if n >= window + 8 and window >= 63:
        assert np.isfinite(want[window + 3:]).all(), (n, window)
    _counts.record(f"rolling/geometry/n{n}_w{window}", outputs_compared=3 * n + len(xr), windows=max(0, n - window + 1))


PLANT_WINDOW = 8500                  # three slabs: a span of 8499 + TILE = 9523 elements for the first tile


@pytest.mark.parametrize("p", (0, BLOCK - 1, BLOCK, TILE - 1, TILE, SLAB - 1, SLAB, SLAB + BLOCK - 1, 2 * SLAB - 1, 2 * SLAB,
                               PLANT_WINDOW - 1 + TILE - 1))
def test_sma_sees_a_planted_element_in_exactly_its_windows(p):
    """Ones with one 3.0 at span position p of the first tile, two tiles of outputs: the sums are exact integers, 8502 for a window
    that holds the 3.0 and 8500 for any other; a read skipped or made twice gives another integer."""
    window, n = PLANT_WINDOW, PLANT_WINDOW - 1 + 2 * TILE
    x = np.ones(n)
    x[p] = 3.0
    t = np.arange(n)
    holds = (t >= p) & (t < p + window)
    closed = np.where(t < window - 1, np.nan, (1.0 / window) * np.where(holds, window + 2.0, float(window)))
    want = H.sma(x, window)
    assert np.array_equal(want, closed, equal_nan=True) and 0 < holds[window - 1:].sum()
    equal(product().sma(x, window), want, f"sma, 3.0 planted at {p}")
    _counts.record(f"rolling/planted/sma_p{p}", outputs_compared=n)


def test_nan_runs_across_a_tile_edge(series):
    """Variance and ratio: NaN runs shorter and longer than the window on both sides of the first and the second tile edge."""
    px, ret = series
    P = product()
    window, n = 20, 3 * TILE
    edge = window - 1 + TILE                                     # the first output of the second tile
    for base, fn_pair in ((ret, "variance"), (px, "ratio")):
        x = np.array(base[:n])
        x[edge - 3:edge + 3] = np.nan                            # shorter than the window, over the edge
        x[edge + TILE - 25:edge + TILE + 15] = np.nan            # longer, over the next edge
        x[edge - window] = np.nan                                # leaves the window exactly at the edge
        if fn_pair == "variance":
            for ddof, mp in ((1, 1), (0, window), (1, window - 5)):
                want = H.rolling_variance_nb(x, window, ddof, mp)
                equal(P.rolling_variance_nb(x, window, ddof, mp), want, f"variance ddof={ddof} mp={mp}")
                assert np.isnan(want[edge + TILE - 5:edge + TILE + 14]).all() and np.isfinite(want[edge + TILE + 40:]).all()
        else:
            for rt in ("log", "simple"):
                want = H.variance_ratio_1_4_core(x, window, 0, rt)
                equal(P.variance_ratio_1_4_core(x, window, 0, rt), want, f"ratio {rt}")
                assert np.isnan(want[edge + TILE:edge + TILE + 14]).all() and np.isfinite(want[edge - 6:edge + 6]).all()
    _counts.record("rolling/nan_runs", outputs_compared=5 * n)


def test_held_prices_across_a_tile_edge(series):
    """z-score: runs of equal prices whose flat windows lie on both sides of a tile edge.  A price the sum of 20 copies of which is
    exact (101.5) has a mean equal to itself and a standard deviation of exactly 0 -> NaN; a price such as 90.89 has a mean one
    rounding away from itself, a tiny non-zero deviation, and a z-score of about -1: both are the reference's bits."""
    px, _ = series
    P = product()
    window, n = 20, 2 * TILE + 100
    edge = window - 1 + TILE
    flat = list(range(edge - 30 + window - 1, edge + 20))           # the windows that hold the held price alone
    for held in (101.5, None):
        x = np.array(px[:n])
        x[edge - 30:edge + 20] = x[edge - 30] if held is None else held
        for ddof in (0, 1):
            want = H.comp_zscore(x, window, ddof)
            equal(P.comp_zscore(x, window, ddof), want, f"zscore held={held} ddof={ddof}")
            nan_at = list(np.nonzero(np.isnan(want[window - 1:]))[0] + window - 1)
            if held is None:
                assert not nan_at and len(set(want[flat])) == 1 and 0.9 < abs(want[flat[0]]) < 1.1
            else:
                assert nan_at == flat and flat[0] < edge < flat[-1]
        want = H.rolling_variance_nb(x, window, 1, 1)
        equal(P.rolling_variance_nb(x, window, 1, 1), want, f"variance held={held}")
        assert (want[flat] == 0.0).all()
    _counts.record("rolling/held", outputs_compared=6 * n)


# ---------------------------------------------------------------------------------------------- transforms and the resident flow
def test_transforms_and_compose(series):
    import pandas as pd
    from finmlkit_amd.feature.core.utils import comp_lagged_returns
    from finmlkit_amd.feature.transforms import SMA, Compose, ReturnT, VarianceRatio14, ZScore
    px, _ = series
    n = 5000
    frame = pd.DataFrame({"px": np.array(px[:n])}, index=pd.date_range("2024-01-01", periods=n, freq="1s"))
    x = frame["px"].values
    for tr, want in ((SMA(7, input_col="px"), H.sma(x, 7)), (ZScore(30, "px", ddof=1), H.comp_zscore(x, 30, 1)),
                     (VarianceRatio14(input_col="px"), H.variance_ratio_1_4_core(x, 32, 0, "log")),
                     (VarianceRatio14(window=50, input_col="px", ret_type="simple", ddof=1), H.variance_ratio_1_4_core(x, 50, 1, "simple"))):
        for backend in ("nb", "pd"):
            s = tr(frame, backend=backend)
            assert s.name == tr.output_name and s.index.equals(frame.index)
            equal(s.values, want, tr.output_name)
    ret = ReturnT(pd.Timedelta(seconds=5), is_log=True, input_col="px")
    lagged = comp_lagged_returns(frame.index.values.astype(np.int64), x, 5.0, True)
    assert np.isnan(lagged[:5]).all() and np.isfinite(lagged[5:]).all()
    for second, want in ((ZScore(50, "ret"), H.comp_zscore(lagged, 50, 0)), (SMA(64, "ret"), H.sma(lagged, 64))):
        chain = Compose(ret, second)
        s = chain(frame)                                         # the device-resident path: ReturnT._dev -> the moment's _dev
        assert s.name == chain.output_name == f"px_ret5.0s_{second.produces[0]}"
        equal(s.values, want, chain.output_name)
        assert np.isnan(want[:second.window + 4]).all() and np.isfinite(want[second.window + 4:]).all()
    with pytest.raises(ValueError, match="window - ddof"):
        Compose(ret, ZScore(3, "ret", ddof=3))(frame)
    _counts.record("rolling/transforms", outputs_compared=10 * n)


def test_device_trades_methods(series):
    from finmlkit_amd import engine
    from finmlkit_amd._ffi import DeviceArray
    px, ret = series
    n = 6000
    x, r = np.array(px[:n]), np.array(ret[:n])
    P = product()
    t = engine.DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), x, np.ones(n, np.float32))
    y = DeviceArray.from_host(t.ctx, r)
    with pytest.raises(TypeError, match="float64"):
        t.sma(DeviceArray.from_host(t.ctx, r.astype(np.float32)), 5)
    got = {"sma": t.sma(y, 100), "zscore": t.zscore(y, 100), "zscore1": t.zscore(y, 100, ddof=1),
           "variance": t.rolling_variance(y, 100), "variance_mp": t.rolling_variance(y, 100, ddof=0, min_periods=100),
           "ratio": t.variance_ratio_1_4(), "ratio_series": t.variance_ratio_1_4(50, 1, "simple", series=y)}
    want = {"sma": P.sma(r, 100), "zscore": P.comp_zscore(r, 100, 0), "zscore1": P.comp_zscore(r, 100, 1),
            "variance": P.rolling_variance_nb(r, 100), "variance_mp": P.rolling_variance_nb(r, 100, 0, 100),
            "ratio": P.variance_ratio_1_4_core(x, 32, 0, "log"), "ratio_series": P.variance_ratio_1_4_core(r, 50, 1, "simple")}
    for k, g in got.items():
        assert isinstance(g, DeviceArray) and g.dtype == np.float64 and g.n == n, k
        equal(g.to_host(), want[k], k)                           # the results come down once, for the comparison
    equal(want["ratio"], H.variance_ratio_1_4_core(x, 32, 0, "log"), "ratio against the restatement")
    _counts.record("rolling/resident", outputs_compared=len(got) * n)
