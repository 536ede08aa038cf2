"""The window statistics on the MI355X -- rolling_kurtosis, trend_slope, hurst_exponent, bipower_variation (csrc/fmk_shape.hip) --
against the reference's recorded outputs (tests/golden/shape.npz) and the NumPy-form restatement of tests/_shape_ref.py: NaN
positions exactly, the values within the tolerances of shape.json, which were measured on the CPU between the reference and the
restatement (times 16, rounded up to a power of ten; absolute for kurtosis, hurst and the slope in degrees, relative for bipower)."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _rolling_ref as R
from tests import _shape_ref as H
from tests.test_shape_host import MANIFEST, OK_CASES, REFUSED, case_input, close, expected, product

pytestmark = pytest.mark.gpu

BLOCK = 256                                                        # lanes per workgroup (csrc/fmk_shape.hip: SHAPE_BLOCK)
TILE = {"kurtosis": 1024, "slope": 1024, "bipower": 1024, "hurst": 512}      # outputs per workgroup (SHAPE_TILE, HURST_TILE)
SLAB = {"kurtosis": 4096, "slope": 4096, "bipower": 4096, "hurst": 1024}     # LDS words per staging (FMK_SLAB_MAX, FMK_SLAB_MAX32)
LONG_WINDOW = {"kurtosis": 4100, "slope": 4100, "bipower": 4100, "hurst": 1100}   # a full tile's span takes more than one slab
ENTRY = {fn: "fmk_" + H.PRODUCT_NAMES[fn] for fn in H.FUNCTIONS}
SERIES_N = 8000


def dev_call(fn, x, window, ctx=None):
    """The `_dev` entry on a resident copy of the series -> host array."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = ctx or _ffi.default_context()
    d_x = DeviceArray.from_host(ctx, np.ascontiguousarray(x, dtype=np.float64))
    out = DeviceArray(ctx, len(x), np.float64)
    ctx.call(ENTRY[fn] + "_dev", d_x.p, C.c_int64(len(x)), C.c_int64(window), out.p)
    return out.to_host()


@pytest.fixture(scope="module")
def series():
    """One seeded series per kind of input, shared by the tests below (never written to)."""
    px, ret = H.grid_walk(SERIES_N, 1501), H.mantissa_returns(SERIES_N, 1502)
    px.setflags(write=False)
    ret.setflags(write=False)
    return {"slope": px, "kurtosis": ret, "hurst": ret, "bipower": ret}


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay(name):
    c, x = MANIFEST[name], case_input(name)
    devs = [close(c["fn"], product(c["fn"])(x, c["window"]), expected(name), name + " (python)"),
            close(c["fn"], dev_call(c["fn"], x, c["window"]), expected(name), name + " (_dev)")]
    print(name, "deviation from the reference", max(devs))
    _counts.record(f"shape/fixture/{name}", outputs_compared=2 * c["n"], finite=c["finite"])


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    c, x = MANIFEST[name], case_input(name)
    ctx = _ffi.default_context()
    with pytest.raises(ValueError) as e:
        dev_call(c["fn"], x, c["window"])
    assert c["message"] in str(e.value)
    out = np.zeros(len(x))
    lib = _ffi.lib()
    rc = getattr(lib, ENTRY[c["fn"]])(ctx.handle, _ffi.ptr(x), C.c_int64(len(x)), C.c_int64(c["window"]), _ffi.ptr(out))
    assert rc == _ffi.E_ARG
    rc = getattr(lib, ENTRY[c["fn"]] + "_dev")(ctx.handle, None, C.c_int64(len(x)), C.c_int64(c["window"]), None)
    assert rc == _ffi.E_ARG                      # refused before any pointer is looked at


# ---------------------------------------------------------------------------------------------- geometry
def _lengths(fn, w):
    """n with 0, 1, 2, T - 1, T, T + 1 and 2 T + 1 outputs (for bipower, whose first output is one later, also one fewer)."""
    t = TILE[fn]
    counts = (0, 1, 2, t - 1, t, t + 1, 2 * t + 1)
    return sorted({w - 1 + m for m in counts} | {H.first_output(fn, w) + m for m in counts})


GEOMETRY = [(fn, n, w) for fn in H.FUNCTIONS for w in (1, 2, 3, 9, 10, 11, 63, 64, 65)
            if not (fn == "hurst" and w < H.HURST_MIN_WINDOW) for n in _lengths(fn, w)]
GEOMETRY += [(fn, LONG_WINDOW[fn] + 2 * TILE[fn] + 1, LONG_WINDOW[fn]) for fn in H.FUNCTIONS]
GEOMETRY += [(fn, SLAB[fn] + 1, SLAB[fn] - TILE[fn] + 1 + d) for fn in H.FUNCTIONS for d in (0, 1, 2)]   # a full tile's span about one slab
GEOMETRY += [(fn, 5, 12) for fn in H.FUNCTIONS]                     # n < window


@pytest.mark.parametrize("fn,n,window", GEOMETRY)
def test_geometry(series, fn, n, window):
    x = series[fn][len(series[fn]) - n:]                            # the last n elements: another phase of the walk at every size
    want = H.call(fn, x, window)
    tail = want[H.first_output(fn, window):]
    if not ((fn, window) in (("kurtosis", 1), ("slope", 1), ("hurst", 9))):
        assert np.isfinite(tail).all(), (fn, n, window)             # agreement alone would pass on an all-NaN output
    else:
        assert np.isnan(want).all()
    dev = close(fn, product(fn)(x, window), want, f"{fn} n={n} w={window}")
    print(fn, n, window, "deviation from the restatement", dev)
    _counts.record(f"shape/geometry/{fn}_n{n}_w{window}", outputs_compared=n, finite=int(np.isfinite(want).sum()))


def test_empty_series():
    from finmlkit_amd import _ffi
    ctx = _ffi.default_context()
    for fn in H.FUNCTIONS:
        r = product(fn)(np.empty(0), 12)
        assert r.dtype == np.float64 and r.shape == (0,)
        assert getattr(_ffi.lib(), ENTRY[fn] + "_dev")(ctx.handle, None, C.c_int64(0), C.c_int64(12), None) == 0


@pytest.mark.parametrize("long_window", (False, True))
@pytest.mark.parametrize("fn", H.FUNCTIONS)
def test_nan_geometry(series, fn, long_window):
    """One refused element (NaN, and once an infinity) where the walk changes hands: the last output of the first tile and the first
    of the second, lanes 63 and 64 of the first wave, and -- at the long window -- the last word of the first slab and the first of
    the second.  Exactly the windows that read it are NaN."""
    t, first_w = TILE[fn], 20
    w = LONG_WINDOW[fn] if long_window else first_w
    first = H.first_output(fn, w)
    n = first + 2 * t + 1
    base = series[fn][:n]
    spots = [first + t - 1, first + t, first + 63, first + 64, 0, 1, n - 1]
    if long_window:
        spots += [SLAB[fn] - 1, SLAB[fn], SLAB[fn] + 1]
    reach = w + 1 if fn == "bipower" else w
    for k, spot in enumerate(spots):
        x = np.array(base)
        x[spot] = np.inf if k == 2 else np.nan
        want = H.call(fn, x, w)
        nan = np.zeros(n, bool)
        nan[:reach - 1] = True
        nan[spot:spot + reach] = True
        assert np.array_equal(np.isnan(want), nan), (fn, w, spot)
        close(fn, product(fn)(x, w), want, f"{fn} w={w} refused element at {spot}")
    _counts.record(f"shape/nan_geometry/{fn}_w{w}", outputs_compared=n * len(spots))


# ---------------------------------------------------------------------------------------------- the resident flow and the transforms
def _resident(x):
    from finmlkit_amd import engine
    from finmlkit_amd._ffi import DeviceArray
    n = len(x)
    t = engine.DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), np.ones(n), np.ones(n, np.float32))
    return t, DeviceArray.from_host(t.ctx, np.ascontiguousarray(x, dtype=np.float64))


def test_resident_chain(series):
    from finmlkit_amd._ffi import DeviceArray
    n = 3000
    for fn, method, w in (("kurtosis", "kurtosis", 32), ("slope", "trend_slope", 24), ("hurst", "hurst_exponent", 24),
                          ("bipower", "bipower_variation", 12)):
        x = np.array(series[fn][:n])
        t, d_x = _resident(x)
        smooth = t.sma(d_x, 5)                                      # a series made on the device: NaN before index 4
        got = getattr(t, method)(smooth, w)
        assert isinstance(got, DeviceArray) and got.dtype == np.float64 and got.n == n
        want = H.call(fn, R.sma(x, 5), w)
        assert np.isfinite(want[w + 4:]).all() and np.isnan(want[:w + 3]).all()
        close(fn, got.to_host(), want, f"resident chain {fn}")     # the result comes down once, for the comparison
        close(fn, got.to_host(), product(fn)(R.sma(x, 5), w), f"resident chain {fn} against the host function")
        with pytest.raises(TypeError, match="float64"):
            getattr(t, method)(DeviceArray.from_host(t.ctx, x.astype(np.float32)), w)
        with pytest.raises(ValueError, match="window must be at least"):
            getattr(t, method)(d_x, 0)
    with pytest.raises(ValueError, match=r"^hurst_exponent: window must be at least 9\.$"):
        t.hurst_exponent(d_x, 8)
    _counts.record("shape/resident", outputs_compared=8 * n)


def test_transforms_and_compose_chain(series):
    import pandas as pd
    from finmlkit_amd.feature import transforms as T
    from finmlkit_amd.feature.core.utils import comp_lagged_returns
    n = 3000
    px = np.array(series["slope"][:n])
    index = pd.date_range("2024-01-01", periods=n, freq="1s")
    frame = pd.DataFrame({"close": px, "ret1": np.array(series["kurtosis"][:n])}, index=index)
    for fn, tr in (("kurtosis", T.KurtosisTransform()), ("slope", T.TrendSlope()), ("hurst", T.HurstExponent()),
                   ("bipower", T.BiPowerVariation()), ("kurtosis", T.KurtosisTransform(100, "close"))):
        host = product(fn)(frame[tr.requires[0]].values, tr.window)
        close(fn, host, H.call(fn, frame[tr.requires[0]].values, tr.window), tr.output_name)
        for backend in ("nb", "pd"):
            s = tr(frame, backend=backend)
            assert s.name == tr.output_name and s.index.equals(frame.index)
            close(fn, s.values, host, tr.output_name)
    ret = comp_lagged_returns(index.values.astype(np.int64), px, 5.0, True)
    for fn, tr in (("kurtosis", T.KurtosisTransform(32, "ret5.0s")), ("hurst", T.HurstExponent(24, "ret5.0s")),
                   ("bipower", T.BiPowerVariation(12, "ret5.0s"))):
        pipe = T.Compose(T.ReturnT(pd.Timedelta(seconds=5), is_log=True, input_col="close"), tr)
        s = pipe(frame)
        assert s.name == "close_ret5.0s_" + tr.produces[0]
        host = product(fn)(ret, tr.window)
        assert np.isfinite(host).sum() > n - 60
        close(fn, s.values, host, s.name)
    got = T.Compose(T.SMA(5, "close"), T.TrendSlope(24, "sma5"))(frame)
    close("slope", got.values, product("slope")(R.sma(px, 5), 24), "Compose(SMA, TrendSlope)")
    with pytest.raises(ValueError, match=r"^hurst_exponent: window must be at least 9\.$"):
        T.Compose(T.SMA(5, "close"), T.HurstExponent(8, "sma5"))(frame)
    with pytest.raises(ValueError, match=r"^window must be at least 1\.$"):
        T.KurtosisTransform(0)(frame)
    _counts.record("shape/transforms", outputs_compared=19 * n)
