"""The rolling approximate entropy on the MI355X (csrc/fmk_entropy.hip) against the reference path's recorded outputs
(tests/golden/entropy.npz) and the kernel-order restatement of tests/_entropy_ref.py: NaN positions exactly, the values within the
tolerance of entropy.json, which was measured on the CPU between the reference path and the restatement (times 16, rounded up to a
power of ten).  Every series compared with the restatement is first shown to have no window on a knife edge (a pair within
2^-40 r of r), where a last-bit difference in r would flip a count."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _entropy_ref as E
from tests import _rolling_ref as R
from tests._shape_ref import grid_walk
from tests.test_entropy_host import MANIFEST, OK_CASES, REFUSED, case_args, case_input, close, expected, product

pytestmark = pytest.mark.gpu

TILE = 256                                                         # outputs, and lanes, per workgroup (csrc/fmk_entropy.hip: APEN_BLOCK)
MASK_WINDOW = 64                                                   # the longest window of the row-mask path (APEN_MASK_WINDOW)
SERIES_N = 1100


def dev_call(x, window, m, tolerance, ctx=None):
    """The `_dev` entry on a resident copy of the series -> host array."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = ctx or _ffi.default_context()
    d_x = DeviceArray.from_host(ctx, np.ascontiguousarray(x, dtype=np.float64))
    out = DeviceArray(ctx, len(x), np.float64)
    ctx.call("fmk_approximate_entropy_dev", d_x.p, C.c_int64(len(x)), C.c_int64(window), C.c_int64(m), C.c_double(tolerance), out.p)
    return out.to_host()


@pytest.fixture(scope="module")
def series():
    """One seeded series per kind of input, shared by the tests below (never written to): returns on the dyadic grid, which tie at
    distance 0, returns that use the whole mantissa, and a price walk."""
    out = {"dyadic": E.dyadic_returns(SERIES_N, 1801), "mantissa": E.mantissa_returns(SERIES_N, 1802), "price": grid_walk(3000, 1803)}
    for v in out.values():
        v.setflags(write=False)
    return out


def restated(x, window, m=2, tolerance=0.2):
    """The kernel-order restatement, after the check that it is a fair yardstick for this series."""
    assert not E.knife_edge(x, window, m, tolerance).any(), ("a window on a knife edge: choose another seed", window, m, tolerance)
    return E.approximate_entropy(x, window, m, tolerance)


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay(name):
    c, x = MANIFEST[name], case_input(name)
    w, m, tol = case_args(name)
    devs = [close(product()(x, w, m, tol), expected(name), name + " (python)")]
    if c["n"]:
        devs.append(close(dev_call(x, w, m, tol), expected(name), name + " (_dev)"))
    print(name, "deviation from the reference path", max(devs))
    _counts.record(f"entropy/fixture/{name}", outputs_compared=2 * c["n"], finite=c["finite"])


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    c, x = MANIFEST[name], case_input(name)
    w, m, tol = case_args(name)
    ctx = _ffi.default_context()
    with pytest.raises(ValueError) as e:
        dev_call(x, w, m, tol)
    assert c["message"] in str(e.value)
    out = np.zeros(len(x))
    lib = _ffi.lib()
    args = (C.c_int64(len(x)), C.c_int64(w), C.c_int64(m), C.c_double(tol))
    assert lib.fmk_approximate_entropy(ctx.handle, _ffi.ptr(x), *args, _ffi.ptr(out)) == _ffi.E_ARG
    assert lib.fmk_approximate_entropy(ctx.handle, None, *args, None) == _ffi.E_ARG
    assert lib.fmk_approximate_entropy_dev(ctx.handle, None, *args, None) == _ffi.E_ARG      # refused before any pointer is looked at
    assert (out == 0.0).all()


# ---------------------------------------------------------------------------------------------- geometry
def _lengths(w):
    """n with 0, 1, 2, T - 1, T, T + 1 and 2 T + 1 outputs."""
    return [w - 1 + k for k in (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]


GEOMETRY = [(m, n, w) for m in (1, 2, E.MAX_M) for w in (m + 1, m + 2, 24, 63, 64, 65, 66) for n in _lengths(w)]
GEOMETRY += [(m, E.MAX_WINDOW + 3, E.MAX_WINDOW) for m in (1, 2, E.MAX_M)]      # n = window + 3: the brute-force oracle stays fast


@pytest.mark.parametrize("m,n,window", GEOMETRY)
def test_geometry(series, m, n, window):
    base = series["dyadic"] if m == 1 else series["mantissa"]       # at m = 1 single ties count
    x = base[len(base) - n:]                                        # the last n elements: another phase at every size
    want = restated(x, window, m)
    assert np.isnan(want[:window - 1]).all() and np.isfinite(want[window - 1:]).all(), (m, n, window)
    dev = close(product()(x, window, m), want, f"m={m} n={n} w={window}")
    print(m, n, window, "deviation from the restatement", dev)
    _counts.record(f"entropy/geometry/m{m}_n{n}_w{window}", outputs_compared=n, finite=int(np.isfinite(want).sum()))


def test_empty_series():
    from finmlkit_amd import _ffi
    ctx = _ffi.default_context()
    r = product()(np.empty(0), 12)
    assert r.dtype == np.float64 and r.shape == (0,)
    args = (C.c_int64(0), C.c_int64(12), C.c_int64(2), C.c_double(0.2))
    assert _ffi.lib().fmk_approximate_entropy_dev(ctx.handle, None, *args, None) == 0
    assert _ffi.lib().fmk_approximate_entropy(ctx.handle, None, *args, None) == 0


@pytest.mark.parametrize("window", (20, 70))
def test_nan_geometry(series, window):
    """One refused element (a NaN, then an infinity) where the tile and the wave change hands: the last output of the first tile and
    the first of the second, lanes 63 and 64 of the first wave, and the ends of the series.  Exactly the windows that read it are
    NaN.  Window 20 takes the row-mask path, window 70 the plain one."""
    assert (window <= MASK_WINDOW) == (window == 20)
    first = window - 1
    n = first + 2 * TILE + 1
    base = series["mantissa"][:n]
    spots = [first + TILE - 1, first + TILE, first + 63, first + 64, 0, 1, n - 1]
    for k, spot in enumerate(spots):
        for bad in (np.nan, -np.inf if k % 2 else np.inf):
            x = np.array(base)
            x[spot] = bad
            want = restated(x, window)
            nan = np.zeros(n, bool)
            nan[:first] = True
            nan[spot:spot + window] = True
            assert np.array_equal(np.isnan(want), nan), (window, spot, bad)
            close(product()(x, window), want, f"w={window} {bad} at {spot}")
    _counts.record(f"entropy/nan_geometry/w{window}", outputs_compared=2 * n * len(spots))


def test_exact_zeros(series):
    """A flat series, and a tolerance under which every pair matches, give 0.0 exactly, with no NaN past the head."""
    n = 2 * TILE + 40
    for window, m in ((3, 2), (24, 2), (64, E.MAX_M), (70, 1), (E.MAX_WINDOW, 2)):
        n_w = max(n, window + 3) if window < E.MAX_WINDOW else window + 3
        for x, tol in ((np.zeros(n_w), 0.2), (np.full(n_w, 0.375), 0.2), (np.full(n_w, -3.0), 0.0), (series["mantissa"][:n_w], 1e6)):
            got = product()(x, window, m, tol)
            assert np.isnan(got[:window - 1]).all(), (window, m, tol)
            assert (got[window - 1:] == 0.0).all() and not np.signbit(got[window - 1:]).any(), (window, m, tol)
    _counts.record("entropy/exact_zeros", outputs_compared=20 * n)


# ---------------------------------------------------------------------------------------------- the resident flow and the transform
def _resident(x):
    from finmlkit_amd import engine
    from finmlkit_amd._ffi import DeviceArray
    n = len(x)
    t = engine.DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), np.ones(n), np.ones(n, np.float32))
    return t, DeviceArray.from_host(t.ctx, np.ascontiguousarray(x, dtype=np.float64))


def test_resident_chain(series):
    from finmlkit_amd._ffi import DeviceArray
    x = np.array(series["mantissa"])
    n = len(x)
    t, d_x = _resident(x)
    smooth = t.sma(d_x, 5)                                          # a series made on the device: NaN before index 4
    for w, m, tol in ((24, 2, 0.2), (70, 3, 0.5)):
        got = t.approximate_entropy(smooth, w, m, tol)
        assert isinstance(got, DeviceArray) and got.dtype == np.float64 and got.n == n
        want = restated(R.sma(x, 5), w, m, tol)
        assert np.isfinite(want[w + 3:]).all() and np.isnan(want[:w + 3]).all()
        close(got.to_host(), want, f"resident chain w={w}")        # the result comes down once, for the comparison
        close(got.to_host(), product()(R.sma(x, 5), w, m, tol), f"resident chain w={w} against the host function")
    got = t.approximate_entropy(smooth, 24)                         # the defaults: m = 2, tolerance = 0.2
    close(got.to_host(), restated(R.sma(x, 5), 24), "resident chain, defaults")
    with pytest.raises(TypeError, match="float64"):
        t.approximate_entropy(DeviceArray.from_host(t.ctx, x.astype(np.float32)), 24)
    for args, message in (((24, 0), E.M_MESSAGE), ((24, E.MAX_M + 1), E.MAX_M_MESSAGE), ((2, 2), E.WINDOW_MESSAGE),
                          ((E.MAX_WINDOW + 1,), E.MAX_WINDOW_MESSAGE), ((24, 2, -0.1), E.TOLERANCE_MESSAGE)):
        with pytest.raises(ValueError) as e:
            t.approximate_entropy(d_x, *args)
        assert str(e.value) == message
    _counts.record("entropy/resident", outputs_compared=5 * n)


def test_transform_and_compose_chain(series):
    import pandas as pd
    from finmlkit_amd.feature import transforms as T
    from finmlkit_amd.feature.core.utils import comp_lagged_returns
    n = 3000
    px = np.array(series["price"][:n])
    ret1 = np.resize(series["mantissa"], n)
    index = pd.date_range("2024-01-01", periods=n, freq="1s")
    frame = pd.DataFrame({"close": px, "ret1": ret1}, index=index)
    for tr in (T.ApproximateEntropy(), T.ApproximateEntropy(70, 3, 0.5), T.ApproximateEntropy(30, 1, 0.2, "close")):
        col = frame[tr.requires[0]].values
        host = product()(col, tr.window, tr.m, tr.tolerance)
        close(host, restated(col, tr.window, tr.m, tr.tolerance), tr.output_name)
        assert np.isfinite(host[tr.window - 1:]).all()
        for backend in ("nb", "pd"):
            s = tr(frame, backend=backend)
            assert s.name == tr.output_name == f"{tr.requires[0]}_apen{tr.window}" and s.index.equals(frame.index)
            close(s.values, host, tr.output_name)
    ret = comp_lagged_returns(index.values.astype(np.int64), px, 5.0, True)
    tr = T.ApproximateEntropy(24, 2, 0.2, "ret5.0s")
    s = T.Compose(T.ReturnT(pd.Timedelta(seconds=5), is_log=True, input_col="close"), tr)(frame)
    assert s.name == "close_ret5.0s_apen24" and s.index.equals(frame.index)
    host = product()(ret, 24)
    assert np.isfinite(host).sum() > n - 60
    close(s.values, host, s.name)
    close(host, restated(ret, 24), s.name + " against the restatement")
    got = T.Compose(T.SMA(5, "close"), T.ApproximateEntropy(24, 2, 0.2, "sma5"))(frame)
    assert got.name == "close_sma5_apen24"
    close(got.values, product()(R.sma(px, 5), 24), "Compose(SMA, ApproximateEntropy)")
    with pytest.raises(ValueError) as e:
        T.Compose(T.SMA(5, "close"), T.ApproximateEntropy(2, 2, 0.2, "sma5"))(frame)
    assert str(e.value) == E.WINDOW_MESSAGE
    with pytest.raises(ValueError) as e:
        T.ApproximateEntropy(24, 0)(frame)
    assert str(e.value) == E.M_MESSAGE
    _counts.record("entropy/transforms", outputs_compared=9 * n)
