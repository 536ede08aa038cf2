"""The rolling price-volume correlation on the MI355X -- rolling_price_volume_correlation (csrc/fmk_corr.hip) -- bit-equal
(np.array_equal, equal_nan=True) to the reference's recorded outputs (tests/golden/price_volume_corr.npz) and to the NumPy-form
restatement of tests/_corr_ref.py.  There is no tolerance: every operation is an IEEE addition, subtraction, product, quotient or
square root in the reference's order."""
import ctypes as C

import numpy as np
import pytest

from tests import _corr_ref as H
from tests import _counts
from tests import _rolling_ref as R
from tests.test_corr_host import MANIFEST, OK_CASES, REFUSED, case_input, expected, product

pytestmark = pytest.mark.gpu

BLOCK = 256                          # lanes per workgroup (csrc/fmk_corr.hip: CORR_BLOCK)
TILE = 1024                          # outputs per workgroup (CORR_TILE = CORR_BLOCK * CORR_OPL)
SLAB = 2048                          # 16-byte LDS words per staging (csrc/fmk_window.h: FMK_SLAB_MAX16)
ONE_SLAB_WINDOW = SLAB - TILE + 1    # the longest window whose full tile reads one slab (window - 1 + CORR_TILE <= FMK_SLAB_MAX16)
TWO_SLAB_WINDOW = 2 * SLAB - TILE + 1
THREE_SLAB_WINDOW = 5200             # a full tile's span of 6223 pairs: the slab 2048 .. 4095 lies wholly inside every window
SERIES_N = 20_001


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert np.array_equal(got, want, equal_nan=True), (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def dev_call(price, volume, window, ctx=None):
    """The `_dev` entry on resident copies of the two series -> host array."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = ctx or _ffi.default_context()
    n = len(price)
    d_p, d_v = (DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=np.float64)) for a in (price, volume))
    out = DeviceArray(ctx, n, np.float64)
    ctx.call("fmk_price_volume_corr_dev", d_p.p, d_v.p, C.c_int64(n), C.c_int64(window), out.p)
    return out.to_host()


@pytest.fixture(scope="module")
def series():
    """One seeded grid walk and dyadic volumes, shared by the tests below (never written to)."""
    px, vol = H.grid_walk(SERIES_N, 911), H.dyadic_volumes(SERIES_N, 912)
    px.setflags(write=False)
    vol.setflags(write=False)
    return px, vol


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay(name):
    c, (p, v) = MANIFEST[name], case_input(name)
    equal(product()(p, v, c["window"]), expected(name), name + " (python)")
    if c["n"]:
        equal(dev_call(p, v, c["window"]), expected(name), name + " (_dev)")
    _counts.record(f"corr/fixture/{name}", outputs_compared=2 * c["n"], finite=c["finite"])


@pytest.mark.parametrize("name", [k for k in REFUSED if MANIFEST[k]["message"] == H.WINDOW_MESSAGE])
def test_refused_arguments_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    c, (p, v) = MANIFEST[name], case_input(name)
    ctx = _ffi.default_context()
    with pytest.raises(ValueError) as e:
        dev_call(p, v, c["window"])
    assert c["message"] in str(e.value)
    # the status itself, from the host-pointer and the device flavour
    out = np.zeros(len(p))
    lib = _ffi.lib()
    rc = lib.fmk_price_volume_corr(ctx.handle, _ffi.ptr(p), _ffi.ptr(v), C.c_int64(len(p)), C.c_int64(c["window"]), _ffi.ptr(out))
    assert rc == _ffi.E_ARG
    rc = lib.fmk_price_volume_corr_dev(ctx.handle, None, None, C.c_int64(len(p)), C.c_int64(c["window"]), None)
    assert rc == _ffi.E_ARG                      # refused before any pointer is looked at


# ---------------------------------------------------------------------------------------------- geometry
def _outputs(window, counts):
    return [(window + m, window) for m in counts]


GEOMETRY = []
for _w in (1, 2, 63, 64, 65):                                  # wave edges; one tile +-1 and two tiles + 1 of outputs
    GEOMETRY += _outputs(_w, (TILE - 1, TILE, TILE + 1, 2 * TILE + 1))
GEOMETRY += _outputs(3, (TILE + 1,)) + _outputs(8, (TILE + 1,))
for _w in (BLOCK - 1, BLOCK + 1, TILE - 1, TILE + 1):          # a lane's outputs are CORR_BLOCK apart; the tile size
    GEOMETRY += _outputs(_w, (TILE + 1,))
# a full tile's span of one slab - 1, one slab, one slab + 1, two slabs, two slabs + 1, about three slabs
for _w in (ONE_SLAB_WINDOW - 1, ONE_SLAB_WINDOW, ONE_SLAB_WINDOW + 1, TWO_SLAB_WINDOW, TWO_SLAB_WINDOW + 1, THREE_SLAB_WINDOW):
    GEOMETRY += _outputs(_w, (TILE + 1,))
GEOMETRY += [(66, 65), (65, 65), (1, 1)]
GEOMETRY = list(dict.fromkeys(GEOMETRY))                       # TILE + 1 is ONE_SLAB_WINDOW

# (+1.0, -1.0, NaN) among the outputs from `window` on, of the restatement on the last n elements of the shared series, at the windows
# where NaN and +-1 are the legitimate answers: window 1 is NaN but for the six special-case outputs, window 2 +-1 or just inside
SMALL_WINDOW_COUNTS = {
    (1024, 1): (6, 0, 1017), (1025, 1): (6, 0, 1018), (1026, 1): (6, 0, 1019), (2050, 1): (6, 0, 2043),
    (1025, 2): (418, 413, 0), (1026, 2): (419, 413, 0), (1027, 2): (419, 413, 0), (2051, 2): (811, 814, 0), (1028, 3): (0, 0, 0),
    (1, 1): (0, 0, 0),
}


@pytest.mark.parametrize("n,window", GEOMETRY)
def test_geometry(series, n, window):
    px, vol = series
    off = len(px) - n                                           # the last n elements: another phase of the walk at every size
    p, v = px[off:], vol[off:]
    want = H.rolling_price_volume_correlation(p, v, window)
    tail = want[window:]
    if window >= 8 and len(tail):
        # equality alone would pass on an all-NaN output: the restatement itself must be numbers
        assert (~np.isfinite(tail)).sum() <= 0.01 * len(tail), (n, window)
    if (n, window) in SMALL_WINDOW_COUNTS:
        assert ((tail == 1.0).sum(), (tail == -1.0).sum(), np.isnan(tail).sum()) == SMALL_WINDOW_COUNTS[(n, window)], (n, window)
    equal(product()(p, v, window), want, f"corr n={n} w={window}")
    _counts.record(f"corr/geometry/n{n}_w{window}", outputs_compared=n, windows=max(0, n - window), finite=int(np.isfinite(want).sum()))


@pytest.mark.parametrize("window", (20, TWO_SLAB_WINDOW + 1))
@pytest.mark.parametrize("m", (TILE - 1, TILE, TILE + 1, 2 * TILE + 1))
def test_nan_geometry(series, m, window):
    """About 10 % NaN in each series and NaN runs in the volumes ten longer than the window: one from element 1 on, and at the
    small window a second that ends where the second tile begins (or three elements before the end of a shorter series).  Inside a
    run the windows hold no valid pair; the output after it has one, its own (NaN), the next one two, and so on up to the window:
    at the multi-slab window every count from 1 on occurs, in windows that span the slab edges."""
    px, vol = series
    n = window + m
    off = len(px) - n
    p, v = np.array(px[off:]), np.array(vol[off:])
    rng = np.random.default_rng(1000 * window + m)
    p[rng.random(n) < 0.1] = np.nan
    v[rng.random(n) < 0.1] = np.nan
    ends = [window + 11] + ([min(window + TILE, n - 3)] if window < TILE else [])
    for end in ends:
        v[end - (window + 10):end] = np.nan
        p[end - 2:end + 3], v[end:end + 3] = px[off + end - 2:off + end + 3], vol[off + end:off + end + 3]
    want = H.rolling_price_volume_correlation(p, v, window)
    for end in ends:
        assert np.isnan(want[end - (window + 10):end + 1]).all() and np.isfinite(want[end + 1:end + 3]).all(), end
    assert np.isfinite(want[window:]).sum() > 0.6 * m
    equal(product()(p, v, window), want, f"corr with NaN n={n} w={window}")
    _counts.record(f"corr/nan_geometry/n{n}_w{window}", outputs_compared=n, finite=int(np.isfinite(want).sum()))


# ---------------------------------------------------------------------------------------------- the six special-case outputs
def _resident(*host):
    from finmlkit_amd import engine
    from finmlkit_amd._ffi import DeviceArray
    n = len(host[0])
    t = engine.DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), np.ones(n), np.ones(n, np.float32))
    return t, [DeviceArray.from_host(t.ctx, np.ascontiguousarray(a, dtype=np.float64)) for a in host]


@pytest.mark.parametrize("window", range(1, 11))
def test_the_six_special_outputs(window):
    """Strictly rising prices whose returns rise too, and volumes that are an exact affine function of the returns, rising or
    falling: outputs 4 .. 9 are the special case's +-1.0; outputs 10 and 11 are the standard path's, +-1 up to the rounding of the
    sums -- exactly 1.0 only through the clamp, or just inside."""
    n = 12
    price = 10.0 * np.cumprod(1.0 + 0.01 * np.arange(1, n + 1))
    ret = H.returns(price)
    ret[0] = 0.0
    vol_up = 100.0 + 10000.0 * ret
    for vol, sign in ((vol_up, 1.0), (1000.0 - vol_up, -1.0)):
        want = H.rolling_price_volume_correlation(price, vol, window)
        assert np.array_equal(want, H.rolling_price_volume_correlation(price, vol, window, form="scalar"), equal_nan=True)
        lo = max(window, 4)
        assert (want[lo:10] == (1.0 if window == 1 else sign)).all() and np.isnan(want[:window]).all()
        if window == 1:
            assert np.isnan(want[10:]).all()
        else:
            assert (np.abs(want[10:]) <= 1.0).all() and (sign * want[10:] > 1.0 - 1e-9).all()
        t, (d_p, d_v) = _resident(price, vol)
        got = t.price_volume_corr(d_p, d_v, window)
        assert got.dtype == np.float64 and got.n == n
        equal(got.to_host(), want, f"special case, window {window}, sign {sign}")
    _counts.record(f"corr/special/w{window}", outputs_compared=2 * n)


# ---------------------------------------------------------------------------------------------- the transform and the resident flow
def test_resident_chain_and_transform(series):
    import pandas as pd
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.feature.transforms import PriceVolumeCorrelation
    px, vol = series
    n = 6000
    p, v = np.array(px[:n]), np.array(vol[:n])
    t, (d_p, d_v) = _resident(p, v)
    smooth = t.sma(d_v, 5)                                       # a volume series made on the device: NaN before index 4
    got = t.price_volume_corr(d_p, smooth, 100)
    assert isinstance(got, DeviceArray) and got.dtype == np.float64 and got.n == n
    want = H.rolling_price_volume_correlation(p, R.sma(v, 5), 100)
    equal(got.to_host(), want, "resident chain")                 # the result comes down once, for the comparison
    assert np.isfinite(want[100:]).all()
    with pytest.raises(TypeError, match="float64"):
        t.price_volume_corr(d_p, DeviceArray.from_host(t.ctx, v.astype(np.float32)), 5)
    frame = pd.DataFrame({"close": p, "volume": v, "px": p[::-1].copy()}, index=pd.date_range("2024-01-01", periods=n, freq="1min"))
    for tr, cols in ((PriceVolumeCorrelation(), ("close", "volume")), (PriceVolumeCorrelation(30, ["px", "volume"]), ("px", "volume"))):
        fn = product()(frame[cols[0]].values, frame[cols[1]].values, tr.window)
        equal(fn, H.rolling_price_volume_correlation(frame[cols[0]].values, frame[cols[1]].values, tr.window), tr.output_name)
        for backend in ("nb", "pd"):
            s = tr(frame, backend=backend)
            assert s.name == f"corr_pv_{tr.window}" and s.index.equals(frame.index)
            equal(s.values, fn, tr.output_name)
    _counts.record("corr/resident", outputs_compared=6 * n)
