"""The CSW CUSUM structural-break test on the MI355X: four float64 arrays, bit-equal (np.array_equal, equal_nan=True) to the
reference's recorded outputs (tests/golden/cusum_test.npz) and to the plain restatement of tests/_break_ref.py.  There is no
tolerance: every operation is an IEEE subtraction, product, quotient or square root, or the host's log."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import _break_ref as H
from tests import _counts
from tests.test_break_host import MANIFEST, NAMES, OK_CASES, RAISING, _NPZ, call, case_input, expected

pytestmark = pytest.mark.gpu

WARMUP = 30
TILE = 256                           # outputs per workgroup (csrc/fmk_break.hip: BRK_TILE)
SLAB_MAX = 4096                      # LDS elements per staging (BRK_SLAB_MAX)
DIAG = ("outputs", "pairs", "slabs", "quotients", "slab", "tiles")


class slab:
    """FMK_BREAK_SLAB for the duration of a block (None: the library's own)."""

    def __init__(self, elements):
        self.elements = elements

    def __enter__(self):
        self.old = os.environ.pop("FMK_BREAK_SLAB", None)
        if self.elements:
            os.environ["FMK_BREAK_SLAB"] = str(self.elements)

    def __exit__(self, *a):
        os.environ.pop("FMK_BREAK_SLAB", None)
        if self.old is not None:
            os.environ["FMK_BREAK_SLAB"] = self.old


def P():
    from finmlkit_amd.feature.core import structural_break
    return structural_break


def diag_last():
    from finmlkit_amd import _ffi
    out = (C.c_int64 * 6)()
    _ffi.default_context().call("fmk_diag_cusum_test_last", out)
    return dict(zip(DIAG, (int(v) for v in out)))


def equal(got, want, what):
    assert len(got) == len(want) == 4
    for g, w, k in zip(got, want, NAMES):
        g = np.asarray(g)
        assert g.dtype == np.float64 and g.shape == np.asarray(w).shape, (what, k)
        bad = np.nonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))[0]
        assert np.array_equal(g, w, equal_nan=True), (what, k, len(bad), bad[:5], g[bad[:3]], np.asarray(w)[bad[:3]])


def check_rolling(x, window, warmup=WARMUP, name=None, want=None, slab_elements=None):
    """cusum_test_rolling through the host API against `want` (default: the vectorised helper) -> (want, diag, helper's stats)."""
    stats = {"pairs": 0, "skipped": 0}
    with np.errstate(all="ignore"):
        own = H.cusum_test_rolling(x, window, warmup, stats=stats)
    want = own if want is None else want
    with slab(slab_elements):
        got = P().cusum_test_rolling(x, window, warmup)
    d = diag_last()
    equal(got, want, name)
    assert d["pairs"] == stats["pairs"] and d["quotients"] == stats["pairs"] - stats["skipped"], (name, d, stats)
    if name:
        _counts.record(f"cusum_test/{name}", outputs_compared=4 * len(x), finite=int(np.isfinite(want[0]).sum()), pairs=d["pairs"])
    return want, d, stats


def check_developing(x, warmup=WARMUP, name=None, want=None):
    stats = {"pairs": 0, "skipped": 0}
    with np.errstate(all="ignore"):
        own = H.cusum_test_developing(x, warmup, stats=stats)
    want = own if want is None else want
    got = P().cusum_test_developing(x, warmup)
    d = diag_last()
    equal(got, want, name)
    assert d["pairs"] == stats["pairs"] and d["quotients"] == stats["pairs"] - stats["skipped"], (name, d, stats)
    if name:
        _counts.record(f"cusum_test/{name}", outputs_compared=4 * len(x), finite=int(np.isfinite(want[0]).sum()), pairs=d["pairs"])
    return want, d, stats


@pytest.fixture(scope="module")
def walk():
    x = H.grid_walk(60_000, 41)
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------- the device's square root
def test_device_sqrt_is_the_hosts():
    """Checked once: the float64 sqrt of the kernels is correctly rounded, as the host's is (so it needs no restatement)."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.random(200_000) * 10.0 ** rng.integers(-300, 300, 200_000), np.arange(0, 5000.0),
                        4.6 + np.log(np.arange(1, 5000.0)), [0.0, np.inf, np.nan, 5e-324, 2.2250738585072014e-308, -1.0, -0.0]])
    ctx = _ffi.default_context()
    d, o = DeviceArray.from_host(ctx, v), DeviceArray(ctx, len(v), np.float64)
    ctx.call("fmk_diag_device_sqrt", d.p, C.c_int64(len(v)), o.p)
    with np.errstate(all="ignore"):
        want = np.array([math.sqrt(a) if a >= 0 else math.nan for a in v.tolist()])
    got = o.to_host()
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)]))
    _counts.record("cusum_test/device_sqrt", values_compared=len(v))


# ---------------------------------------------------------------------------------------------- the reference's recorded outputs
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay_host_api(name):
    equal(call(P(), name), expected(name), name)
    _counts.record(f"cusum_test/fixture/{name}", outputs_compared=4 * MANIFEST[name]["n"], finite=MANIFEST[name]["finite"])


@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay_dev_api_and_device_trades(name):
    from finmlkit_amd import _ffi, engine
    from finmlkit_amd._ffi import DeviceArray
    c, x = MANIFEST[name], case_input(name)
    ctx = _ffi.default_context()
    n = len(x)
    d_x = DeviceArray.from_host(ctx, x)
    out = [DeviceArray(ctx, n, np.float64) for _ in range(4)]
    if c["fn"] == "rolling":
        ctx.call("fmk_cusum_test_rolling_dev", d_x.p, C.c_int64(n), C.c_int64(c["window"]), C.c_int64(c["warmup"]), *[o.p for o in out])
    else:
        warmup = c["warmup"] if c["fn"] == "developing" else n - 1
        ctx.call("fmk_cusum_test_developing_dev", d_x.p, C.c_int64(n), C.c_int64(warmup), *[o.p for o in out])
    got = [o.to_host() for o in out]
    equal(got if c["fn"] != "last" else [g[-1:] for g in got], expected(name), name)
    if c["fn"] == "rolling":
        t = engine.DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), x, np.ones(n, np.float32))
        equal([o.to_host() for o in t.cusum_test_rolling(c["window"], c["warmup"])], expected(name), name)


@pytest.mark.parametrize("name", RAISING)
def test_fixture_replay_raising(name):
    from finmlkit_amd import _ffi, engine
    x, c = case_input(name), MANIFEST[name]
    with pytest.raises(ValueError) as e:
        call(P(), name)
    assert str(e.value) == c["message"]
    # ... and the library itself says the same through the C ABI, host and device flavour
    ctx = _ffi.default_context()
    out = [np.zeros(len(x)) for _ in range(4)]
    with pytest.raises(ValueError) as e:
        ctx.call("fmk_cusum_test_rolling", _ffi.ptr(x), C.c_int64(len(x)), C.c_int64(c["window"]), C.c_int64(c["warmup"]),
                 *[_ffi.ptr(o) for o in out])
    assert str(e.value) == c["message"]
    t = engine.DeviceTrades.from_numpy(np.arange(len(x), dtype=np.int64), x, np.ones(len(x), np.float32))
    with pytest.raises(ValueError) as e:
        t.cusum_test_rolling(c["window"], c["warmup"])
    assert str(e.value) == c["message"]


def test_warmup_below_two_is_refused_by_the_library():
    from finmlkit_amd import _ffi
    ctx = _ffi.default_context()
    x = np.asarray(H.grid_walk(64, 5))
    out = [np.zeros(64) for _ in range(4)]
    for name, args in (("fmk_cusum_test_rolling", (C.c_int64(50), C.c_int64(1))), ("fmk_cusum_test_developing", (C.c_int64(1),))):
        with pytest.raises(ValueError) as e:
            ctx.call(name, _ffi.ptr(x), C.c_int64(64), *args, *[_ffi.ptr(o) for o in out])
        assert str(e.value) == H.WARMUP_MESSAGE


# ---------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("window", [32, 33, 50, 64, 65, 1000])
def test_geometry_rolling(walk, window):
    sizes = [window + 1 + extra for extra in (0, 1, 63, 64, 65, 255, 256, 257, 3000)]
    sizes += [window, window - 1, WARMUP + 1, WARMUP + 2]
    for n in sizes:
        x = walk[len(walk) - n:]                    # the last n elements: another phase of the walk at every size
        want, d, _ = check_rolling(x, window, name=f"geometry/w{window}/n{n}")
        if n >= WARMUP + 2:
            assert d["outputs"] == n - WARMUP and d["slabs"] == 1 and np.isfinite(want[0][WARMUP:]).all()
        else:
            assert d["outputs"] == 0 and np.isnan(np.concatenate(want)).all()


@pytest.mark.parametrize("n", [WARMUP, WARMUP + 1, WARMUP + 2, 255 + WARMUP, 256 + WARMUP, 257 + WARMUP, 1500])
def test_geometry_developing(walk, n):
    want, d, _ = check_developing(walk[:n], name=f"geometry/developing/n{n}")
    assert int(np.isfinite(want[0]).sum()) == max(0, n - WARMUP) == d["outputs"]      # n = warmup + 1: one value


def test_small_window_is_raised_to_warmup_plus_two(walk):
    x = walk[:700]
    want, _, _ = check_rolling(x, 5, name="window_raised")
    equal(P().cusum_test_rolling(x, WARMUP + 2, WARMUP), want, "window 32")
    equal(P().cusum_test_rolling(x, 0, WARMUP), want, "window 0")
    assert not np.array_equal(H.cusum_test_rolling(x, WARMUP + 3, WARMUP)[0], want[0], equal_nan=True)


def test_last_is_the_last_developing_output(walk):
    x = walk[:500]
    got = P().cusum_test_last(x)
    assert all(type(v) is float for v in got) and got == H.cusum_test_last(x)
    assert got == tuple(float(a[-1]) for a in H.cusum_test_developing(x, WARMUP))


# ---------------------------------------------------------------------------------------------- windows wider than one staging
def test_forced_slabs(walk):
    x = walk[:2600]
    want, d, _ = check_rolling(x, 1000, name="slab256/w1000", slab_elements=256)
    assert d["slab"] == 256 and d["slabs"] == -(-(1000 + TILE) // 256) > 1
    check_rolling(x, 1000, want=want, slab_elements=64)
    check_rolling(x[:700], 50, slab_elements=100, name="slab100/w50")
    assert diag_last()["slabs"] == -(-(50 + TILE) // 100)


def test_window_wider_than_one_staging(walk):
    window = SLAB_MAX + 900
    x = walk[:window + 300]
    _, d, _ = check_rolling(x, window, name=f"wide_window/w{window}")
    assert d["slab"] == SLAB_MAX and d["slabs"] > 1


# ---------------------------------------------------------------------------------------------- the tie rule
def test_monotone_series_first_n_wins():
    n, w = 900, 200
    down = 100.0 * np.exp(-1e-3 * np.arange(n) - 1e-4 * np.sin(np.arange(n)))        # strictly decreasing
    assert (np.diff(down) < 0).all()
    for x, zero_side, crit_side in ((down, 0, 2), (1e4 / down, 1, 3)):
        want, _, _ = check_rolling(x, w, name=f"monotone/{'down' if zero_side == 0 else 'up'}")
        T = np.minimum(np.arange(n), w)
        first = np.array([math.sqrt(4.6 + math.log(t - 1)) for t in T[WARMUP:]])
        assert (want[zero_side][WARMUP:] == 0.0).all()              # every statistic of that side is 0.0: the first n_rel keeps it
        assert np.array_equal(want[crit_side][WARMUP:], first)
        assert (want[1 - zero_side][WARMUP:] > 0.0).all()
        check_developing(x[:400], name=f"monotone/developing/{zero_side}")


def test_equal_prices_different_k():
    x = H.grid_walk(3000, 43, step=1, hold=0.9)                     # long runs of equal prices: equal dyn, different k
    assert (np.diff(x) == 0).mean() > 0.8
    check_rolling(x, 50, name="plateaus/w50")
    check_rolling(x, 300, name="plateaus/w300")
    check_developing(x[:1200], name="plateaus/developing")


# ---------------------------------------------------------------------------------------------- degenerate variance
def test_constant_series():
    x = np.full(600, 123.45)
    want, d, stats = check_rolling(x, 50, name="constant")
    assert stats["pairs"] == 0
    for a, v in zip(want, (-1e-6, -1e-6, 0.0, 0.0)):
        assert (a[WARMUP:] == v).all()
    check_developing(x[:300], name="constant/developing")


def test_one_ulp_move_skips_the_smallest_k_only():
    x = np.ones(400)
    x[200:] = 1.0 + 2.0 ** -52                                      # sigma = 2^-52 / 7: den <= 1e-16 for k <= 9
    want, d, stats = check_rolling(x, 50, name="one_ulp")
    assert 0 < stats["skipped"] < stats["pairs"] and d["quotients"] == stats["pairs"] - stats["skipped"]
    inside = slice(201, 250)
    assert (want[0][inside] >= 0.0).all() and (want[2][inside] > 0.0).all()
    assert (want[0][300:] == -1e-6).all()


# ---------------------------------------------------------------------------------------------- odd values
def test_nan_and_inf_inside_a_rolling_series():
    """The recorded case odd.rolling_nan_inf (the reference's own answer): every window that holds the NaN gets
    (-1e-6, -1e-6, 0, 0) -- sigma and every quotient are NaN, and NaN never wins.  A window that holds +inf has sigma = den = inf:
    a finite dyn gives 0.0 / inf = 0.0, which does beat -1e-6, and inf / inf is NaN -- so there no statistic is positive."""
    x, want = case_input("odd.rolling_nan_inf"), expected("odd.rolling_nan_inf")
    assert np.isnan(x[400]) and x[800] == np.inf
    w = 50
    check_rolling(x, w, name="nan_inf/w50", want=want)
    for a, v in zip(want, (-1e-6, -1e-6, 0.0, 0.0)):                # every window that holds the NaN
        assert (a[400:400 + w + 1] == v).all()
    assert (want[0][800:800 + w + 1] <= 0.0).all() and (want[1][800:800 + w + 1] <= 0.0).all()
    assert (want[0][801:800 + w + 1] == 0.0).all()                  # ... and 0.0 / inf = 0.0 has won
    for at in (400, 800):
        assert want[0][at - 1] > 0 or want[1][at - 1] > 0           # the windows around them are ordinary
        assert want[0][at + w + 1] > 0 or want[1][at + w + 1] > 0
    check_rolling(x, 1000, name="nan_inf/w1000")


def test_zero_and_negative_prices(walk):
    x = np.array(walk[:300])
    x[[50, 120, 121]] = [0.0, -3.0, -0.0]
    for bad in (x, np.where(x == 0.0, 1.0, x)):
        with pytest.raises(ValueError, match=r"^All close prices must be positive\.$"):
            P().cusum_test_rolling(bad, 50, WARMUP)
    check_developing(x, name="zero_negative/developing")          # what IEEE and the host's log give
    check_developing(x[100:], name="zero_negative/developing_tail")


# ---------------------------------------------------------------------------------------------- size
def test_size_rolling(walk):
    x = walk[:50_000]
    want, d, stats = check_rolling(x, 1000, name="size/rolling_50000_w1000")
    assert d["pairs"] == stats["pairs"] > 4.8e7 and d["tiles"] == -(-(50_000 - WARMUP) // TILE)


def test_size_developing(walk):
    want, d, stats = check_developing(walk[:6000], name="size/developing_6000")
    assert d["pairs"] == sum(t - 2 for t in range(WARMUP, 6000))


# ---------------------------------------------------------------------------------------------- resident flow
def test_resident_flow(walk):
    from finmlkit_amd import _ffi, engine
    from finmlkit_amd._ffi import DeviceArray
    n = 20_000
    px, other = np.array(walk[:n]), np.array(walk[n:2 * n])
    t = engine.DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), px, np.ones(n, np.float32))
    series = DeviceArray.from_host(t.ctx, other)
    with pytest.raises(TypeError, match="float64"):
        t.cusum_test_rolling(50, series=DeviceArray.from_host(t.ctx, other.astype(np.float32)))
    for x, kw, what in ((px, {}, "price"), (other, {"series": series}, "series")):
        want = H.cusum_test_rolling(x, 50, WARMUP)
        got = t.cusum_test_rolling(50, **kw)
        assert all(isinstance(g, DeviceArray) and g.dtype == np.float64 and g.n == n for g in got)
        # the four results are DeviceArrays and come down once, for the comparison; nothing crosses in between
        equal([g.to_host() for g in got], want, what)
        _counts.record(f"cusum_test/resident/{what}", outputs_compared=4 * n)


# ---------------------------------------------------------------------------------------------- the transform
def test_transform_on_the_recorded_frame():
    import pandas as pd
    from finmlkit_amd.feature.transforms import CUSUMTest
    c = MANIFEST["transform"]
    close = case_input("transform")
    frame = pd.DataFrame({"close": close}, index=pd.date_range("2024-01-01", periods=c["n"], freq="5min"))
    six = CUSUMTest()(frame)
    assert [s.name for s in six] == c["names"]
    for s, name in zip(six, c["names"]):
        want = _NPZ["transform.out." + name]
        assert s.index.equals(frame.index) and s.values.dtype == want.dtype, name
        assert np.array_equal(s.values, want, equal_nan=want.dtype.kind == "f"), name
    _counts.record("cusum_test/transform/recorded", outputs_compared=6 * c["n"])


def test_transform_on_a_long_frame(walk):
    import pandas as pd
    from finmlkit_amd.feature.transforms import CUSUMTest
    n = 20_000
    frame = pd.DataFrame({"px": np.array(walk[30_000:30_000 + n])}, index=pd.date_range("2024-01-01", periods=n, freq="1min"))
    tr = CUSUMTest(window_size=120, warmup_period=40, max_age=60, input_col="px")
    six = tr(frame)
    want = H.cusum_transform(*H.cusum_test_rolling(frame["px"].values, 120, 40), max_age=60)
    for s, w, name in zip(six, want, tr.output_name):
        assert s.name == name and s.values.dtype == w.dtype and np.array_equal(s.values, w, equal_nan=w.dtype.kind == "f"), name
    assert six[2].values.sum() > 10 and six[3].values.sum() > 10 and six[4].values.max() == 60
    _counts.record("cusum_test/transform/long", outputs_compared=6 * n)
