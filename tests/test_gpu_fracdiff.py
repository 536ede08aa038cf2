"""The causal FIR filter and the fractional differentiation on the MI355X (csrc/fmk_fir.hip) against the fold of
tests/_fracdiff_ref.py: NaN positions exactly, every finite output bit for bit.  No case asks the oracle for
more than about 5e5 tap-products."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _counts
from tests import _fracdiff_ref as F

pytestmark = pytest.mark.gpu

TILE = 512                           # outputs per workgroup (csrc/fmk_common.h: FMK_FIR_TILE)
TAPS = 512                           # taps per staging pass (csrc/fmk_common.h: FMK_FIR_TAPS)
MAX_WIDTH = 8192                     # csrc/fmk_common.h: FMK_FIR_MAX_WIDTH
CAP = 600_000                        # tap-products per oracle call: "about 5e5"
SEAM_N = 2 * TILE + 77
SEAM_WIDTHS = (1, 2, 3, 63, 64, 65, TAPS - 1, TAPS, TAPS + 1, 2 * TAPS + 3)
LENGTH_WIDTHS = (1, 65, TAPS + 1)


def test_the_constants_above_are_the_librarys():
    from finmlkit_amd.feature.core import fracdiff as P
    assert P.geometry() == (TILE, TAPS) and P.FIR_MAX_WIDTH == MAX_WIDTH
    assert 2 * TAPS + 3 < SEAM_N, "the widest seam case still has outputs"


def ctx_():
    from finmlkit_amd import _ffi
    return _ffi.default_context()


def dev_call(x, w, offset=0):
    """fmk_fir_dev through the raw ABI on a resident copy of x, from element `offset` on -> host array of len(x) - offset."""
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.feature.core import fracdiff as P
    ctx = ctx_()
    x = np.ascontiguousarray(x, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    d_x = DeviceArray.from_host(ctx, x)
    n = len(x) - offset
    out = DeviceArray(ctx, n, np.float64)
    rc = P.entries()[1](ctx.handle, C.c_void_p(d_x.ptr + 8 * offset), n, w.ctypes.data_as(C.c_void_p), len(w), out.p)
    assert rc == 0, rc
    return out.to_host()


def host_call(x, w):
    """fmk_fir, the host-pointer entry, through the raw ABI."""
    from finmlkit_amd import _ffi
    from finmlkit_amd.feature.core import fracdiff as P
    x = np.ascontiguousarray(x, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.empty(len(x))
    assert P.entries()[0](ctx_().handle, _ffi.ptr(x), len(x), _ffi.ptr(w), len(w), _ffi.ptr(out)) == 0
    return out


def oracle(x, w):
    assert F.products(len(x), len(w)) <= CAP, (len(x), len(w))
    return F.fir_ref(x, w)


def same(got, want, what):
    assert F.bits_equal(got, want), what
    return len(want), int(np.isfinite(want).sum())


@pytest.fixture(scope="module")
def series():
    """The two seeded inputs, shared by the tests below (never written to)."""
    s = {"walk": F.log_price_walk(SEAM_N, 2101), "mantissa": F.mantissa_returns(SEAM_N, 2102)}
    for v in s.values():
        v.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def whole(series):
    """(weights, oracle outputs) of the mantissa series per width, computed once for the tests that start from the whole series."""
    out = {}
    for width in (3, 65):
        w = F.random_weights(width, 2200 + width)
        out[width] = (w, oracle(series["mantissa"], w))
    return out


# ---------------------------------------------------------------------------------------------- widths
@pytest.mark.parametrize("width", SEAM_WIDTHS)
@pytest.mark.parametrize("kind", ["walk", "mantissa"])
def test_widths_at_the_seams(series, kind, width):
    x, w = series[kind], F.random_weights(width, 2300 + width)
    want = oracle(x, w)
    assert np.isnan(want[:width - 1]).all() and np.isfinite(want[width - 1:]).all()
    n, finite = same(dev_call(x, w), want, f"{kind} W={width} (_dev)")
    same(host_call(x, w), want, f"{kind} W={width} (host pointers)")
    _counts.record(f"fracdiff/widths/{kind}_w{width}", outputs_compared=2 * n, finite=2 * finite)


def test_the_maximum_width(series):
    n = MAX_WIDTH + 70
    x, w = np.resize(series["mantissa"], n), F.random_weights(MAX_WIDTH, 2400)
    want = oracle(x, w)
    assert int(np.isfinite(want).sum()) == 71 and np.isfinite(want[MAX_WIDTH - 1])
    same(dev_call(x, w), want, "W=8192 (_dev)")
    same(host_call(x, w), want, "W=8192 (host pointers)")
    _counts.record("fracdiff/max_width", outputs_compared=2 * n, finite=2 * 71)


@pytest.mark.parametrize("width", LENGTH_WIDTHS)
def test_lengths_at_the_seams(series, width):
    lengths = sorted({n for n in (1, width - 1, width, width + 1, TILE - 1, TILE, TILE + 1, TILE + width - 1, TILE + width) if n >= 1})
    lengths = [n for n in lengths if F.products(n, width) <= CAP]
    assert len(lengths) >= 5 and TILE + width in lengths
    w = F.random_weights(width, 2500 + width)
    compared = finite = 0
    for n in lengths:
        x = series["mantissa"][:n]
        want = oracle(x, w)
        assert int(np.isfinite(want).sum()) == max(0, n - width + 1)
        a, b = same(dev_call(x, w), want, f"W={width} n={n} (_dev)")
        same(host_call(x, w), want, f"W={width} n={n} (host pointers)")
        compared, finite = compared + 2 * a, finite + 2 * b
    _counts.record(f"fracdiff/lengths/w{width}", outputs_compared=compared, finite=finite)


def test_a_halo_longer_than_a_tile(series):
    width = min(2 * TILE + 5, MAX_WIDTH)
    n = width + TILE + 3
    x, w = np.resize(series["walk"], n), F.random_weights(width, 2600)
    want = oracle(x, w)
    a, b = same(dev_call(x, w), want, f"W={width} (_dev)")
    _counts.record("fracdiff/long_halo", outputs_compared=a, finite=b)


# ---------------------------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize("width", [3, 65])
def test_one_non_finite_element_blanks_exactly_its_windows(series, whole, width):
    w, base = whole[width]
    n = SEAM_N
    compared = 0
    for bad in (math.nan, math.inf, -math.inf):
        for i in (0, TILE - 1, TILE, n - 1, n // 2 + 3):
            x = np.array(series["mantissa"])
            x[i] = bad
            want = np.array(base)
            want[i:i + width] = np.nan                                   # the outputs t in [i, i + W - 1]; t < W - 1 is NaN already
            got = dev_call(x, w)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (width, bad, i)
            same(got, want, f"W={width} {bad} at {i}")
            compared += n
    _counts.record(f"fracdiff/non_finite/w{width}", outputs_compared=compared)


# ---------------------------------------------------------------------------------------------- geometry and alignment
def test_the_bits_do_not_depend_on_where_the_series_starts(series, whole):
    compared = 0
    for width in (3, 65):
        w, base = whole[width]
        assert F.bits_equal(dev_call(series["mantissa"], w), base)
        for s in (1, 3, TILE - 1, TILE + 1):
            got = dev_call(series["mantissa"], w, offset=s)          # an 8-byte aligned pointer; tiles s elements further on
            assert np.isnan(got[:width - 1]).all()
            assert np.array_equal(got[width - 1:].view(np.int64), base[s + width - 1:].view(np.int64)), (width, s)
            compared += len(got) - (width - 1)
    _counts.record("fracdiff/offsets", outputs_compared=compared, finite=compared)


def test_subnormal_products_and_sums():
    rng = np.random.default_rng(2700)
    n, width = TILE + 90, 5
    x = rng.uniform(-3.0, 3.0, n) * 1e-310
    w = rng.uniform(-3.0, 3.0, width) * 1e-3
    want = F.fir_ref(x, w, fma=F.fma_fraction)                           # the definition itself
    assert F.bits_equal(F.fir_ref(x, w), want)
    tiny = want[width - 1:]
    assert (np.abs(tiny) < 2.0 ** -1022).all() and (tiny != 0.0).sum() > n - 20
    a, b = same(dev_call(x, w), want, "subnormals (_dev)")
    same(host_call(x, w), want, "subnormals (host pointers)")
    _counts.record("fracdiff/subnormals", outputs_compared=2 * a, finite=2 * b)


# ---------------------------------------------------------------------------------------------- FFD end to end
@pytest.mark.parametrize("d,threshold,n", [(0.4, 1e-3, 1500), (0.4, 1e-4, 1500), (0.1, 1e-5, 4076 + 60)])
def test_frac_diff_ffd(d, threshold, n):
    from finmlkit_amd.feature.core import fracdiff as P
    x = F.log_price_walk(n, 2800)
    w = F.weights_ref(d, threshold)
    want = oracle(x, w)
    got = P.frac_diff_ffd(x, d, threshold)
    a, b = same(got, want, f"frac_diff_ffd d={d} threshold={threshold}")
    assert b == n - len(w) + 1
    assert F.bits_equal(P.fir(x, P.frac_diff_weights(d, threshold)), want)
    _counts.record(f"fracdiff/ffd/d{d}_thr{threshold}", outputs_compared=2 * a, finite=2 * b)


def test_integer_orders():
    from finmlkit_amd.feature.core import fracdiff as P
    x = F.log_price_walk(1300, 2801)
    x[[200, 900]] = [math.inf, math.nan]
    one = P.frac_diff_ffd(x, 1)
    ok = np.ones(1300, bool)
    ok[[0, 200, 201, 900, 901]] = False
    assert np.array_equal(np.isnan(one), ~ok)
    assert np.array_equal(one[ok].view(np.int64), np.diff(x)[ok[1:]].view(np.int64))
    zero = P.frac_diff_ffd(x, 0)
    fin = np.isfinite(x)
    assert np.array_equal(np.isnan(zero), ~fin) and np.array_equal(zero[fin], x[fin])
    _counts.record("fracdiff/integer_orders", outputs_compared=2600, finite=int(ok.sum() + fin.sum()))


# ---------------------------------------------------------------------------------------------- resident and composed forms
def trades_of(price):
    from finmlkit_amd import engine
    n = len(price)
    ts = (np.arange(n, dtype=np.int64) + 1_700_000_000) * 1_000_000_000
    return engine.DeviceTrades.from_numpy(ts, price, np.ones(n, np.float32))


def test_device_trades_methods():
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.feature.core import fracdiff as P
    from finmlkit_amd.sampling.filters import cusum_filter
    logp = F.log_price_walk(3000, 2900)
    t = trades_of(np.exp(logp))
    d_logp = DeviceArray.from_host(t.ctx, logp)
    ffd = t.frac_diff(d_logp, 0.4, 1e-3)
    assert isinstance(ffd, DeviceArray) and ffd.n == 3000 and ffd.dtype == np.float64
    host = P.frac_diff_ffd(logp, 0.4, 1e-3)
    assert F.bits_equal(ffd.to_host(), host)
    w = F.random_weights(9, 2901)
    assert F.bits_equal(t.fir(d_logp, w).to_host(), P.fir(logp, w))
    assert F.bits_equal(t.fir(d_logp, w).to_host(), F.fir_ref(logp, w))
    with pytest.raises(ValueError) as e:
        t.frac_diff(d_logp, -0.5)
    assert str(e.value) == P.D_MESSAGE
    with pytest.raises(ValueError) as e:
        t.fir(d_logp, [1.0, math.nan])
    assert str(e.value) == P.FIR_FINITE_MESSAGE
    # the differentiated series feeds the event filter without leaving the device (the filter's NaN returns clamp to zero)
    assert (host[54:] > 0.0).all()
    threshold = 4.0 * float(np.std(np.diff(np.log(host[54:]))))
    events = t.cusum_filter(threshold, series=ffd).to_host()
    assert np.array_equal(events, cusum_filter(host, np.array([threshold])))
    assert 5 < len(events) < 2000 and events.min() > 54
    assert t.zscore(ffd, 24).n == 3000
    _counts.record("fracdiff/device_trades", outputs_compared=3 * 3000 + len(events))


def test_compose_keeps_the_chain_on_the_device(monkeypatch):
    import pandas as pd
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.feature import transforms as T
    from finmlkit_amd.feature.core import fracdiff as P
    from finmlkit_amd.feature.core.ma import sma
    n = 2000
    price = F.log_price_walk(n, 2902)
    frame = pd.DataFrame({"price": price}, index=pd.date_range("2024-01-01", periods=n, freq="1s"))
    want = sma(P.frac_diff_ffd(price, 0.4, 1e-3), 24)
    uploads = []
    plain = DeviceArray.from_host.__func__

    def counting(cls, ctx, a):
        uploads.append(np.asarray(a).dtype)
        return plain(cls, ctx, a)
    monkeypatch.setattr(DeviceArray, "from_host", classmethod(counting))
    got = T.Compose(T.FracDiff(0.4, 1e-3, input_col="price"), T.SMA(24))(frame)
    assert uploads == [np.int64, np.float64], "timestamps and the input, nothing else"
    monkeypatch.undo()
    assert got.name == "price_ffd0.4_sma24" and got.index.equals(frame.index)
    assert F.bits_equal(got.values, want) and np.isfinite(want[54 + 23:]).all()
    alone = T.FracDiff(0.4, 1e-3, input_col="price")(frame)
    assert alone.name == "price_ffd0.4" and F.bits_equal(alone.values, P.frac_diff_ffd(price, 0.4, 1e-3))
    _counts.record("fracdiff/compose", outputs_compared=2 * n)


# ---------------------------------------------------------------------------------------------- refusals with a live context
def test_refusals_through_the_raw_abi(series):
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.feature.core import fracdiff as P
    ctx = ctx_()
    x = np.array(series["walk"][:100])
    d_x, d_out, out = DeviceArray.from_host(ctx, x), DeviceArray(ctx, 100, np.float64), np.empty(100)
    good, bad = np.ones(3), np.array([1.0, math.nan, 1.0])
    cases = [(0, good, False, P.FIR_EMPTY_MESSAGE), (MAX_WIDTH + 1, good, False, P.FIR_MAX_WIDTH_MESSAGE),
             (3, bad, False, P.FIR_FINITE_MESSAGE), (3, good, True, P.FIR_ALIAS_MESSAGE)]
    host_entry, dev_entry = P.entries()
    for width, w, alias, message in cases:
        rc = dev_entry(ctx.handle, d_x.p, 100, _ffi.ptr(w), width, d_x.p if alias else d_out.p)
        assert rc == _ffi.E_ARG and _ffi.lib().fmk_last_error(ctx.handle).decode() == message, (width, message)
        rc = host_entry(ctx.handle, _ffi.ptr(x), 100, _ffi.ptr(w), width, _ffi.ptr(x) if alias else _ffi.ptr(out))
        assert rc == _ffi.E_ARG and _ffi.lib().fmk_last_error(ctx.handle).decode() == message, (width, message)
    # nothing was written, and the context still serves
    assert np.array_equal(d_x.to_host(), x)
    assert F.bits_equal(dev_call(x, good), F.fir_ref(x, good))
