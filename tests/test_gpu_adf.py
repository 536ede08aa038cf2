"""GPU: the ADF / SADF statistic (csrc/fmk_sadf.hip) against the longdouble restatement of its definition (tests/_adf_ref.py) on the
inputs of tests/test_adf_host.py, which also measures the tolerance and asserts, on the reference alone, that no input sits on a
threshold.  "Equal" means: NaN, +-inf, start == -1 and the skipped count exactly; a finite statistic within the measured tolerance
relative to max(1, |stat|); start exactly, except at an end point whose best and runner-up lie within twice the tolerance, where any
start whose reference statistic lies in that band is taken."""
import ctypes as C

import numpy as np
import pytest

from tests import _adf_ref as R
from tests import _counts
from tests import _fracdiff_ref as F
from tests import test_adf_host as H

pytestmark = pytest.mark.gpu

NAMES = [item[0] for item in H.all_inputs()]


def P():
    from finmlkit_amd.feature.core import structural_break
    return structural_break


def compare(name, stat, start, n_skipped=None):
    """The comparison of the module docstring -> the largest relative error met."""
    ref, tol = H.reference(name), H.tolerance(name)
    want, want_start = ref["stat"], ref["start"]
    assert stat.dtype == np.float64 and start.dtype == np.int64 and stat.shape == start.shape == want.shape, name
    assert np.array_equal(np.isnan(stat), np.isnan(want)), (name, np.flatnonzero(np.isnan(stat) != np.isnan(want))[:8])
    inf = np.isinf(want)
    assert np.array_equal(stat[inf], want[inf]) and not np.isinf(stat[~inf]).any(), name
    assert np.array_equal(start == -1, np.isnan(want)) and np.array_equal(want_start == -1, np.isnan(want)), name
    if n_skipped is not None:
        assert n_skipped == ref["n_skipped"] == int(np.isnan(want).sum()), name
    fin = np.isfinite(want)
    err = np.abs(stat[fin] - want[fin]) / np.maximum(1, np.abs(want[fin]))
    worst = float(err.max()) if fin.any() else 0.0
    print(f"{name}: {int(fin.sum())} finite, {int(inf.sum())} infinite, {int(np.isnan(want).sum())} skipped, error {worst:.3g} "
          f"(tolerance {tol:.3g})")
    assert worst <= tol, (name, worst, tol)
    close = H.close_end_points(ref, tol)
    exact = ~np.isnan(want) & ~close
    assert np.array_equal(start[exact], want_start[exact]), (name, np.flatnonzero(exact & (start != want_start))[:8])
    for e in np.flatnonzero(close & (start != want_start)):
        m = ref["end"][e] - start[e] + 1
        at = np.flatnonzero(ref["lengths"] == m)
        assert len(at) == 1, (name, e, m)
        assert float(ref["table"][e, at[0]]) >= want[e] - 2 * tol * max(1, abs(want[e])), (name, e, m)
    return worst


# ---------------------------------------------------------------------------------------------- every input, host form
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    y, ev, lo, hi, step, lags, trend = H.input_of(name)
    stat, start = P().sadf(y, lo, hi, lags, trend, step, ev)
    worst = compare(name, stat, start)
    _counts.record(f"adf/{name}", outputs_compared=2 * len(stat), worst_error=worst)


def test_max_len_none_is_all_history():
    y, _, lo, hi, step, lags, trend = H.input_of("all_history")
    assert hi == len(y)
    stat, start = P().sadf(y, lo)
    compare("all_history", stat, start)
    longer = P().sadf(y, lo, 10 * len(y))                   # a max_len beyond the series walks the same rows
    assert F.bits_equal(longer[0], stat) and np.array_equal(longer[1], start)


# ---------------------------------------------------------------------------------------------- the forms agree bit for bit
def trades_of(price):
    from finmlkit_amd import engine
    n = len(price)
    ts = (np.arange(n, dtype=np.int64) + 1_700_000_000) * 1_000_000_000
    return engine.DeviceTrades.from_numpy(ts, price, np.ones(n, np.float32))


@pytest.mark.parametrize("name", ["len/logwalk/129", "odd/4ct", "ends/65", "ends/0", "tiny/1"])
def test_resident_form_gives_the_hosts_bits(name):
    from finmlkit_amd._ffi import DeviceArray
    y, ev, lo, hi, step, lags, trend = H.input_of(name)
    host = P().sadf(y, lo, hi, lags, trend, step, ev)
    t = trades_of(np.where(np.isfinite(y), y, 1.0))
    d_y = DeviceArray.from_host(t.ctx, y)
    d_ev = None if ev is None else DeviceArray.from_host(t.ctx, ev)
    stat, start, skipped = t.sadf(lo, hi, lags, trend, step, end_idx=d_ev, series=d_y)
    assert isinstance(stat, DeviceArray) and stat.dtype == np.float64 and start.dtype == np.int64 and skipped.n == 1
    assert F.bits_equal(stat.to_host(), host[0]) and np.array_equal(start.to_host(), host[1])
    compare(name, stat.to_host(), start.to_host(), int(skipped.to_host()[0]))
    _counts.record(f"adf/resident/{name}", outputs_compared=2 * stat.n)


def test_default_series_is_the_price_column_and_events_stay_on_the_device():
    """events -> SADF at the events without leaving the device: the end points are what cusum_filter returns."""
    price = np.exp(H.walk("logwalk", 3001))
    t = trades_of(price)
    events = t.cusum_filter(0.03)
    ev = events.to_host()
    assert 20 < len(ev) < 1500
    stat, start, skipped = t.sadf(12, 65, end_idx=events)
    want = P().sadf(price, 12, 65, end_idxs=ev)
    assert F.bits_equal(stat.to_host(), want[0]) and np.array_equal(start.to_host(), want[1])
    ref = R.sadf(price, ev, 12, 65)
    assert int(skipped.to_host()[0]) == ref["n_skipped"] and np.array_equal(np.isnan(want[0]), np.isnan(ref["stat"]))
    fin = np.isfinite(ref["stat"])
    assert (np.abs(want[0][fin] - ref["stat"][fin]) <= H.tolerance("ends/65") * np.maximum(1, np.abs(ref["stat"][fin]))).all()
    rolling = t.adf_rolling(40)
    assert F.bits_equal(rolling.to_host(), P().adf_rolling(price, 40))
    _counts.record("adf/events", outputs_compared=2 * len(ev) + len(price))


def test_compose_keeps_the_chain_on_the_device(monkeypatch):
    import pandas as pd
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.feature import transforms as T
    from finmlkit_amd.feature.core import fracdiff
    n = 2000
    logp = F.log_price_walk(n, 3100)
    frame = pd.DataFrame({"price": logp}, index=pd.date_range("2024-01-01", periods=n, freq="1s"))
    want = P().sadf(fracdiff.frac_diff_ffd(logp, 0.4, 1e-3), 12, 64)[0]
    uploads = []
    plain = DeviceArray.from_host.__func__

    def counting(cls, ctx, a):
        uploads.append(np.asarray(a).dtype)
        return plain(cls, ctx, a)
    monkeypatch.setattr(DeviceArray, "from_host", classmethod(counting))
    got = T.Compose(T.FracDiff(0.4, 1e-3, input_col="price"), T.SADF(12, 64))(frame)
    assert uploads == [np.int64, np.float64], "timestamps and the input, nothing else"
    monkeypatch.undo()
    assert got.name == "price_ffd0.4_sadf_12_64" and got.index.equals(frame.index)
    assert F.bits_equal(got.values, want) and np.isfinite(want[54 + 14:]).all() and np.isnan(want[:54 + 13]).all()
    alone = T.SADF(12, 64, input_col="price")(frame)
    assert alone.name == "price_sadf_12_64" and F.bits_equal(alone.values, P().sadf(logp, 12, 64)[0])
    _counts.record("adf/compose", outputs_compared=2 * n)


# ---------------------------------------------------------------------------------------------- rolling and whole-series ADF
@pytest.mark.parametrize("lags,trend,window", [(1, "c", 12), (0, "c", 64), (4, "ct", 65), (2, "ct", 200)])
def test_adf_rolling_is_sadf_with_one_length(lags, trend, window):
    y = H.walk("bubble")
    rolling = P().adf_rolling(y, window, lags, trend)
    stat, start = P().sadf(y, window, window, lags, trend)
    assert F.bits_equal(rolling, stat)
    have = ~np.isnan(stat)
    assert np.array_equal(start[have], np.flatnonzero(have) - window + 1) and (start[~have] == -1).all()
    assert np.array_equal(have, np.arange(len(y)) >= window + lags)
    ref = R.sadf(y, None, window, window, 1, lags, trend)
    assert (np.abs(stat[have] - ref["stat"][have]) <= H.tolerance("len/x") * np.maximum(1, np.abs(ref["stat"][have]))).all()
    _counts.record(f"adf/rolling/{lags}{trend}{window}", outputs_compared=len(y))


@pytest.mark.parametrize("lags,trend", [(0, "c"), (1, "c"), (4, "ct")])
def test_adf_stat_is_the_last_element_of_the_longest_window(lags, trend):
    y = H.walk("logwalk")
    rows = len(y) - lags - 1
    whole = P().adf_stat(y, lags, trend)
    stat, start = P().sadf(y, rows, rows, lags, trend)
    assert isinstance(whole, float) and np.isnan(stat[:-1]).all() and start[-1] == lags + 1
    assert np.array([whole]).view(np.int64)[0] == stat[-1:].view(np.int64)[0]
    want = R.lstsq_adf(y, lags + 1, len(y) - 1, lags, trend)
    assert abs(whole - want) <= 1e-8 * max(1, abs(want))
    _counts.record(f"adf/stat/{lags}{trend}", outputs_compared=1)


# ---------------------------------------------------------------------------------------------- the stopping rule of FFD
def test_min_ffd_d_on_a_random_walk():
    from finmlkit_amd.feature.core import fracdiff
    logp = F.log_price_walk(3000, 3200)
    ds = np.linspace(0, 1, 11)
    d, stats = fracdiff.min_ffd_d(logp, ds, threshold=1e-3)
    want = []
    for dd in ds:                                        # the restatement: the exact fold, then the longdouble ADF of its tail
        w = F.weights_ref(dd, 1e-3)
        tail = F.fir_ref(logp, w)[len(w) - 1:]
        rows = len(tail) - 2
        want.append(R.sadf(tail, [len(tail) - 1], rows, rows, 1, 1, "c")["stat"][0])
    want = np.array(want)
    assert np.isfinite(want).all() and (np.abs(stats - want) <= H.tolerance("len/x") * np.maximum(1, np.abs(want))).all()
    choice = ds[np.flatnonzero(want < fracdiff.ADF_CRIT_95)[0]]
    assert d == choice and 0.0 < d <= 1.0 and stats[list(ds).index(d)] < fracdiff.ADF_CRIT_95 < stats[0]
    assert np.abs(want - fracdiff.ADF_CRIT_95).min() > 1e-6             # the choice does not hang on the tolerance
    none, again = fracdiff.min_ffd_d(logp, ds, threshold=1e-3, crit=-1e6)
    assert none is None and F.bits_equal(again, stats)
    _counts.record("adf/min_ffd_d", outputs_compared=len(ds))


# ---------------------------------------------------------------------------------------------- refusals with a live context
def test_refusals_through_the_raw_abi():
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray, c_i64
    ctx = _ffi.default_context()
    y = H.walk("logwalk")
    d_y, d_stat, d_start = DeviceArray.from_host(ctx, y), DeviceArray(ctx, 400, np.float64), DeviceArray(ctx, 400, np.int64)

    def call(min_len=12, max_len=64, step=1, lags=1, trend=0, ev=None, n_end=400, stat=d_stat, start=d_start):
        return _ffi.lib().fmk_sadf_dev(ctx.handle, d_y.p, c_i64(400), None if ev is None else ev.p, c_i64(n_end), c_i64(min_len),
                                       c_i64(max_len), c_i64(step), c_i64(lags), C.c_int(trend), stat.p, start.p, None)
    for kw in (dict(lags=5), dict(lags=-1), dict(trend=2), dict(min_len=3), dict(min_len=4, trend=1), dict(max_len=11), dict(step=0),
               dict(stat=d_y), dict(start=d_y), dict(n_end=-1)):
        assert call(**kw) == _ffi.E_ARG, kw
    bad = DeviceArray.from_host(ctx, np.array([5, 400, -1, 399], np.int64))
    assert call(ev=bad, n_end=4) == _ffi.E_ARG
    with pytest.raises(ValueError, match=r"2 end points outside \[0, 400\)"):
        _ffi.check(call(ev=bad, n_end=4), ctx.handle)
    assert call() == _ffi.OK and call(n_end=0) == _ffi.OK
    assert F.bits_equal(d_stat.to_host(), P().sadf(y, 12, 64)[0])
    with pytest.raises(ValueError, match="2 end points outside"):
        trades_of(np.exp(y)).sadf(12, 64, end_idx=bad)
