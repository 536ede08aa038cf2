"""Trend-scanning labels on the MI355X against the longdouble restatement of the definition (tests/_trend_ref.py) on the inputs of
tests/test_trend_host.py.  "Equal" means: ret, the special t-values (+-inf, 0.0, NaN) and n_skipped bit for bit; a finite t-value
within tolerance(name) = 4 x the error measured on the CPU (test_trend_host.py, beside E_SWEEP); label and touch index exactly,
except for close events (best and runner-up |t| within twice the tolerance), where any span inside that band is accepted and
whose share is asserted to stay under 2 %."""
import warnings

import numpy as np
import pytest

from tests import _label_ref as H
from tests import _trend_ref as R
from tests import test_trend_host as T

pytestmark = pytest.mark.gpu

_resident = {}


def trades_of(y):
    """The series as the price column of a resident tape (one per tape, kept for the session)."""
    from finmlkit_amd import engine
    if id(y) not in _resident:
        n = len(y)
        ts = 1_600_000_000_000_000_000 + np.arange(n, dtype=np.int64) * 1_000_000
        _resident[id(y)] = (y, engine.DeviceTrades.from_numpy(ts, np.asarray(y), np.ones(n, np.float32)))
    return _resident[id(y)][1]


def run_resident(y, ev, lo, hi, st):
    """-> (labels, t_value, touch_idx, ret, n_skipped) on the host"""
    from finmlkit_amd._ffi import DeviceArray
    t = trades_of(y)
    out = t.trend_scanning(DeviceArray.from_host(t.ctx, np.ascontiguousarray(ev, dtype=np.int64)), lo, hi, st)
    assert [o.dtype.str[1:] for o in out] == ["i1", "f8", "i8", "f8", "i8"] and out[4].n == 1
    return tuple(o.to_host() for o in out[:4]) + (int(out[4].to_host()[0]),)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind == "f":
        return bool(np.all((got.view("u8") == want.view("u8")) | (np.isnan(got) & np.isnan(want))))
    return bool(np.array_equal(got, want))


def compare(name, y, ev, got, ref, tol):
    """The comparison of the module's docstring -> (largest relative error of a finite t-value, close events)."""
    labels, tval, touch, ret, n_skipped = got
    y, ev = np.asarray(y), np.asarray(ev)
    assert labels.dtype == np.int8 and tval.dtype == np.float64 and touch.dtype == np.int64 and ret.dtype == np.float64
    assert n_skipped == ref["n_skipped"], (name, n_skipped, ref["n_skipped"])
    sk = ref["skipped"]
    assert np.all(labels[sk] == 0) and np.all(np.isnan(tval[sk])) and np.all(np.isnan(ret[sk])) and np.array_equal(touch[sk], ev[sk])
    close = T.close_events(ref, tol)
    assert close.sum() * 50 <= len(close), f"{name}: {close.sum()} close events of {len(close)}"
    rt = ref["t_value"]
    special = ~np.isfinite(rt) | (rt == 0)
    finite = ~special & ~close
    err = np.abs(tval[finite].astype(np.longdouble) - rt[finite]) / np.abs(rt[finite]) if finite.any() else np.zeros(1)
    print(f"{name}: events {len(ev)}, skipped {n_skipped}, finite {int(finite.sum())}, close {int(close.sum())}, "
          f"max rel err {float(err.max()):.3e} (tolerance {tol:.3e})")
    strict = ~close
    assert np.array_equal(touch[strict], ref["touch_idx"][strict]), name
    assert np.array_equal(labels[strict], ref["labels"][strict]), name
    assert same_bits(ret[strict], ref["ret"][strict]), name
    assert same_bits(tval[special & strict], rt[special & strict].astype(np.float64)), name
    assert float(err.max()) <= tol, name
    row_of = {int(e): r for r, e in enumerate(ref["fit"])}
    for i in np.flatnonzero(close):                              # any span inside the band, and everything consistent with it
        row = ref["table"][row_of[int(i)]]
        k = np.flatnonzero(ref["spans"] == touch[i] - ev[i] + 1)
        assert len(k) == 1, (name, i)
        want = row[k[0]]
        assert abs(want) >= abs(rt[i]) * (1 - 2 * tol) and abs(np.longdouble(tval[i]) - want) <= tol * abs(want), (name, i)
        assert labels[i] == np.sign(want) and same_bits(ret[i:i + 1], y[touch[i]:touch[i] + 1] / y[ev[i]:ev[i] + 1] - 1.0)
    return float(err.max()), int(close.sum())


def check_input(name):
    for nm, y, ev, lo, hi, st in T.all_inputs():
        if nm == name:
            return compare(name, y, ev, run_resident(y, ev, lo, hi, st), T.reference(name), T.tolerance(name))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- shapes x tapes
@pytest.mark.parametrize("max_len", T.MAX_LENS)
@pytest.mark.parametrize("family", T.FAMILIES)
def test_shape_sweep(family, max_len):
    """One step of the walk (3, 5, 63, 64), the step boundary (65), carried sums (129, 257, 1000); step 1, 7 and max_len, and the
    single span min_len = max_len; events every 211 ticks with duplicates, unsorted, the last that fits and the first that
    does not."""
    for lo, hi, st in T.shapes(max_len):
        name = f"{family}/{lo}-{hi}/{st}"
        check_input(name)
        ref, ev = T.reference(name), T.events(max_len)
        last, first_out = np.flatnonzero(ev == T.N - max_len), np.flatnonzero(ev == T.N - max_len + 1)
        assert not ref["skipped"][last].any() and ref["skipped"][first_out].all() and ref["n_skipped"] >= 2


def test_more_events_than_waves():
    """6 000 events at max_len = 65: the work counter hands every wave several events."""
    check_input("counter")


@pytest.mark.parametrize("shape", T.ODD_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_hand_built_windows(shape):
    lo, hi, st = shape
    name = f"odd/{lo}-{hi}/{st}"
    check_input(name)
    y, ev = T.odd_tape()
    labels, tval, touch, ret, _ = run_resident(y, ev, lo, hi, st)
    at = lambda t0: np.flatnonzero(ev == t0)
    # a NaN, +inf or -inf tick inside the window: the spans in front of it stay eligible, the ones that hold it do not
    for bad_tick in (1010, 2020, 3005):
        for t0 in range(bad_tick - 12, bad_tick):
            if len(at(t0)) and bad_tick - t0 >= lo:
                assert np.all(touch[at(t0)] < bad_tick) and np.all(np.isfinite(tval[at(t0)])), (bad_tick, t0)
        for t0 in range(max(bad_tick - lo + 1, bad_tick - 12), bad_tick + 1):       # every span holds it, or it is t0 itself
            if len(at(t0)):
                assert np.all(np.isnan(tval[at(t0)])) and np.all(touch[at(t0)] == t0) and np.all(labels[at(t0)] == 0), (bad_tick, t0)
    for t0 in list(range(4000, 4010)) + list(range(4100, 4110)):                    # all-constant windows
        assert np.all(tval[at(t0)] == 0.0) and not np.signbit(tval[at(t0)]).any() and np.all(labels[at(t0)] == 0)
        assert np.all(touch[at(t0)] == t0 + lo - 1) and np.all(ret[at(t0)] == 0.0)
    for t0 in range(5000, 5010):                                                    # 100.00, 100.01, 100.02, ...: +inf at min_len
        assert np.all(np.isposinf(tval[at(t0)])) and np.all(labels[at(t0)] == 1) and np.all(touch[at(t0)] == t0 + lo - 1)
    for t0 in range(6000, 6010):
        assert np.all(np.isneginf(tval[at(t0)])) and np.all(labels[at(t0)] == -1) and np.all(touch[at(t0)] == t0 + lo - 1)


def test_near_threshold_ramps():
    """u = 2^-20 on the even ramps (a finite t-value, compared within the ramps' own measured tolerance), 2^-32 on the odd ones
    (+-inf, bit for bit)."""
    check_input("threshold")
    y, ev, us = T.threshold_tape()
    _, tval, _, _, n_skipped = run_resident(y, ev, T.THRESHOLD_L, T.THRESHOLD_L, 1)
    assert np.all(np.isfinite(tval[0::2])) and np.all(np.isinf(tval[1::2])) and n_skipped == 0
    assert np.all((us[0::2] > 2.0 ** -22) & (us[1::2] < 2.0 ** -30))


def test_empty_call_and_argument_errors():
    from finmlkit_amd import label
    from finmlkit_amd._ffi import DeviceArray
    y = T.tape("lognormal")
    out = run_resident(y, np.zeros(0, np.int64), 3, 10, 1)                          # n_events = 0 through the C ABI
    assert [len(o) for o in out[:4]] == [0, 0, 0, 0] and out[4] == 0
    t = trades_of(y)
    for bad in ([0, T.N], [-1, 5], [5, 2 ** 40]):                                   # resident events: the library's own check
        with pytest.raises(ValueError, match="event indices outside"):
            t.trend_scanning(DeviceArray.from_host(t.ctx, np.array(bad, np.int64)), 3, 10)
    for kw in (dict(min_len=2, max_len=10), dict(min_len=5, max_len=4), dict(min_len=3, max_len=10, step=0)):
        with pytest.raises(ValueError, match="trend_scanning"):
            t.trend_scanning(DeviceArray.from_host(t.ctx, np.array([0], np.int64)), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lab, tv, tc, rt = label.trend_scanning(y, np.array([7]))                    # the defaults: spans 5 .. 20
    assert tc[0] - 7 + 1 in range(5, 21) and lab[0] == np.sign(tv[0])


def test_host_function_and_resident_method_agree():
    from finmlkit_amd import label
    name, (lo, hi, st) = "grid01/3-129/1", (3, 129, 1)
    y, ev = T.tape("grid01"), T.events(129)
    res = run_resident(y, ev, lo, hi, st)
    with pytest.warns(RuntimeWarning, match=f"trend_scanning: {res[4]} of {len(ev)} events") as rec:
        host = label.trend_scanning(y, ev, lo, hi, st)
    assert res[4] == T.reference(name)["n_skipped"] > 0
    for h, r, what in zip(host, res[:4], ("labels", "t_value", "touch_idx", "ret")):
        assert same_bits(h, r), what
    series = run_resident(T.tape("grid001"), ev, lo, hi, st)                        # series= another resident column
    from finmlkit_amd._ffi import DeviceArray
    t = trades_of(y)
    other = t.trend_scanning(DeviceArray.from_host(t.ctx, np.ascontiguousarray(ev)), lo, hi, st,
                             series=DeviceArray.from_host(t.ctx, np.asarray(T.tape("grid001"))))
    for o, s in zip(other[:4], series[:4]):
        assert same_bits(o.to_host(), s)


# ---------------------------------------------------------------------------------------------- end to end
def test_events_to_labels_to_weights_stays_resident():
    """cusum_filter -> trend_scanning -> label_concurrency -> label_weights on the device; the touch indices are the reference's,
    so the weights are those of the reference's touch indices, bit for bit, and they meet the weights' own contract against the
    NumPy restatement (tests/_label_ref.py).  The same outputs as a labels frame feed SampleWeights.compute_info_weights."""
    import pandas as pd
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.bar.data_model import TradesData
    from finmlkit_amd.label import SampleWeights
    y = T.tape("lognormal")
    t = trades_of(y)
    d_ev = t.cusum_filter(0.001)
    ev = d_ev.to_host()
    assert 100 <= len(ev) <= 6000
    lo, hi, st = 5, 300, 1
    labels, tval, d_touch, ret, skipped = t.trend_scanning(d_ev, lo, hi, st)
    conc = t.label_concurrency(d_ev, d_touch)
    avg, att = t.label_weights(d_ev, d_touch, conc)
    touch = d_touch.to_host()
    assert np.all(touch >= ev)
    ref = R.trend_scanning(y, ev, lo, hi, st)
    tol = T.tolerance("pipeline")
    err, _, moved = R.relative_error(y, ev, lo, hi, st)                             # E_SWEEP covers this input too
    print(f"pipeline: {len(ev)} events, float64 restatement within {err:.3e} of the reference")
    assert err <= T.E_SWEEP and moved == 0 and not T.close_events(ref, tol).any()
    compare("pipeline", y, ev, (labels.to_host(), tval.to_host(), touch, ret.to_host(), int(skipped.to_host()[0])), ref, tol)
    assert np.array_equal(touch, ref["touch_idx"]) and ref["n_skipped"] * 4 < len(ev)
    d_ref_touch = DeviceArray.from_host(t.ctx, ref["touch_idx"])
    conc2 = t.label_concurrency(d_ev, d_ref_touch)
    avg2, att2 = t.label_weights(d_ev, d_ref_touch, conc2)
    assert same_bits(conc.to_host(), conc2.to_host()) and same_bits(avg.to_host(), avg2.to_host())
    assert same_bits(att.to_host(), att2.to_host())
    ts = t.ts.to_host()
    want_avg, want_conc = H.average_uniqueness(ts, ev, ref["touch_idx"])
    assert np.array_equal(conc.to_host(), want_conc)
    assert np.all(np.abs(avg.to_host() - want_avg) <= 1e-9 * want_avg)
    want_att, bound = H.return_attribution(ev, ref["touch_idx"], y, want_conc, False)
    assert np.all(np.abs(att.to_host() - want_att) <= bound)
    # the quick start: the outputs as a labels frame
    frame = pd.DataFrame({"event_idx": ev, "touch_idx": touch, "labels": labels.to_host(), "t_value": tval.to_host(),
                          "returns": ret.to_host()}, index=pd.to_datetime(ts[ev]))
    trades = TradesData(ts, np.asarray(y), np.ones(len(y)), np.arange(len(y)), dt_index=pd.to_datetime(ts))
    w = SampleWeights.compute_info_weights(trades, frame)
    assert w.index.equals(frame.index) and list(w.columns) == ["avg_uniqueness", "return_attribution"]
    assert np.all(np.abs(w["avg_uniqueness"].values - want_avg) <= 1e-9 * want_avg)
    assert np.all(np.abs(w["return_attribution"].values - want_att) <= bound)
