"""CPU-only: the bar-clock, run-length and opening-range features (bar_duration, bar_duration_ewma, bar_rate, dir_run_len, orb_break).
The NumPy restatement (tests/_clock_ref.py) against the reference's recorded outputs (tests/golden/clock.npz, written by
tools/gen_clock_golden.py from the untouched reference), the regenerated inputs against their recorded hashes, the refusals of the
host layer, which need no device, the empty series, the entries in include/fmk.h and in the built library, and the transforms' names
against the ones the reference's transforms were recorded with.  bar_duration, bar_rate, dir_run_len and orb_break are compared bit
for bit; bar_duration_ewma within 1e-9 relative with its NaN exact (the contract of the recurrence scans)."""
import inspect
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

from tests import _clock_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RECORD = json.load(open(os.path.join(GOLD, "clock.json")))
MANIFEST = RECORD["cases"]
_NPZ = np.load(os.path.join(GOLD, "clock.npz"))
ENTRIES = ("fmk_bar_duration", "fmk_bar_duration_ewma", "fmk_bar_rate", "fmk_dir_run_len", "fmk_orb_break")
SPAN_MESSAGE = "span size is less than or equal to 1. Please provide a span size greater than 1."
WINDOW_MESSAGE = "bar_rate: the window must be at least one nanosecond."


def product():
    from finmlkit_amd.feature.core import clock
    return clock


def expected(name):
    return tuple(_NPZ[f"{name}.out{k}"] for k in range(2 if MANIFEST[name]["fn"] == "orb" else 1))


def test_the_fixture_covers_the_cases_of_the_kernels_tiles():
    """The cases are laid out for the tile sizes of the built kernels: a kernel whose tile changes needs the fixture written again."""
    geo = product().geometry()
    assert geo == RECORD["geometry"]
    assert sorted(H.cases(geo)) == sorted(MANIFEST)
    for name, c in H.cases(geo).items():
        assert (c["fn"], c["args"], c["source"], c["reference"]) == tuple(MANIFEST[name][k] for k in ("fn", "args", "source", "reference"))
    assert 0.0 < RECORD["dew_ref_dev"] <= RECORD["dew_bound"] == H.DEW_BOUND
    assert "127" in RECORD["dir_run_len_note"]


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_restatement_equals_the_reference(name):
    c = MANIFEST[name]
    inputs = H.generate(c["source"])
    assert H.sha256(*inputs) == c["input_sha256"] and len(inputs[0]) == c["n"]
    got, want = H.call(c["fn"], inputs, c["args"]), expected(name)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if H.EXACT[c["fn"]]:
            assert H.same_bits(g, w), name
        else:
            dev = H.dew_deviation(g, w)
            assert dev is not None and dev <= H.DEW_BOUND, (name, dev)


def test_the_wrapped_run_lengths():
    """What the untouched reference cannot pin (its interpreter store overflows): a run of 128 reads -128, one of 256 reads 0."""
    out = H.dir_run_len(H.run_pattern([5, 257, 3])[0])
    run = out[6:6 + 257].astype(np.int64)
    assert list(run[[126, 127, 128, 254, 255, 256]]) == [127, -128, -127, -1, 0, 1]
    assert not any(MANIFEST[f"run.r{r}"]["reference"] for r in (128, 255, 256, 257)) and MANIFEST["run.r127"]["reference"]
    assert list(H.dir_run_len(np.array([3.0]))) == [0] and H.dir_run_len(np.array([3.0])).dtype == np.int8


def test_refusals_need_no_device():
    P = product()
    ts = np.arange(5, dtype=np.int64)
    for span in (0, 0.5, -3, float("nan")):
        with pytest.raises(ValueError) as e:
            P.bar_duration_ewma(ts, span)
        assert str(e.value) == SPAN_MESSAGE == P.SPAN_MESSAGE
        with pytest.raises(ValueError) as e:
            H.bar_duration_ewma(ts, span)
        assert str(e.value) == SPAN_MESSAGE
    for w in (0.0, -1.0, 4e-10, float("nan"), float("inf")):
        with pytest.raises(ValueError) as e:
            P.bar_rate(ts, w)
        assert str(e.value) == WINDOW_MESSAGE == P.BAR_RATE_WINDOW_MESSAGE
    for fn in (lambda: P.bar_duration(ts.astype(np.float64)), lambda: P.bar_duration_ewma(ts.astype(np.int32), 3),
               lambda: P.bar_rate(ts.astype("datetime64[ns]"), 1.0), lambda: P.orb_break(ts.astype(np.uint64), ts, ts, ts)):
        with pytest.raises(TypeError, match="int64"):
            fn()
    with pytest.raises(ValueError, match="one-dimensional"):
        P.bar_duration(ts.reshape(1, 5))
    with pytest.raises(ValueError, match="one-dimensional"):
        P.dir_run_len(np.ones((2, 2)))
    x = np.ones(5)
    for fn in (lambda: P.orb_break(ts, x[:4], x, x), lambda: P.orb_break(ts, x, x, np.ones(6)), lambda: P.orb_break(ts[:3], x, x, x)):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == P.ORB_SHAPE_MESSAGE


def test_empty_series_need_no_device():
    P = product()
    e64, ef = np.empty(0, np.int64), np.empty(0)
    for mod in (H, P):
        for out, dt in ((mod.bar_duration(e64, 3), np.float64), (mod.bar_duration_ewma(e64, 20), np.float64),
                        (mod.bar_rate(e64, 5.0), np.float64), (mod.dir_run_len(ef), np.int8)):
            assert out.dtype == dt and out.shape == (0,)
        lg, sh = mod.orb_break(e64, ef, ef, ef)
        assert lg.dtype == sh.dtype == np.bool_ and lg.shape == sh.shape == (0,)


def test_device_trades_methods_check_before_the_device():
    from finmlkit_amd import engine
    t = engine.DeviceTrades.__new__(engine.DeviceTrades)               # no context: the checks come first
    ts = SimpleNamespace(dtype=np.dtype(np.int64), n=10)
    y = SimpleNamespace(dtype=np.dtype(np.float64), n=10)
    short = SimpleNamespace(dtype=np.dtype(np.float64), n=9)
    with pytest.raises(ValueError, match=r"^span size is less than or equal to 1\. Please provide a span size greater than 1\.$"):
        t.bar_duration_ewma(0, ts=ts)
    with pytest.raises(ValueError, match=r"^bar_rate: the window must be at least one nanosecond\.$"):
        t.bar_rate(0.0, ts=ts)
    for fn in (lambda: t.bar_duration(1, ts=y), lambda: t.bar_duration_ewma(20, ts=y), lambda: t.bar_rate(5.0, ts=y),
               lambda: t.orb_break(y, y, y, ts=y)):
        with pytest.raises(TypeError, match="int64"):
            fn()
    for fn in (lambda: t.dir_run_len(ts), lambda: t.orb_break(y, ts, y, ts=ts)):
        with pytest.raises(TypeError, match="float64"):
            fn()
    with pytest.raises(ValueError, match=r"^orb_break: ts, high, low and close must have the same length\.$"):
        t.orb_break(y, short, y, ts=ts)


def test_library_exports_and_header_declares_the_ten_entries():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmk.h")).read(), flags=re.S)
    for s in ENTRIES:
        for name in (s, s + "_dev"):
            assert re.search(rf"\bint {name}\(fmk_ctx \*ctx, ", header), name
            assert hasattr(lib, name), name
    assert "fmk_clock.hip" in open(os.path.join(ROOT, "finmlkit_amd", "csrc", "Makefile")).read()
    P = product()
    assert sorted(op.entry for op in P.CLOCK_OPS.values()) == sorted(ENTRIES)
    from finmlkit_amd.feature.series_ops import OPS
    assert not set(P.CLOCK_OPS) & set(OPS)


def test_signatures():
    P = product()
    from finmlkit_amd.feature import core
    for f in ("bar_duration", "bar_duration_ewma", "bar_rate", "dir_run_len", "orb_break"):
        assert getattr(core, f) is getattr(P, f) and f in core.__all__
    sig = inspect.signature(P.bar_duration)
    assert list(sig.parameters) == ["ts", "periods"] and sig.parameters["periods"].default == 1
    sig = inspect.signature(P.bar_duration_ewma)
    assert list(sig.parameters) == ["ts", "span"] and sig.parameters["span"].default == 20
    assert list(inspect.signature(P.bar_rate).parameters) == ["ts", "window_sec"]
    assert list(inspect.signature(P.dir_run_len).parameters) == ["x"]
    assert list(inspect.signature(P.orb_break).parameters) == ["ts", "high", "low", "close"]
    from finmlkit_amd import engine
    D = engine.DeviceTrades
    assert list(inspect.signature(D.bar_duration).parameters) == ["self", "periods", "ts"]
    assert list(inspect.signature(D.bar_duration_ewma).parameters) == ["self", "span", "ts"]
    assert list(inspect.signature(D.bar_rate).parameters) == ["self", "window_sec", "ts"]
    assert list(inspect.signature(D.dir_run_len).parameters) == ["self", "y"]
    assert list(inspect.signature(D.orb_break).parameters) == ["self", "high", "low", "close", "ts"]
    assert inspect.signature(D.bar_duration).parameters["periods"].default == 1
    assert inspect.signature(D.bar_duration_ewma).parameters["span"].default == 20


def test_transform_names_equal_the_recorded_ones():
    from finmlkit_amd.feature import transforms as T
    made = {"BarDuration()": T.BarDuration(), "BarDuration(3)": T.BarDuration(3), "BarDuration(2, 'vwap')": T.BarDuration(2, "vwap"),
            "BarDurationEWMA()": T.BarDurationEWMA(), "BarDurationEWMA(7)": T.BarDurationEWMA(7),
            "BarRate(6min)": T.BarRate(pd.Timedelta(minutes=6)), "BarRate(90s)": T.BarRate(pd.Timedelta(seconds=90)),
            "BarRate(30min)": T.BarRate(pd.Timedelta(minutes=30)), "DirRunLen()": T.DirRunLen(), "DirRunLen('close')": T.DirRunLen("close"),
            "ORBBreak()": T.ORBBreak()}
    assert sorted(made) == sorted(RECORD["names"])
    for key, t in made.items():
        rec = RECORD["names"][key]
        assert (t.output_name, list(t.requires), list(t.produces)) == (rec["output_name"], rec["requires"], rec["produces"]), key
        if isinstance(t, T._ClockTransform):
            assert t.out_name == rec["series"], key                   # the returned Series carries no input column, as the reference's
    assert isinstance(made["DirRunLen()"], T.SISOTransform) and isinstance(made["ORBBreak()"], T.MISOTransform)
    assert T.BarDurationEWMA().span == 20 and T.BarDuration().periods == 1 and T.BarRate(pd.Timedelta(seconds=90)).window_sec == 90.0
    assert T.ORBBreak(["h", "l", "c"]).requires == ["h", "l", "c"]
    assert T.Compose(T.ReturnT(pd.Timedelta(seconds=5), input_col="price"), T.DirRunLen("ret5.0s")).output_name == "price_ret5.0s_dir_run_len"
    assert T.Compose(T.BarDuration(), T.EWMA(10, "dur_1bar")).output_name == "close_dur_1bar_ewma10"


def test_transforms_refuse_before_a_device_is_needed():
    from finmlkit_amd.feature import transforms as T
    cols = {"close": [1.0, 2.0, 3.0], "high": [1.0, 2.0, 3.0], "low": [1.0, 2.0, 3.0], "ret1": [0.1, 0.2, -0.1]}
    plain = pd.DataFrame(cols)
    ewma_message = "Input DataFrame must have a DatetimeIndex for BarDurationEWMA calculation"          # the reference's, for both
    for t, message in ((T.BarDuration(), ewma_message), (T.BarDurationEWMA(), ewma_message),
                       (T.BarRate(pd.Timedelta(minutes=6)), "Input DataFrame must have a DatetimeIndex for BarRate calculation"),
                       (T.ORBBreak(), "Input DataFrame must have a DatetimeIndex for ORB calculation")):
        with pytest.raises(ValueError) as e:
            t(plain)
        assert str(e.value) == message
    back = pd.DataFrame(cols, index=pd.DatetimeIndex(["2024-01-01 00:00", "2024-01-01 00:30", "2024-01-01 00:15"]))
    for t in (T.BarDuration(), T.BarDurationEWMA(), T.BarRate(pd.Timedelta(minutes=6)), T.ORBBreak()):
        with pytest.raises(ValueError, match="monotonic increasing"):
            t(back)
    twice = pd.DataFrame(cols, index=pd.DatetimeIndex(["2024-01-01 00:00", "2024-01-01 00:15", "2024-01-01 00:15"]))
    with pytest.raises(ValueError, match="unique"):
        T.ORBBreak()(twice)
    good = pd.DataFrame(cols, index=pd.date_range("2024-01-01", periods=3, freq="15min"))
    with pytest.raises(ValueError, match="span size"):
        T.BarDurationEWMA(0)(good)
    with pytest.raises(ValueError, match="bar_rate: the window"):
        T.BarRate(pd.Timedelta(0))(good)
    with pytest.raises(ValueError, match="not found"):
        T.DirRunLen()(good.drop(columns=["ret1"]))
    ts = SimpleNamespace(ctx=None, dtype=np.dtype(np.int64), n=3)
    with pytest.raises(ValueError, match="span size"):
        T.BarDurationEWMA(0)._dev(ts, None)
    with pytest.raises(ValueError, match="bar_rate: the window"):
        T.BarRate(pd.Timedelta(0))._dev(ts, None)
    # an empty frame is answered without a device
    none = good.iloc[:0]
    assert len(T.BarDuration()(none)) == 0 and len(T.DirRunLen()(none)) == 0 and T.ORBBreak()(none)[0].dtype == np.bool_
