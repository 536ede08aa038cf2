"""CPU-only: the window statistics rolling_kurtosis, trend_slope, hurst_exponent and bipower_variation.  Both forms of the plain
restatement (tests/_shape_ref.py) against the reference's recorded outputs (tests/golden/shape.npz, written by
tools/gen_shape_golden.py) within the tolerances recorded beside them (shape.json: measured on the CPU between the reference and the
restatement, times 16, rounded up to a power of ten), NaN positions exactly; the regenerated inputs against their recorded hashes;
the exact-value cases; the argument checks of the host layer, which need no device; the transforms' names; the library's symbols."""
import inspect
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _shape_ref as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_JSON = json.load(open(os.path.join(GOLD, "shape.json")))
MANIFEST, TOLERANCES = _JSON["cases"], _JSON["tolerances"]
_NPZ = np.load(os.path.join(GOLD, "shape.npz"))

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)
INF = math.inf


def product(fn):
    from finmlkit_amd.feature.core import shape
    return getattr(shape, H.PRODUCT_NAMES[fn])


def case_input(name):
    """The input of a fixture case: stored, or regenerated from the case's seeds."""
    src = MANIFEST[name].get("source")
    return _NPZ[name + ".x"] if src is None else H.generate(src)


def expected(name):
    return _NPZ[name + ".out"]


def tolerance(fn):
    return TOLERANCES[fn]["tolerance"]


def close(fn, got, want, what):
    """NaN positions exactly, the values within the statistic's recorded tolerance in its measure."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(np.isnan(got) != np.isnan(want))[0]
    assert len(bad) == 0, (what, "NaN positions", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    dev = H.deviation(fn, got, want)
    assert dev <= tolerance(fn), (what, dev, tolerance(fn))
    return dev


def test_fixture_holds_what_it_should():
    for fn in H.FUNCTIONS:
        t = TOLERANCES[fn]
        assert t["measure"] == ("relative" if H.RELATIVE[fn] else "absolute")
        assert 0.0 < t["ref_dev"] and t["tolerance"] == H.tolerance_from(t["ref_dev"]) and 16 * t["ref_dev"] <= t["tolerance"] <= 160 * t["ref_dev"]
        assert t["ref_dev"] == max(MANIFEST[k]["dev_vector"] for k in OK_CASES if MANIFEST[k]["fn"] == fn)
    assert max(TOLERANCES[fn]["tolerance"] for fn in H.FUNCTIONS) <= 1e-10
    windows = {fn: {MANIFEST[k]["window"] for k in OK_CASES if MANIFEST[k]["fn"] == fn and k.startswith("walk.")} for fn in H.FUNCTIONS}
    assert {1, 2, 3, 64, 65, 257} <= windows["kurtosis"] and {1, 2, 64, 65, 300} <= windows["slope"]
    assert {9, 10, 11, 64, 65, 300} <= windows["hurst"] and {1, 2, 64, 65, 300} <= windows["bipower"]
    assert len(REFUSED) == 10 and sum(MANIFEST[k]["finite"] for k in OK_CASES) > 20000
    # the exact values: two points have kurtosis -2, three points -1.5; one point and nine points have none
    assert (expected("walk.kurtosis_w2")[1:] == -2.0).all() and np.isnan(expected("walk.kurtosis_w1")).all()
    out = expected("walk.kurtosis_w3")[2:]
    assert np.abs(out + 1.5).max() < 1e-14
    assert np.isnan(expected("walk.hurst_w9")).all() and np.isnan(expected("walk.slope_w1")).all()
    # constant windows of zeros and dyadic values: NaN for kurtosis and hurst, 0 for the slope and for bipower on zeros
    for k in OK_CASES:
        if k.startswith("const.") and "stretch" not in k:
            c = MANIFEST[k]
            if c["fn"] in ("kurtosis", "hurst"):
                assert c["finite"] == 0, k
            elif c["fn"] == "slope" or "zeros" in k:
                assert c["zeros"] == c["finite"] == c["n"] - H.first_output(c["fn"], c["window"]), k
    assert np.array_equal(expected("const.bipower_half_w5")[5:], np.full(35, H.BV_SCALE * 1.25))
    # bipower starts one output later than the others
    assert np.isnan(expected("walk.bipower_w12")[:12]).all() and np.isfinite(expected("walk.bipower_w12")[12:]).all()
    assert np.isnan(expected("walk.kurtosis_w32")[:31]).all() and np.isfinite(expected("walk.kurtosis_w32")[31:]).all()
    for name in ("shape.npz", "shape.json"):
        assert os.path.getsize(os.path.join(GOLD, name)) <= os.path.getsize(os.path.join(GOLD, "recur.npz"))


def test_a_refused_element_poisons_exactly_the_windows_that_read_it():
    """edge.*: NaN, +-inf (the slope: also 0, -0 and a negative price) at 60, 140, ...: NaN from there to the last window that holds
    it -- as its last element, and as its first (hurst: the element that enters no difference; bipower reads window + 1)."""
    for fn in H.FUNCTIONS:
        for w in (12, 33):
            name = f"edge.{fn}_w{w}"
            out, x = expected(name), case_input(name)
            reach = w + 1 if fn == "bipower" else w
            hit = np.nonzero(~(np.isfinite(x) & ((x > 0) | (fn != "slope"))))[0]
            assert len(hit) == (6 if fn == "slope" else 3)
            want_nan = np.zeros(len(x), bool)
            want_nan[:reach - 1] = True
            for i in hit:
                want_nan[i:i + reach] = True
            assert np.array_equal(np.isnan(out), want_nan), name
    out = expected("edge.bipower_inf_zero_w4")                          # inf times zero and inf times a number: NaN, never inf
    assert np.isnan(out[40:45]).all() and np.isnan(out[81:86]).all() and np.isfinite(out[[39, 45, 80, 86]]).all()
    assert not np.isinf(np.concatenate([expected(k) for k in OK_CASES])).any()


def test_regenerated_inputs_hash_to_the_recorded_ones():
    seen = 0
    for name, c in MANIFEST.items():
        if "source" in c:
            x = case_input(name)
            assert H.sha256(x) == c["input_sha256"] and len(x) == c["n"], name
            seen += 1
    assert seen >= 30


@pytest.mark.parametrize("form", ("vector", "scalar"))
@pytest.mark.parametrize("name", OK_CASES)
def test_restatement_equals_the_reference(name, form):
    c = MANIFEST[name]
    close(c["fn"], H.call(c["fn"], case_input(name), c["window"], form=form), expected(name), name)


def test_exact_values():
    for form in ("scalar", "vector"):
        x = H.dyadic_returns(50, 5)
        assert np.isnan(H.rolling_kurtosis(x, 1, form)).all()
        k2, k3 = H.rolling_kurtosis(x, 2, form), H.rolling_kurtosis(x, 3, form)
        flat2, flat3 = x[1:] == x[:-1], (x[2:] == x[1:-1]) & (x[1:-1] == x[:-2])
        assert np.isnan(k2[0]) and np.array_equal(k2[1:][~flat2], np.full((~flat2).sum(), -2.0)) and np.isnan(k2[1:][flat2]).all()
        assert np.isnan(k3[:2]).all() and np.abs(k3[2:][~flat3] + 1.5).max() < 1e-14
        assert np.isnan(H.hurst_exponent(x, 9, form)).all() and np.isfinite(H.hurst_exponent(x, 10, form)[9:]).sum() >= 40
        assert np.isnan(H.trend_slope(H.grid_walk(50, 6), 1, form)).all()
        for v in (0.0, 0.5, 3.0):
            c = np.full(30, v)
            assert np.isnan(H.rolling_kurtosis(c, 4, form)).all() and np.isnan(H.hurst_exponent(c, 10, form)).all()
            bv = H.bipower_variation(c, 4, form)
            assert np.isnan(bv[:4]).all() and np.array_equal(bv[4:], np.full(26, H.BV_SCALE * (4 * v * v)))
        for v in (100.0, 0.5, 3.0):
            s = H.trend_slope(np.full(30, v), 6, form)
            assert np.isnan(s[:5]).all() and (s[5:] == 0.0).all()
        # a price doubling every step: ln is linear, the slope ln 2, the angle atan(ln 2)
        s = H.trend_slope(2.0 ** np.arange(20), 5, form)
        assert np.abs(s[4:] - math.degrees(math.atan(math.log(2.0)))).max() < 1e-13
        # a price the logarithm refuses, a NaN or an infinity: NaN in exactly the windows that read it
        for w in (1, 2, 5):
            for bad in (0.0, -0.0, -1.0, math.nan, INF, -INF):
                p = np.full(20, 100.0)
                p[10] = bad
                s = H.trend_slope(p, w, form)
                assert np.isnan(s[10:10 + w]).all() and np.isnan(s[:w - 1]).all()
                assert (np.isnan(s[w - 1:10]) == (w == 1)).all() and (np.isnan(s[10 + w:]) == (w == 1)).all(), (w, bad)


@pytest.mark.parametrize("fn", H.FUNCTIONS)
def test_first_and_last_position_of_a_window(fn):
    """A NaN or an infinity as the first and as the last element a window reads, at window 10 and 11: the outputs that read it are
    NaN, their neighbours are numbers.  For hurst the first position enters no difference and poisons all the same."""
    base = H.grid_walk(80, 7) if fn == "slope" else H.dyadic_returns(80, 7)
    for w in (10, 11):
        reach = w + 1 if fn == "bipower" else w
        for bad in (math.nan, INF, -INF):
            x = np.array(base)
            x[40] = bad
            for form in ("scalar", "vector"):
                out = H.call(fn, x, w, form)
                assert np.isnan(out[40:40 + reach]).all(), (w, bad, form)          # 40 is the last position, ..., the first
                assert np.isfinite(out[reach - 1:40]).all() and np.isfinite(out[40 + reach:]).all(), (w, bad, form)


def test_the_two_forms_agree_on_long_windows():
    x, p = np.array(H.mantissa_returns(800, 8)), np.array(H.grid_walk(800, 9))
    x[[50, 51, 400, 799]] = np.nan
    p[[50, 51, 400, 799]] = (np.nan, 0.0, INF, -3.0)
    for fn in H.FUNCTIONS:
        for window in (9, 200, 333):
            a, b = (H.call(fn, p if fn == "slope" else x, window, form=f) for f in ("scalar", "vector"))
            dev = H.deviation(fn, a, b)
            assert dev is not None and dev <= tolerance(fn) and np.isfinite(a).sum() >= (0 if (fn, window) == ("hurst", 9) else 60), (fn, window)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_raise_without_a_device(name):
    c = MANIFEST[name]
    x = case_input(name)
    for fn, kw in ((H.call, {"form": "scalar"}), (H.call, {})):
        with pytest.raises(ValueError) as e:
            fn(c["fn"], x, c["window"], **kw)
        assert str(e.value) == c["message"]
    with pytest.raises(ValueError) as e:
        product(c["fn"])(x, c["window"])
    assert str(e.value) == c["message"]


def test_messages_empty_series_and_signatures_need_no_device():
    from finmlkit_amd.feature import core
    for fn in H.FUNCTIONS:
        P = product(fn)
        assert getattr(core, H.PRODUCT_NAMES[fn]) is P and H.PRODUCT_NAMES[fn] in core.__all__
        assert list(inspect.signature(P).parameters) == ["x", "window"]
        for f in (P, getattr(H, H.PRODUCT_NAMES[fn])):
            with pytest.raises(ValueError, match=r"^window must be at least 1\.$"):
                f(np.arange(12.0), 0)
            r = f(np.empty(0), 12)
            assert r.dtype == np.float64 and r.shape == (0,)
    for f in (product("hurst"), H.hurst_exponent):
        for w in (1, 8):
            with pytest.raises(ValueError, match=r"^hurst_exponent: window must be at least 9\.$"):
                f(np.arange(12.0), w)
        assert f(np.empty(0), 9).shape == (0,)


def test_transform_names_and_defaults():
    from finmlkit_amd.feature import transforms as T
    for cls, window, col, name in ((T.KurtosisTransform, 32, "ret1", "ret1_kurt_32"), (T.TrendSlope, 24, "close", "close_trend_slope_24"),
                                   (T.HurstExponent, 24, "ret1", "ret1_hurst24"), (T.BiPowerVariation, 12, "ret1", "ret1_bv_12")):
        t = cls()
        assert isinstance(t, T.SISOTransform) and (t.window, t.requires, t.output_name) == (window, [col], name)
        assert list(inspect.signature(cls.__init__).parameters) == ["self", "window", "input_col"]
        t = cls(window=40, input_col="y")
        assert t.window == 40 and t.requires == ["y"] and t.output_name == "y_" + name.split("_", 1)[1].replace(str(window), "40")
        with pytest.raises(ValueError, match=r"^window must be at least 1\.$"):
            cls(0)._dev(SimpleNamespace(ctx=None), SimpleNamespace(n=5))
    with pytest.raises(ValueError, match=r"^hurst_exponent: window must be at least 9\.$"):
        T.HurstExponent(8)._dev(SimpleNamespace(ctx=None), SimpleNamespace(n=5))


def test_device_trades_methods_check_before_the_device():
    from finmlkit_amd import engine
    t = engine.DeviceTrades.__new__(engine.DeviceTrades)               # no context: the checks come first
    y = SimpleNamespace(dtype=np.dtype(np.float64), n=10)
    for method in (t.kurtosis, t.trend_slope, t.hurst_exponent, t.bipower_variation):
        with pytest.raises(ValueError, match=r"^window must be at least 1\.$"):
            method(y, 0)
        with pytest.raises(TypeError, match="float64"):
            method(SimpleNamespace(dtype=np.dtype(np.float32), n=10), 12)
    with pytest.raises(ValueError, match=r"^hurst_exponent: window must be at least 9\.$"):
        t.hurst_exponent(y, 8)


def test_library_exports_the_window_statistics():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    for name in ("rolling_kurtosis", "trend_slope", "hurst_exponent", "bipower_variation"):
        assert hasattr(lib, "fmk_" + name) and hasattr(lib, "fmk_" + name + "_dev")
