"""CPU-only: the rolling price-volume correlation (rolling_price_volume_correlation).  Both forms of the plain restatement
(tests/_corr_ref.py) against the reference's recorded outputs (tests/golden/price_volume_corr.npz, written by
tools/gen_corr_golden.py), the regenerated inputs against their recorded hashes, the argument checks of the host layer, which need
no device, the transform's name and columns, and the library's symbols.  There is no tolerance anywhere: every comparison is bit for
bit, NaN positions included."""
import inspect
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _corr_ref as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "price_volume_corr.json")))
_NPZ = np.load(os.path.join(GOLD, "price_volume_corr.npz"))

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)


def product():
    from finmlkit_amd.feature.core.correlation import rolling_price_volume_correlation
    return rolling_price_volume_correlation


def case_input(name):
    """(price, volume) of a fixture case: stored, or regenerated from the case's seeds."""
    src = MANIFEST[name].get("source")
    if src is None:
        return _NPZ[name + ".price"], _NPZ[name + ".volume"]
    return H.generate(src)


def expected(name):
    return _NPZ[name + ".out"]


def same(got, want):
    return np.asarray(got).dtype == np.float64 and np.array_equal(got, want, equal_nan=True)


def test_fixture_holds_what_it_should():
    windows = {MANIFEST[k]["window"] for k in OK_CASES if k.startswith("walk.")}
    assert {1, 2, 3, 4, 9, 10, 64, 65, 300} <= windows
    assert len([k for k in MANIFEST if k.startswith("refcall.")]) == 8 and len(REFUSED) == 4
    assert sum(MANIFEST[k]["finite"] for k in OK_CASES) > 15000
    # the reference's own perfect cases: outputs 4 .. 9 are the special case's
    assert np.array_equal(expected("refcall.perfect")[4:], np.ones(6)) and np.array_equal(expected("refcall.inverse")[4:], -np.ones(6))
    assert np.isnan(expected("refcall.perfect")[:4]).all()
    # window 1: one pair per window, NaN -- but for outputs 4 .. 9, where the special case compares nothing and gives 1.0
    for k in ("walk.dyadic_w1", "walk.mantissa_w1"):
        out = expected(k)
        assert (out[4:10] == 1.0).all() and np.isnan(out[:4]).all() and np.isnan(out[10:]).all()
    # window 2: two points -- about three quarters exactly +-1, the clamp and the sign
    c = MANIFEST["clamp.w2"]
    assert c["plus_one"] > 300 and c["minus_one"] > 300 and 0.7 < (c["plus_one"] + c["minus_one"]) / c["finite"] < 0.85
    # monotone series: 1.0 / -1.0 at outputs 4 .. 9 for every window up to 9, none at window 10; outputs 10 .. 13 are the standard
    # path's
    for w in range(1, 10):
        lo = max(w, 4)
        up, down = expected(f"mono.up_up_w{w}"), expected(f"mono.up_down_w{w}")
        assert (up[lo:10] == 1.0).all() and (down[lo:10] == (1.0 if w == 1 else -1.0)).all(), w
        assert np.isnan(up[:w]).all()
        if w >= 3:                                                      # the returns of an arithmetic rise fall: about -0.99
            assert (up[10:] > -1.0).all() and (up[10:] < -0.9).all() and (down[10:] < 1.0).all() and (down[10:] > 0.9).all(), w
    assert MANIFEST["mono.up_up_w10"]["plus_one"] == 0 and MANIFEST["mono.up_up_w10"]["finite"] == 4
    # a NaN inside a special-case window fails no comparison: still 1.0 / -1.0; at the current position: NaN
    out = expected("mono.nan_volume_up_w4")
    assert np.isnan(out[5]) and (out[6:10] == 1.0).all() and out[4] == 1.0
    out = expected("mono.nan_price_down_w4")
    assert np.isnan(out[6:8]).all() and (out[[4, 5, 8, 9]] == -1.0).all()
    # windows left with 0, 1 and 2 valid pairs
    out = expected("nan.counts_price_w4")
    assert np.isnan(out[20:25]).all() and np.isfinite(out[25:]).all() and abs(out[25]) == 1.0
    out = expected("nan.counts_both_w4")
    assert np.isnan(out[20:26]).all() and abs(out[26]) == 1.0
    # constant series: NaN throughout
    assert all(MANIFEST[k]["finite"] == 0 for k in ("const.price_w5", "const.volume_w5", "const.both_w3"))
    for w in (1, 5, 12):
        for n in sorted({1, 2, w, w + 1}):
            c = MANIFEST[f"length.n{n}_w{w}"]
            assert c["n"] == n and len(expected(f"length.n{n}_w{w}")) == n \
                and c["finite"] == (1 if n == w + 1 and w > 1 else 0)           # window 1: one pair, NaN
    assert os.path.getsize(os.path.join(GOLD, "price_volume_corr.npz")) <= os.path.getsize(os.path.join(GOLD, "runsum.npz"))


def test_regenerated_inputs_hash_to_the_recorded_ones():
    seen = 0
    for name, c in MANIFEST.items():
        if "source" in c:
            p, v = case_input(name)
            assert H.sha256(p, v) == c["input_sha256"] and len(p) == len(v) == c["n"], name
            seen += 1
    assert seen >= 20


@pytest.mark.parametrize("form", ("vector", "scalar"))
@pytest.mark.parametrize("name", OK_CASES)
def test_restatement_equals_the_reference(name, form):
    p, v = case_input(name)
    assert same(H.rolling_price_volume_correlation(p, v, MANIFEST[name]["window"], form=form), expected(name)), name


def test_the_two_forms_agree_on_a_long_window():
    """Several hundred positions per window, NaN in both series: the vector form keeps the sequential order per output."""
    p, v = H.grid_walk(700, 781), H.mantissa_volumes(700, 881)
    p = np.array(p)
    p[[50, 300, 301, 640]] = np.nan
    v[[10, 350, 641]] = np.nan
    for window in (7, 200, 333):
        a, b = (H.rolling_price_volume_correlation(p, v, window, form=f) for f in ("scalar", "vector"))
        assert same(a, b) and np.isfinite(a[window:]).sum() > 300, window


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_raise_without_a_device(name):
    c = MANIFEST[name]
    p, v = case_input(name)
    for fn, kw in ((H.rolling_price_volume_correlation, {"form": "scalar"}), (H.rolling_price_volume_correlation, {}), (product(), {})):
        with pytest.raises(ValueError) as e:
            fn(p, v, c["window"], **kw)
        assert str(e.value) == c["message"]


def test_shapes_empty_series_and_signature_need_no_device():
    P = product()
    x = np.arange(12.0) + 1.0
    for fn in (H.rolling_price_volume_correlation, P):
        with pytest.raises(ValueError, match="one-dimensional and of the same length"):
            fn(x.reshape(3, 4), x.reshape(3, 4), 2)
        with pytest.raises(ValueError, match="one-dimensional and of the same length"):
            fn(x, x.reshape(3, 4), 2)
        with pytest.raises(ValueError, match=r"^window must be at least 1\.$"):
            fn(x.reshape(3, 4), x, 0)                                  # the window rule comes first
        r = fn(np.empty(0), np.empty(0), 3)
        assert r.dtype == np.float64 and r.shape == (0,)
    assert list(inspect.signature(P).parameters) == ["price", "volume", "window"]


def test_transform_name_and_default_columns():
    from finmlkit_amd.feature.transforms import MISOTransform, PriceVolumeCorrelation
    t = PriceVolumeCorrelation()
    assert isinstance(t, MISOTransform)
    assert (t.window, t.requires, t.produces, t.output_name) == (8, ["close", "volume"], ["corr_pv_8"], "corr_pv_8")
    t = PriceVolumeCorrelation(window=4, input_cols=["price", "vol"])
    assert (t.window, t.requires, t.output_name) == (4, ["price", "vol"], "corr_pv_4")
    assert list(inspect.signature(PriceVolumeCorrelation.__init__).parameters) == ["self", "window", "input_cols"]


def test_device_trades_method_checks_before_the_device():
    from finmlkit_amd import engine
    t = engine.DeviceTrades.__new__(engine.DeviceTrades)               # no context: the checks come first
    y, z = SimpleNamespace(dtype=np.dtype(np.float64), n=10), SimpleNamespace(dtype=np.dtype(np.float64), n=9)
    with pytest.raises(ValueError, match=r"^window must be at least 1\.$"):
        t.price_volume_corr(y, y, 0)
    with pytest.raises(ValueError, match="must have the same length"):
        t.price_volume_corr(y, z, 3)
    with pytest.raises(TypeError, match="float64"):
        t.price_volume_corr(y, SimpleNamespace(dtype=np.dtype(np.float32), n=10), 3)


def test_library_exports_the_correlation():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    assert hasattr(lib, "fmk_price_volume_corr") and hasattr(lib, "fmk_price_volume_corr_dev")
