"""CPU-only: the rolling-window moments (sma, comp_zscore, rolling_variance_nb, variance_ratio_1_4_core).  Both forms of the plain
restatement (tests/_rolling_ref.py) against the reference's recorded outputs (tests/golden/rolling_stats.npz, written by
tools/gen_rolling_golden.py), the regenerated walks against their recorded hashes, and the argument checks of the host layer, which
need no device.  There is no tolerance anywhere: every comparison is bit for bit, NaN positions included."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _rolling_ref as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "rolling_stats.json")))
_NPZ = np.load(os.path.join(GOLD, "rolling_stats.npz"))

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)


def product():
    """The package's four functions under the reference's names."""
    from finmlkit_amd.feature.core.ma import sma
    from finmlkit_amd.feature.core.utils import comp_zscore
    from finmlkit_amd.feature.core.volatility import rolling_variance_nb, variance_ratio_1_4_core
    return SimpleNamespace(sma=sma, comp_zscore=comp_zscore, rolling_variance_nb=rolling_variance_nb,
                           variance_ratio_1_4_core=variance_ratio_1_4_core)


def case_input(name):
    """The series of a fixture case: stored, or regenerated from the case's seed (a grid walk, or its log returns)."""
    src = MANIFEST[name].get("source")
    if src is None:
        return _NPZ[name + ".x"]
    return H.walk_returns(*src["walk"]) if src.get("returns") else H.grid_walk(*src["walk"])


def expected(name):
    return _NPZ[name + ".out"]


def call(name, x=None, **kw):
    c = MANIFEST[name]
    return H.call(c["fn"], case_input(name) if x is None else x, c["window"], c.get("ddof"), c.get("min_periods"), c.get("ret_type"),
                  **kw)


def same(got, want):
    return np.asarray(got).dtype == np.float64 and np.array_equal(got, want, equal_nan=True)


def test_fixture_holds_what_it_should():
    fns = {c["fn"] for c in MANIFEST.values()}
    assert fns == {"sma", "zscore", "variance", "ratio"}
    for fn in fns:
        assert {1, 2, 7, 8, 50, 200, 1000} <= {c["window"] for k, c in MANIFEST.items() if k.startswith("walk.") and c["fn"] == fn}
    assert len([k for k in MANIFEST if k.startswith("refcall.")]) == 13 and len(REFUSED) == 10
    assert sum(MANIFEST[k]["finite"] for k in OK_CASES) > 80000
    # every case below 8 elements per window agrees with the untouched reference; from 8 up NumPy's pairwise sums differ
    assert all(MANIFEST[k]["np_pairwise_differs"] == 0 for k in OK_CASES if MANIFEST[k]["window"] < 8)
    assert all(MANIFEST[k]["np_pairwise_differs"] > 400 for k in OK_CASES
               if k.startswith("walk.") and MANIFEST[k]["window"] >= 8 and MANIFEST[k]["fn"] in ("sma", "zscore"))
    assert all(MANIFEST[k]["np_pairwise_differs"] == 0 for k in OK_CASES if MANIFEST[k]["fn"] in ("variance", "ratio"))
    # flat windows: a standard deviation of exactly 0 (NaN z-score inside the series), variances clamped to 0, a zero 4-step variance
    for w in (5, 50):
        z, v, r = (expected(f"held.w{w}.{k}") for k in ("zscore_ddof0", "variance", "ratio_log"))
        assert np.isnan(z[w - 1:]).sum() > 10 and (v == 0).sum() > 10 and np.isnan(r[w + 3:]).sum() > 10
    assert np.isnan(expected("odd.variance_ddof0_mp21")).all() and MANIFEST["odd.variance_ddof0_mp20"]["finite"] == 500
    for n, finite in ((0, 0), (9, 0), (10, 0), (13, 0), (14, 5)):
        assert MANIFEST[f"length.n{n}.ratio_log"]["finite"] == finite and len(expected(f"length.n{n}.ratio_log")) == n
    assert MANIFEST["length.n10.sma"]["finite"] == 1 and MANIFEST["length.n9.sma"]["finite"] == 0


def test_regenerated_walks_hash_to_the_recorded_ones():
    seen = 0
    for name, c in MANIFEST.items():
        if "source" in c:
            assert H.sha256(H.grid_walk(*c["source"]["walk"])) == c["walk_sha256"], name
            assert len(case_input(name)) == c["n"]
            seen += 1
    assert seen > 50


@pytest.mark.parametrize("name", OK_CASES)
def test_vector_form_equals_the_reference(name):
    assert same(call(name), expected(name)), name


@pytest.mark.parametrize("name", OK_CASES)
def test_scalar_form_equals_the_reference(name):
    c, x, want = MANIFEST[name], case_input(name), expected(name)
    if c["n"] > 500 and c["window"] >= 50:
        # the scalar loop on the long cases: the last 50 outputs, from the slice that holds all they read (the ratio's returns
        # reach window + 3 elements back)
        x = x[-(c["window"] + 60):]
        assert np.array_equal(call(name, x, form="scalar")[-50:], want[-50:], equal_nan=True), name
        return
    assert same(call(name, form="scalar"), want), name


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_raise_without_a_device(name):
    c = MANIFEST[name]
    for kw in ({"form": "scalar"}, {"form": "vector"}, {"mod": product()}):
        with pytest.raises(ValueError) as e:
            call(name, **kw)
        assert str(e.value) == c["message"]


def test_empty_series_and_defaults_need_no_device():
    P = product()
    for mod, kw in ((H, {"form": "scalar"}), (H, {}), (P, {})):
        for r in (mod.sma(np.empty(0), 3, **kw), mod.comp_zscore(np.empty(0), 3, 0, **kw), mod.rolling_variance_nb(np.empty(0), 3, **kw),
                  mod.variance_ratio_1_4_core(np.empty(0), 3, 0, "log", **kw)):
            assert r.dtype == np.float64 and r.shape == (0,)
    import inspect
    sig = inspect.signature(P.rolling_variance_nb)
    assert [p.name for p in sig.parameters.values()] == ["series", "window", "ddof", "min_periods"]
    assert (sig.parameters["ddof"].default, sig.parameters["min_periods"].default) == (1, 1)
    assert list(inspect.signature(P.variance_ratio_1_4_core).parameters) == ["price", "window", "ddof", "ret_type"]
    assert list(inspect.signature(P.comp_zscore).parameters) == ["x", "window", "ddof"]
    assert list(inspect.signature(P.sma).parameters) == ["array", "window"]


def test_transform_names_and_defaults():
    from finmlkit_amd.feature.transforms import SMA, VarianceRatio14, ZScore
    s, z, v = SMA(5), ZScore(20, "ret"), VarianceRatio14()
    assert (s.requires, s.produces, s.output_name) == (["x"], ["sma5"], "x_sma5")
    assert (z.requires, z.produces, z.ddof, z.output_name) == (["ret"], ["z20"], 0, "ret_z20")
    assert (v.requires, v.produces, v.window, v.ret_type, v.ddof) == (["close"], ["var_ratio_1_4_32"], 32, "log", 0)
    assert VarianceRatio14(window=20, input_col="high").output_name == "high_var_ratio_1_4_20"


def test_device_trades_methods_check_before_the_device():
    from finmlkit_amd import engine
    t = engine.DeviceTrades.__new__(engine.DeviceTrades)               # no context: the checks come first
    y = SimpleNamespace(dtype=np.dtype(np.float64), n=10)
    for fn in (lambda: t.sma(y, 0), lambda: t.zscore(y, -1), lambda: t.rolling_variance(y, 0),
               lambda: t.variance_ratio_1_4(0, series=y)):
        with pytest.raises(ValueError, match=r"^window must be at least 1\.$"):
            fn()
    with pytest.raises(ValueError, match=r"^comp_zscore: window - ddof must be positive\.$"):
        t.zscore(y, 5, ddof=5)


def test_library_exports_the_rolling_moments():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    for s in ("fmk_sma", "fmk_zscore", "fmk_rolling_variance", "fmk_variance_ratio_1_4"):
        assert hasattr(lib, s) and hasattr(lib, s + "_dev"), s
