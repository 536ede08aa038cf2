"""CPU-only: the CSW CUSUM structural-break test.  Both forms of the plain restatement (tests/_break_ref.py) against the reference's
recorded outputs (tests/golden/cusum_test.npz, written by tools/gen_break_golden.py), the argument checks without a device, and the
CUSUMTest post-processing on the recorded four arrays.  There is no tolerance anywhere: every comparison is bit for bit, NaN
positions included."""
import json
import os

import numpy as np
import pytest

from tests import _break_ref as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "cusum_test.json")))
_NPZ = np.load(os.path.join(GOLD, "cusum_test.npz"))
NAMES = ("up", "down", "crit_up", "crit_down")
EXC = {"ValueError": ValueError}

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v and k != "transform")
RAISING = sorted(k for k, v in MANIFEST.items() if "raises" in v)


def case_input(name):
    """The price series of a fixture case: stored, or regenerated from the case's seed (`walk.*`, `transform`)."""
    c = MANIFEST[name]
    if "seed" in c:
        return H.grid_walk(c["n"], c["seed"], c["step"], c["hold"])
    return _NPZ[name + ".x"]


def expected(name):
    return tuple(_NPZ[f"{name}.{k}"] for k in NAMES)


def call(mod, name, **kw):
    """The fixture case's call on `mod` (the helper or the product) -> four arrays (cusum_test_last: of one element each)."""
    c, x = MANIFEST[name], case_input(name)
    if c["fn"] == "rolling":
        return mod.cusum_test_rolling(x, c["window"], c["warmup"], **kw)
    if c["fn"] == "developing":
        return mod.cusum_test_developing(x, c["warmup"], **kw)
    r = mod.cusum_test_last(x, **kw)
    assert all(type(v) is float for v in r)
    return tuple(np.array([v]) for v in r)


def same(got, want):
    return len(got) == len(want) and all(np.asarray(g).dtype == np.float64 and np.array_equal(g, w, equal_nan=True)
                                         for g, w in zip(got, want))


def test_fixture_holds_what_it_should():
    assert len([k for k in MANIFEST if k.startswith("refcall.")]) == 6 and len(RAISING) == 2
    assert {MANIFEST[k]["window"] for k in MANIFEST if k.startswith("walk.rolling_w")} == {32, 50, 200, 1000}
    assert sum(MANIFEST[k]["finite"] for k in OK_CASES) > 10000
    assert MANIFEST["transform"]["n"] == 3000 and min(MANIFEST["transform"]["flags"]) > 10
    # the interpreted reference (NumPy's own log) rounds this many recorded elements differently from the host's log
    assert sum(MANIFEST[k].get("np_log_differs", 0) for k in MANIFEST) == 3


@pytest.mark.parametrize("form", ["scalar", "vector"])
@pytest.mark.parametrize("name", OK_CASES)
def test_helper_equals_the_reference(name, form):
    if form == "scalar" and MANIFEST[name]["n"] > 500:
        x = case_input(name)                       # the scalar loop on the long cases: every 7th output, the same windows
        y, d2 = H.prepare(x)
        want, c = expected(name), MANIFEST[name]
        w = max(c["window"], c["warmup"] + 2) if c["window"] is not None else len(x)
        for t in range(c["warmup"], len(x), 7):
            got = H.window_scalar(y, d2, max(0, t - w), t)
            assert all(g == a[t] for g, a in zip(got, want)), (name, t)
        return
    assert same(call(H, name, form=form), expected(name)), name


def test_first_window_is_the_developing_test():
    x = H.grid_walk(400, 11)
    roll = H.cusum_test_rolling(x, 200, 30)
    dev = H.cusum_test_developing(x[:201], 30)
    assert same([a[:201] for a in roll], dev)
    assert H.cusum_test_last(x[100:301]) == tuple(a[300] for a in roll)


@pytest.mark.parametrize("name", RAISING)
def test_recorded_raising_calls_raise_without_a_device(name):
    from finmlkit_amd.feature.core import structural_break as P
    for mod in (H, P):
        with pytest.raises(EXC[MANIFEST[name]["raises"]]) as e:
            call(mod, name)
        assert str(e.value) == MANIFEST[name]["message"]


def test_value_errors_and_their_messages():
    from finmlkit_amd.feature.core import structural_break as P
    x = H.grid_walk(100, 12)
    for mod in (H, P):
        for w in (1, 0, -3):
            with pytest.raises(ValueError, match=r"^warmup_period must be at least 2\.$"):
                mod.cusum_test_rolling(x, 50, w)
            with pytest.raises(ValueError, match=r"^warmup_period must be at least 2\.$"):
                mod.cusum_test_developing(x, w)
        for n in (0, 1, 2):
            with pytest.raises(ValueError, match=r"^cusum_test_last needs at least 3 elements\.$"):
                mod.cusum_test_last(x[:n])
        bad = x.copy()
        bad[70] = 0.0
        with pytest.raises(ValueError, match=r"^All close prices must be positive\.$"):
            mod.cusum_test_rolling(bad, 50, 30)
        bad[70] = np.nan                           # NaN passes the check (the helper needs no device to go on)
    assert np.isnan(H.cusum_test_rolling(bad, 50, 30)[0][:30]).all()


def test_transform_names_and_post_processing():
    from finmlkit_amd.feature.transforms import CUSUMTest
    c = MANIFEST["transform"]
    tr = CUSUMTest()
    assert (tr.window_size, tr.warmup_period, tr.max_age, tr.requires) == (50, 30, 144, ["close"])
    assert tr.produces == c["names"] == [f"cumote_{s}50_{k}" for k in ("score", "flag", "age") for s in ("up", "down")]
    assert tr.output_name == c["names"]                              # the recorded Series names: no input-column prefix
    assert CUSUMTest(window_size=7, input_col="p").output_name[0] == "cumote_up7_score"
    four = tuple(_NPZ[f"transform.{k}"] for k in NAMES)
    for fn in (lambda: CUSUMTest.features(*four, c["max_age"]), lambda: H.cusum_transform(*four, max_age=c["max_age"])):
        six = fn()
        for got, name, dt in zip(six, c["names"], c["dtypes"]):
            want = _NPZ["transform.out." + name]
            assert got.dtype == want.dtype == np.dtype(dt), name
            assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), name
    # ages clip: a small max_age, and a flag on the very first element
    up = np.array([3.0, 0.0, 0.0, 0.0, 3.0, 0.0])
    six = CUSUMTest.features(up, up[::-1].copy(), np.ones(6), np.ones(6), 2)
    assert list(six[4]) == [0, 1, 2, 2, 0, 1] and list(six[5]) == [0, 0, 1, 2, 2, 0] and list(six[2]) == [1, 0, 0, 0, 1, 0]


def test_library_exports_the_break_test():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    for s in ("fmk_cusum_test_rolling_dev", "fmk_cusum_test_developing_dev", "fmk_cusum_test_rolling", "fmk_cusum_test_developing",
              "fmk_diag_cusum_test_last"):
        assert hasattr(lib, s), s
