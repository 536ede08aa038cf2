"""CPU-only: the rolling approximate entropy.  Both forms of the plain restatement (tests/_entropy_ref.py) against the reference
path's recorded outputs (tests/golden/entropy.npz, written by tools/gen_entropy_golden.py: the reference's ApproximateEntropy over a
stand-in for antropy.app_entropy that follows the published algorithm) within the tolerance recorded beside them (entropy.json:
measured on the CPU between the reference path and the kernel-order restatement, times 16, rounded up to a power of ten), NaN
positions exactly; the regenerated inputs against their recorded hashes; the exact zeros; the knife-edge record; the argument
checks of the Python layers, which need no device; the transform's name; the library's symbols."""
import inspect
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _entropy_ref as E

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_JSON = json.load(open(os.path.join(GOLD, "entropy.json")))
MANIFEST, TOLERANCES, KNIFE = _JSON["cases"], _JSON["tolerances"], _JSON["knife_edge"]
_NPZ = np.load(os.path.join(GOLD, "entropy.npz"))

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)
TOLERANCE = TOLERANCES["tolerance"]
INF = math.inf


def product():
    from finmlkit_amd.feature.core import entropy
    return entropy.approximate_entropy


def case_input(name):
    """The input of a fixture case: stored, or regenerated from the case's seeds."""
    src = MANIFEST[name].get("source")
    return _NPZ[name + ".x"] if src is None else E.generate(src)


def case_args(name):
    c = MANIFEST[name]
    return c["window"], c["m"], float(c["tolerance"])


def expected(name):
    return _NPZ[name + ".out"]


def close(got, want, what):
    """NaN positions exactly, the values within the recorded tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(np.isnan(got) != np.isnan(want))[0]
    assert len(bad) == 0, (what, "NaN positions", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    dev = E.deviation(got, want)
    assert dev <= TOLERANCE, (what, dev, TOLERANCE)
    return dev


def test_fixture_holds_what_it_should():
    t = TOLERANCES
    assert t["measure"] == "absolute" and 0.0 < t["ref_dev"]
    assert t["tolerance"] == E.tolerance_from(t["ref_dev"]) and 16 * t["ref_dev"] <= t["tolerance"] <= 160 * t["ref_dev"] <= 1e-9
    assert t["ref_dev"] == max(MANIFEST[k]["dev_vector"] for k in OK_CASES)
    assert t["ref_dev_scalar"] == max(MANIFEST[k]["dev_scalar"] for k in OK_CASES) <= t["ref_dev"]
    # no window of any case within the guard of a knife edge
    assert KNIFE["guard"] == E.KNIFE == 2.0 ** -40 and KNIFE["windows"] == 0
    assert KNIFE["smallest_margin"] == min(MANIFEST[k]["margin"] for k in OK_CASES) > 1000 * E.KNIFE
    windows = {m: {MANIFEST[k]["window"] for k in OK_CASES if MANIFEST[k]["m"] == m} for m in (1, 2, 3, E.MAX_M)}
    assert {3, 4, 24, 63, 64, 65, 300, E.MAX_WINDOW} <= windows[2]
    for m in (1, 3, E.MAX_M):
        assert {m + 1, m + 2, 24, 64, 65} <= windows[m], m
    assert {float(MANIFEST[k]["tolerance"]) for k in OK_CASES} >= {0.0, 0.2, 1.0, 1e6}
    assert len(REFUSED) == 10 and {MANIFEST[k]["message"] for k in REFUSED} == set(E.MESSAGES)
    assert sum(MANIFEST[k]["finite"] for k in OK_CASES) > 15000
    assert all(MANIFEST[k]["windows_counted"] == MANIFEST[k]["finite"] for k in OK_CASES)
    # the head, and the lengths about the window
    out = expected("walk.m2_w24")
    assert np.isnan(out[:23]).all() and np.isfinite(out[23:]).all() and (out != 0.0).all()
    assert (expected("walk.m2_w3")[2:] <= 0.0).all() and (expected("walk.m2_w3")[2:] < 0.0).any()      # the result can be negative
    for w in (3, 12, 70):
        assert np.isnan(expected(f"length.n{w - 1}_w{w}")).all() and len(expected(f"length.n{w - 1}_w{w}")) == w - 1
        assert np.isfinite(expected(f"length.n{w}_w{w}")).sum() == 1 and np.isfinite(expected(f"length.n{w + 2}_w{w}")).sum() == 3
    assert expected("length.empty_w12").shape == (0,)
    for name in ("entropy.npz", "entropy.json"):
        assert os.path.getsize(os.path.join(GOLD, name)) <= os.path.getsize(os.path.join(GOLD, "shape.npz"))


def test_exact_zeros_in_the_fixture():
    """A window in which every pair matches -- constant, or under a huge tolerance -- is exactly 0.0, never -0.0 or rounding noise."""
    for k in OK_CASES:
        c, out = MANIFEST[k], expected(k)
        if (k.startswith("const.") and "stretch" not in k) or k.startswith("tolerance.every_pair"):
            assert c["zeros"] == c["finite"] == c["n"] - c["window"] + 1 > 0, k
            assert not np.signbit(out[c["window"] - 1:]).any(), k
    out = expected("const.stretch_w24")                                 # x[60:140] is constant: the windows ending at 83 .. 139
    assert (out[83:140] == 0.0).all() and (out[23:83] != 0.0).all() and (out[140:] != 0.0).all()
    # tolerance 0: only equal values match; the dyadic grid has ties, the mantissa series has none, so every count is 1 there and
    # the output is ln(N_{m+1}) - ln(N_m) up to rounding
    for w in (24, 65):
        out = expected(f"tolerance.0_mantissa_w{w}")[w - 1:]
        assert np.abs(out - (math.log(w - 2) - math.log(w - 1))).max() < 1e-14
    # the two-valued series under tolerance 0: every match is a tie at distance 0, and there are many
    for w in (12, 70):
        out = expected(f"two_valued.tolerance0_w{w}")[w - 1:]
        assert (out > math.log(w - 2) - math.log(w - 1)).all() and np.median(out) > 0.1
        assert np.array_equal(E.approximate_entropy(case_input(f"two_valued.tolerance0_w{w}"), w, 2, 0.0, "scalar")[w - 1:], out)


def test_a_refused_element_poisons_exactly_the_windows_that_read_it():
    for w in (12, 70):
        name = f"edge.w{w}"
        out, x = expected(name), case_input(name)
        hit = np.nonzero(~np.isfinite(x))[0]
        assert list(hit) == [100, 260, 420] and np.isnan(x[100]) and x[260] == INF and x[420] == -INF
        want_nan = np.zeros(len(x), bool)
        want_nan[:w - 1] = True
        for i in hit:
            want_nan[i:i + w] = True                                    # from the window it ends to the window it starts
        assert np.array_equal(np.isnan(out), want_nan), name
    out = expected("edge.ends_w10")
    assert np.isnan(out[:10]).all() and np.isfinite(out[10:90]).all() and np.isnan(out[90:100]).all() and np.isfinite(out[100:199]).all()
    assert np.isnan(out[199])
    assert not np.isinf(np.concatenate([expected(k) for k in OK_CASES])).any()


def test_regenerated_inputs_hash_to_the_recorded_ones():
    seen = 0
    for name, c in MANIFEST.items():
        if "source" in c:
            x = case_input(name)
            assert E.sha256(x) == c["input_sha256"] and len(x) == c["n"], name
            seen += 1
    assert seen >= 30


@pytest.mark.parametrize("form", ("vector", "scalar"))
@pytest.mark.parametrize("name", OK_CASES)
def test_restatement_equals_the_reference_path(name, form):
    w, m, tol = case_args(name)
    close(E.approximate_entropy(case_input(name), w, m, tol, form), expected(name), name)


def test_no_fixture_window_is_on_a_knife_edge():
    for name in OK_CASES:
        w, m, tol = case_args(name)
        if w <= 70:
            assert not E.knife_edge(case_input(name), w, m, tol).any(), name


def test_knife_edge_finds_a_planted_edge():
    # 0, 1, 0, 1: std is exactly 0.5, so under tolerance 2 the pairs (0, 1) are at distance exactly r
    x = np.array([0.0, 1.0] * 8)
    assert E.knife_edge(x, 4, 1, 2.0)[3:].all() and not E.knife_edge(x, 4, 1, 2.0)[:3].any()
    assert not E.knife_edge(x, 4, 1, 1.0).any() and not E.knife_edge(x, 4, 1, 0.0).any()
    assert not E.knife_edge(np.full(12, 0.5), 4, 1, 0.2).any()          # r == 0: no edge
    assert E.margin(x, 4, 1, 1.0) == 1.0 and E.margin(x, 4, 1, 2.0) == 0.0


def test_exact_values():
    for form in ("scalar", "vector"):
        f = lambda x, w, m=2, tol=0.2: E.approximate_entropy(x, w, m, tol, form)     # noqa: E731
        for v in (0.0, 0.5, -3.0):
            out = f(np.full(30, v), 6)
            assert np.isnan(out[:5]).all() and (out[5:] == 0.0).all() and not np.signbit(out[5:]).any()
        x = E.mantissa_returns(60, 11)
        out = f(x, 9, 3, 1e9)
        assert np.isnan(out[:8]).all() and (out[8:] == 0.0).all()
        # all values distinct and tolerance 0: every count is 1
        out = f(x, 9, 3, 0.0)
        assert np.abs(out[8:] - (math.log(6) - math.log(7))).max() < 1e-15
        # window m + 1: one vector of order m + 1 (phi = 0) and two of order m, which match each other or do not
        out = f(np.array([0.0, 0.0, 0.0, 1.0, 5.0, 1.0, 5.0]), 3, 2, 0.2)
        assert np.isnan(out[:2]).all() and out[2] == 0.0 and np.abs(out[3:] - math.log(0.5)).max() < 1e-15
        # a NaN or an infinity: NaN in exactly the windows that read it
        for bad in (math.nan, INF, -INF):
            y = np.array(x)
            y[30] = bad
            out = f(y, 7, 2)
            assert np.isnan(out[30:37]).all() and np.isfinite(out[6:30]).all() and np.isfinite(out[37:]).all()


def test_the_two_forms_agree():
    x = np.array(E.mantissa_returns(260, 12))
    x[[50, 200]] = (np.nan, INF)
    for w, m, tol in ((3, 2, 0.2), (24, 1, 0.5), (64, 2, 0.2), (65, 3, 0.2), (130, E.MAX_M, 1.0)):
        assert not E.knife_edge(x, w, m, tol).any()
        a, b = (E.approximate_entropy(x, w, m, tol, form) for form in ("scalar", "vector"))
        dev = E.deviation(a, b)
        assert dev is not None and dev <= TOLERANCE and np.isfinite(a).sum() >= 260 - 3 * w, (w, m, tol)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_raise_without_a_device(name):
    c = MANIFEST[name]
    w, m, tol = case_args(name)
    x = case_input(name)
    for f in (lambda: E.approximate_entropy(x, w, m, tol, "scalar"), lambda: E.approximate_entropy(x, w, m, tol),
              lambda: product()(x, w, m, tol), lambda: product()(np.empty(0), w, m, tol)):
        with pytest.raises(ValueError) as e:
            f()
        assert str(e.value) == c["message"]


def test_messages_empty_series_and_signature_need_no_device():
    from finmlkit_amd.feature import core
    from finmlkit_amd.feature.core import entropy
    P = product()
    assert core.approximate_entropy is P and "approximate_entropy" in core.__all__
    sig = inspect.signature(P)
    assert list(sig.parameters) == ["x", "window", "m", "tolerance"]
    assert (sig.parameters["m"].default, sig.parameters["tolerance"].default) == (2, 0.2)
    assert (entropy.APEN_MAX_M, entropy.APEN_MAX_WINDOW) == (E.MAX_M, E.MAX_WINDOW) and E.MAX_M >= 4
    assert (entropy.APEN_M_MESSAGE, entropy.APEN_MAX_M_MESSAGE, entropy.APEN_WINDOW_MESSAGE, entropy.APEN_MAX_WINDOW_MESSAGE,
            entropy.APEN_TOLERANCE_MESSAGE) == E.MESSAGES
    for f in (P, E.approximate_entropy):
        r = f(np.empty(0), 12)
        assert r.dtype == np.float64 and r.shape == (0,)
        assert f(np.empty(0), 3, 2, 0.0).shape == (0,)                  # tolerance 0 and window m + 1 are legal
        assert f(np.empty(0), E.MAX_WINDOW, E.MAX_M).shape == (0,)
        # m is asked before the window, the window before the tolerance
        with pytest.raises(ValueError, match=r"^approximate_entropy: m must be at least 1\.$"):
            f(np.arange(12.0), 0, 0, -1.0)
        with pytest.raises(ValueError, match=r"^approximate_entropy: window must be at least m \+ 1\.$"):
            f(np.arange(12.0), 4, 4, math.nan)


def test_transform_name_and_defaults():
    import sys
    from finmlkit_amd.feature import transforms as T
    t = T.ApproximateEntropy()
    assert isinstance(t, T.SISOTransform) and (t.window, t.m, t.tolerance, t.requires, t.output_name) == (24, 2, 0.2, ["ret1"], "ret1_apen24")
    assert list(inspect.signature(T.ApproximateEntropy.__init__).parameters) == ["self", "window", "m", "tolerance", "input_col"]
    t = T.ApproximateEntropy(window=40, m=3, tolerance=0.5, input_col="y")
    assert (t.window, t.m, t.tolerance, t.requires, t.output_name) == (40, 3, 0.5, ["y"], "y_apen40")
    assert "antropy" not in sys.modules
    for args, message in (((12, 0), E.M_MESSAGE), ((12, E.MAX_M + 1), E.MAX_M_MESSAGE), ((2, 2), E.WINDOW_MESSAGE),
                          ((E.MAX_WINDOW + 1, 2), E.MAX_WINDOW_MESSAGE), ((12, 2, -1.0), E.TOLERANCE_MESSAGE)):
        with pytest.raises(ValueError) as e:
            T.ApproximateEntropy(*args)._dev(SimpleNamespace(ctx=None), SimpleNamespace(n=5))
        assert str(e.value) == message


def test_device_trades_method_checks_before_the_device():
    from finmlkit_amd import engine
    t = engine.DeviceTrades.__new__(engine.DeviceTrades)               # no context: the checks come first
    y = SimpleNamespace(dtype=np.dtype(np.float64), n=10)
    sig = inspect.signature(engine.DeviceTrades.approximate_entropy)
    assert list(sig.parameters) == ["self", "y", "window", "m", "tolerance"]
    assert (sig.parameters["m"].default, sig.parameters["tolerance"].default) == (2, 0.2)
    for args, message in (((12, 0), E.M_MESSAGE), ((12, E.MAX_M + 1), E.MAX_M_MESSAGE), ((2, 2), E.WINDOW_MESSAGE),
                          ((E.MAX_WINDOW + 1, 2), E.MAX_WINDOW_MESSAGE), ((12, 2, INF), E.TOLERANCE_MESSAGE)):
        with pytest.raises(ValueError) as e:
            t.approximate_entropy(y, *args)
        assert str(e.value) == message
    with pytest.raises(TypeError, match="float64"):
        t.approximate_entropy(SimpleNamespace(dtype=np.dtype(np.float32), n=10), 12)


def test_library_exports_the_entries():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    assert hasattr(lib, "fmk_approximate_entropy") and hasattr(lib, "fmk_approximate_entropy_dev")
