"""CPU-only: rolling kurtosis and the Hurst exponent where a window has no statistic or the statistic is badly conditioned -- held
prices and returns, whole-series constants, one odd element, periodic series, prices offset by 1e5, 1e7 and 1e9, and a held price at
the window whose span takes more than one slab (tests/golden/shape_degenerate.npz + .json, written by
tools/gen_shape_degenerate_golden.py).  The truth is exact rational arithmetic on the float64 inputs: a window is of class `none`
(exact m2 == 0, or some exact tau_k == 0: NaN) or `value` (the exact statistic).  Both forms of tests/_shape_ref.py give NaN on exactly
the head plus the `none` windows and the exact value elsewhere within the tolerance recorded per statistic and input family (16 times
the vector form's worst error against the exact value, rounded up to a power of ten; no window is left out).  At the long window the
fixture holds the class mask only."""
import json
import os

import numpy as np
import pytest

from tests import _shape_ref as H
from tests import test_shape_host as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_JSON = json.load(open(os.path.join(GOLD, "shape_degenerate.json")))
MANIFEST, TOLERANCES = _JSON["cases"], _JSON["tolerances"]
_NPZ = np.load(os.path.join(GOLD, "shape_degenerate.npz"))
CASES = sorted(MANIFEST)
FAMILIES = {"kurtosis": {"held_price", "held_return", "constant", "one_odd", "offset_1e5", "offset_1e7", "offset_1e9", "long"},
            "hurst": {"held_price", "held_return", "constant", "one_odd", "period", "offset_1e5", "offset_1e7", "long"}}
LONG_TAIL = 60                                                     # outputs of the long case that the sequential form recomputes


def case_input(name):
    return H.generate(MANIFEST[name]["source"])


def none_mask(name):
    return np.unpackbits(_NPZ[name + ".none"])[:MANIFEST[name]["n"]].astype(bool)


def exact(name):
    """The exact values (NaN on the head and on `none` windows), or None where the fixture holds the class mask only."""
    return _NPZ[name + ".exact"] if MANIFEST[name].get("exact_values", True) else None


def want_nan(name):
    nan = none_mask(name)
    nan[:MANIFEST[name]["window"] - 1] = True
    return nan


def tolerance(name):
    c = MANIFEST[name]
    return TOLERANCES[c["fn"]][c["family"]]["tolerance"]


def check(name, got, what):
    """NaN on exactly the head plus the `none` windows; elsewhere within the family's tolerance of the exact value -> worst deviation
    (None at the long window, whose values the caller compares with the restatement)."""
    got = np.asarray(got)
    nan = want_nan(name)
    assert got.dtype == np.float64 and got.shape == nan.shape, what
    bad = np.nonzero(np.isnan(got) != nan)[0]
    assert len(bad) == 0, (what, "NaN positions", len(bad), bad[:5], got[bad[:5]], nan[bad[:5]])
    want = exact(name)
    if want is None:
        return None
    assert np.array_equal(np.isnan(want), nan), name
    dev = float(np.abs(got[~nan] - want[~nan]).max()) if (~nan).any() else 0.0
    assert dev <= tolerance(name), (what, dev, tolerance(name))
    return dev


def test_fixture_holds_what_it_should():
    seen = {fn: set() for fn in FAMILIES}
    for name in CASES:
        c, nan = MANIFEST[name], none_mask(name)
        seen[c["fn"]].add(c["family"])
        first = c["window"] - 1
        assert not nan[:first].any() and int(nan.sum()) == c["none"] and c["none"] + c["value"] == c["n"] - first, name
        ref = _NPZ[name + ".ref"]
        assert len(ref) == c["n"] and np.isnan(ref[:first]).all() and np.isfinite(ref[first:][~nan[first:]]).all(), name
        assert int(np.isfinite(ref[nan]).sum()) == c["reference_finite_on_none"], name
        if exact(name) is not None:
            for form in ("vector", "scalar"):
                assert c["err_" + form] <= 16.0 * c["err_reference"] + S.tolerance(c["fn"]), name
    assert seen == FAMILIES
    for fn, fams in TOLERANCES.items():
        for fam, t in fams.items():
            members = [MANIFEST[k] for k in CASES if (MANIFEST[k]["fn"], MANIFEST[k]["family"]) == (fn, fam)]
            assert t["err_vector"] == max(m["err_vector"] for m in members) and t["tolerance"] == H.tolerance_from(t["err_vector"])
            assert t["tolerance"] == 0.0 or 16 * t["err_vector"] <= t["tolerance"] <= 160 * t["err_vector"]
    assert _JSON["dropped"] == {}                                   # 1e300, 5e-324 and 1e-160: the reference gives NaN too
    # both classes where a family is meant to have both, one where it is meant to have one: the counts, so that an all-NaN or an
    # all-finite output cannot pass
    for name in CASES:
        c = MANIFEST[name]
        fam, w = c["family"], c["window"]
        if (c["fn"], w) == ("hurst", 9):
            assert c["value"] == 0, name
        elif fam in ("held_price", "held_return"):
            assert c["none"] >= 150 and c["value"] >= 15, name
        elif fam == "long":
            assert c["none"] >= 21 and c["value"] >= 400, name
        elif fam == "constant":
            assert c["value"] == 0 and c["none"] == c["n"] - w + 1, name
        elif fam == "one_odd":
            # the windows that hold the odd element, less hurst's first position, which enters no sum; at window 10 lag 8 has two
            # sums, which differ only where the odd element is in one of them: at either end
            assert c["value"] == (w if c["fn"] == "kurtosis" else 2 if w == 10 else w - 1) and c["none"] >= 11, name
        elif fam == "period":
            assert (c["none"], c["value"]) == ((0, 61) if "_p3_" in name else (61, 0)), name
        elif fam == "offset_1e9":
            assert c["none"] >= 30 and c["value"] >= 300, name
        else:
            assert fam in ("offset_1e5", "offset_1e7") and c["none"] == 0 and c["value"] == 151, name
    for fn, windows in (("kurtosis", {2, 3, 5, 12, 32, 64, 100}), ("hurst", {9, 10, 12, 17, 24, 64, 100})):
        for fam in ("held_price", "held_return", "offset_1e5", "offset_1e7"):
            assert {MANIFEST[k]["window"] for k in CASES if (MANIFEST[k]["fn"], MANIFEST[k]["family"]) == (fn, fam)} == windows
    # the held runs lie on both sides of the first tile edge: NaN at the last outputs of the first tile and the first of the second
    for fn, tile in (("kurtosis", 1024), ("hurst", 512)):
        for fam in ("held_price", "held_return"):
            for k in CASES:
                c = MANIFEST[k]
                if (c["fn"], c["family"]) == (fn, fam):
                    edge = c["window"] - 1 + tile
                    assert none_mask(k)[edge - 20:edge + 20].all() and none_mask(k)[c["window"] - 1 + 60:c["window"] - 1 + 68].all(), k
    size = sum(os.path.getsize(os.path.join(GOLD, "shape_degenerate" + e)) for e in (".npz", ".json"))
    assert size <= sum(os.path.getsize(os.path.join(GOLD, "shape" + e)) for e in (".npz", ".json"))


def test_regenerated_inputs_hash_to_the_recorded_ones():
    for name in CASES:
        x = case_input(name)
        assert H.sha256(x) == MANIFEST[name]["input_sha256"] and len(x) == MANIFEST[name]["n"], name


@pytest.mark.parametrize("name", CASES)
def test_restatement_gives_nan_or_the_exact_value(name):
    c, x = MANIFEST[name], case_input(name)
    vector = H.call(c["fn"], x, c["window"], "vector")
    check(name, vector, name + " (vector)")
    if exact(name) is not None:
        scalar = H.call(c["fn"], x, c["window"], "scalar")
        check(name, scalar, name + " (scalar)")
    else:                                                           # the long window: the sequential form on the last outputs only
        lo = c["n"] - LONG_TAIL - (c["window"] - 1)
        scalar = np.concatenate((vector[:c["n"] - LONG_TAIL], H.call(c["fn"], x[lo:], c["window"], "scalar")[c["window"] - 1:]))
        assert want_nan(name)[c["n"] - LONG_TAIL:].sum() >= 21 and (~want_nan(name)[c["n"] - LONG_TAIL:]).sum() >= 10
        dev = H.deviation(c["fn"], scalar, vector)
        assert dev is not None and dev <= S.tolerance(c["fn"]), (name, dev)
    assert np.array_equal(np.isnan(scalar), np.isnan(vector)), name


def test_the_recorded_cases_of_the_walks_do_not_move():
    """The rule changes no window that has a statistic: on every case of shape.npz both forms still give the reference's NaN
    positions and its values within the tolerances of shape.json (while the rule was written they were compared with the restatement
    before it: equal in every value, NaN for NaN)."""
    for name in S.OK_CASES:
        c = S.MANIFEST[name]
        if c["fn"] in ("kurtosis", "hurst"):
            for form in ("vector", "scalar"):
                S.close(c["fn"], H.call(c["fn"], S.case_input(name), c["window"], form), S.expected(name), name)


def test_a_held_price_has_neither_statistic():
    """24 copies of 99.55: fl(sum / w) != x leaves m2 = delta^2 (a kurtosis of -2) and tau_k = delta (a Hurst exponent of 1.3) unless the
    words themselves are compared; 99.55, 100.07, 99.55, ...: every sum of 2, 4 and 8 is equal."""
    held, alternating = np.full(24, 99.55), np.resize(np.array([99.55, 100.07]), 160)
    for form in ("vector", "scalar"):
        assert np.isnan(H.rolling_kurtosis(held, 24, form)).all() and np.isnan(H.hurst_exponent(held, 24, form)).all()
        assert np.isnan(H.rolling_kurtosis(held, 1, form)).all() and np.isnan(H.rolling_kurtosis(held, 7, form)).all()
        for w in (12, 24, 100):
            assert np.isnan(H.hurst_exponent(alternating, w, form)).all()
        assert np.isfinite(H.rolling_kurtosis(alternating, 12, form)[11:]).all()
        # +0 and -0 compare equal
        assert np.isnan(H.rolling_kurtosis(np.array([0.0, -0.0, 0.0, -0.0]), 2, form)).all()
