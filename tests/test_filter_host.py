"""CPU-only: the symmetric CUSUM event filter's argument checks, the plain-Python yardstick (tests/_filter_ref.py) against the
reference's recorded outputs (tests/golden/cusum_filter.npz, written by tools/gen_filter_golden.py), and the two new symbols."""
import json
import os

import numpy as np
import pytest

from tests import _filter_ref as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "cusum_filter.json")))
_NPZ = np.load(os.path.join(GOLD, "cusum_filter.npz"))
EXC = {"ValueError": ValueError}


def case_inputs(name, orc):
    """-> (x, thr) of a fixture case: stored, or regenerated from the case's seed (`tape.*`)."""
    c = MANIFEST[name]
    if name.startswith("tape."):
        _, px, _, _ = orc.synth(c["seed"], 0, c["n"])
        return px, H.hashed_threshold(c["n"], c["c"], c["per_element"], c["shift"])
    return _NPZ[name + ".x"], _NPZ[name + ".thr"]


def expected(name):
    return _NPZ[name + ".events"]


OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
RAISING = sorted(k for k, v in MANIFEST.items() if "raises" in v)


def test_fixture_holds_the_reference_test_calls():
    assert len([k for k in MANIFEST if k.startswith("refcall.")]) == 6 and len(RAISING) == 3
    assert sum(MANIFEST[k]["events"] for k in OK_CASES) > 10000


@pytest.mark.parametrize("name", OK_CASES)
def test_helper_equals_the_reference(orc, name):
    x, thr = case_inputs(name, orc)
    ev = H.cusum_filter(x, thr)
    assert ev.dtype == np.int64 and np.array_equal(ev, expected(name))
    assert len(ev) == MANIFEST[name]["events"]


@pytest.mark.parametrize("name", RAISING)
def test_recorded_raising_calls_raise_without_a_device(orc, name):
    from finmlkit_amd.sampling import cusum_filter
    x, thr = case_inputs(name, orc)
    for fn in (H.cusum_filter, cusum_filter):
        with pytest.raises(EXC[MANIFEST[name]["raises"]]) as e:
            fn(x, thr)
        assert str(e.value) == MANIFEST[name]["message"]


def test_value_errors_and_their_messages():
    from finmlkit_amd import sampling
    with pytest.raises(ValueError, match=r"^Input time series must have at least 2 elements\.$"):
        sampling.cusum_filter(np.array([100.0]), np.array([0.01]))
    with pytest.raises(ValueError, match=r"^Input time series must have at least 2 elements\.$"):
        sampling.cusum_filter(np.array([]), np.array([0.01, 0.02]))          # the length of the series is checked first
    with pytest.raises(ValueError, match=r"^Threshold array must either contain 1 const\. element or len\(raw_time_series\) elements\.$"):
        sampling.cusum_filter(np.array([100.0, 101.0, 102.0]), np.array([0.01, 0.02]))
    with pytest.raises(NotImplementedError):
        sampling.z_score_peak_filter(np.arange(10.0), 3)


def test_priority_case_separates_the_two_orders():
    x, thr = _NPZ["hand.priority.x"], _NPZ["hand.priority.thr"]
    neg_first, s_neg = H.cusum_filter(x, thr, return_state=True)
    pos_first, s_pos = H.cusum_filter(x, thr, negative_first=False, return_state=True)
    assert list(neg_first) == [2] and list(pos_first) == [2, 4]
    assert s_neg != s_pos


def test_library_exports_the_filter():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    for s in ("fmk_cusum_filter_dev", "fmk_cusum_filter", "fmk_diag_cusum_filter_last"):
        assert hasattr(lib, s), s
