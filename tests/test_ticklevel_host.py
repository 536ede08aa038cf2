"""CPU-only: the tick-level features (comp_lagged_returns, ewmst, ewmst_mean0, ewms, realized_vol).  The plain restatement
(tests/_ticklevel_ref.py) against the reference's recorded outputs (tests/golden/ticklevel_edges.npz, written by
tools/gen_ticklevel_edges_golden.py from the untouched reference with libm's exp and log), the regenerated tapes against their
recorded hashes, and the C oracle (oracle/fmk_oracle.c), which the older GPU tests trust at full size, against the restatement.

Bit for bit, NaN positions and the sign of every zero included: comp_lagged_returns, ewmst, ewmst_mean0, ewms.  realized_vol: the
restatement is the correctly rounded value and the reference sums pairwise, so the two agree in NaN and inf positions and within
the deviation recorded per case; the oracle restates the pairwise sum and is held against the reference bit for bit.  Cases of
more than 2100 elements record the hash of the reference's output instead of the output."""
import json
import math
import os

import numpy as np
import pytest

from tests import _ticklevel_ref as H

from tests._ticklevel_fixture import (GATED_CASES, GOLD, MANIFEST, NOTES, OK_CASES, REFUSED, RV_CASES, case_input,  # noqa: F401
                                      holds_reference, relative_deviation, restated, same_bits)


def test_fixture_holds_what_it_should():
    assert {c["fn"] for c in MANIFEST.values()} == set(H.FUNCTIONS)
    assert set(OK_CASES) | set(NOTES["left_out_names"]) == set(H.fixture_cases()) and set(REFUSED) == set(H.refused_cases())
    for name in NOTES["left_out_names"]:                 # only the half lives the issue allows to leave out
        assert ".half_life." in name and name.rsplit(".half_life.", 1)[1] in ("0.0", "-1.0")
    for fn in ("ewmst", "ewmst0"):
        hls = {MANIFEST[k]["args"][0] for k in OK_CASES if k.startswith(fn + ".half_life.")}
        assert set(H.HALF_LIVES) <= hls and hls <= set(H.HALF_LIVES + H.ODD_HALF_LIVES)
        assert {MANIFEST[k]["args"][1] for k in OK_CASES if k.startswith(fn + ".floor.")} == {1e-12, 0.0, 1e-3}
        assert {MANIFEST[k]["n"] for k in OK_CASES if k.startswith(fn + ".length.")} == set(H.EW_LENGTHS)
    assert math.nextafter(2.0, 0.0) in H.HALF_LIVES and np.float64(math.nextafter(2.0, 0.0)).view(np.uint64) & 0xFFFFFFFFFFFFF == 0xFFFFFFFFFFFFF
    # a dt == 0 run crossing tick 2048, a whole tile of them, and a 3-day gap at tick 2047 and at tick 2048
    dt = {tag: np.diff(case_input(f"ewmst.tape.{tag}")[0]) for tag in H.TAPE_PLACED}         # dt[k] belongs to tick k + 1
    assert (dt["zero2040_2060"][2039:2060] == 0).all() and (dt["zero_tile"][2047:4095] == 0).all()
    assert dt["gap2047"][2046] == H.DAY3_NS and dt["gap2048"][2047] == H.DAY3_NS
    assert dt["back2050"][2049] == -1_000_000 and (np.delete(dt["back2050"], 2049) >= 0).all()
    # what the tapes hold: every kind of gap, runs of equal timestamps, the long run, and alpha exactly 0 and exactly 1
    ts = case_input("lr.mixed.simple")[0]
    assert set(np.unique(np.diff(ts)).tolist()) == {0, 1, 1_000_000, 1_000_000_000, H.DAY3_NS}
    runs = H.equal_run_lengths(ts)
    assert runs.max() >= H.LONG_RUN > H.LR_CAP and (np.diff(ts) == H.DAY3_NS).sum() == 2
    assert H.alpha_of(0, 5.0) == 0.0 and H.alpha_of(H.DAY3_NS, 5.0) == 1.0
    assert case_input("lr.small.n1025.w1.0.simple")[0].max() < 1 << 53
    # the outputs hold what the cases are about
    assert MANIFEST["lr.odd_prices.simple"]["inf"] > 0 and MANIFEST["lr.odd_prices.log"]["inf"] > 0
    for lg in ("simple", "log"):
        assert MANIFEST[f"lr.burst.n1025.w1e-07.{lg}"]["finite"] == 0          # below the float64 spacing: ti <= target
        assert MANIFEST[f"lr.small.n1025.w1e-07.{lg}"]["finite"] > 0           # exact timestamps: a lag of 1 ns exists
        assert MANIFEST[f"lr.burst.n1025.w2.56e-07.{lg}"]["finite"] > 0
        assert MANIFEST[f"lr.burst.n1025.w10000000.0.{lg}"]["finite"] == 0
    for fn in ("ewmst", "ewmst0"):
        c = MANIFEST[f"{fn}.floor.0.001"]
        out = restated(f"{fn}.floor.0.001")               # every output that is a number is the floor
        assert (out[~np.isnan(out)] == 1e-3).all() and 1 <= c["nan"] < 100
        assert np.isnan(case_input(f"{fn}.nan.all")[1]).all()
    assert MANIFEST["ewmst.floor.0.0"]["zeros"] > 0
    assert MANIFEST["ewms.span.0"]["nan"] == MANIFEST["ewms.span.1"]["nan"] == H.N_EW
    assert MANIFEST["rv.w1.n2304"]["nan"] == 2304 and MANIFEST["rv.w0"]["nan"] == 50
    assert {MANIFEST[k]["args"][0] for k in RV_CASES} == set(H.RV_WINDOWS) | {0}
    assert all(MANIFEST[k]["n"] <= H.RECORD_MAX for k in OK_CASES)
    for f in ("ticklevel_edges.npz", "ticklevel_edges.json"):
        assert os.path.getsize(os.path.join(GOLD, f)) < 1 << 20


def test_regenerated_tapes_hash_to_the_recorded_ones():
    for name, c in MANIFEST.items():
        ins = case_input(name)
        assert [H.input_hash(a) for a in ins] == c["input_sha256"], name
        assert all(len(a) == c["n"] for a in ins), name
    table = {**H.fixture_cases(), **H.refused_cases()}
    for name, c in MANIFEST.items():                      # the table of cases is the recorded one (JSON has lists for tuples)
        assert json.loads(json.dumps(table[name]["source"])) == c["source"] and json.loads(json.dumps(table[name]["args"])) == c["args"], name


@pytest.mark.parametrize("name", GATED_CASES)
def test_restatement_equals_the_reference(name):
    c = MANIFEST[name]
    if c["fn"] != "ewms":
        assert holds_reference(name, restated(name)), name
        return
    # ewms: the recorded run is interpreted, its `x ** 2` is libm's pow(x, 2.0); with that power the restatement is the reference in
    # every bit.  The contract is the compiled reference's x * x (the restatement's default): NaN where the recorded output has them,
    # and as far from it as the generator recorded.
    as_run = H.ewms(*case_input(name), *c["args"], square=H.libm_square)
    assert holds_reference(name, as_run), name
    own = restated(name)
    assert H.sha256(H.nan_canonical(own)) == c["restatement_sha256"], name
    assert np.array_equal(np.isnan(own), np.isnan(as_run)), name
    assert int((~((own == as_run) | np.isnan(own))).sum()) == c["pow_differs"], name
    assert relative_deviation(own, as_run) == c["pow_deviation"] <= NOTES["pow_deviation_max"] < 1e-12, name


@pytest.mark.parametrize("name", GATED_CASES)
def test_oracle_equals_the_restatement(orc, name):
    """The C oracle, which the older GPU tests compare with at full size, against the restatement, bit for bit."""
    c = MANIFEST[name]
    assert same_bits(H.call(c["fn"], case_input(name), c["args"], mod=orc), restated(name)), name


@pytest.mark.parametrize("name", RV_CASES)
def test_realized_vol_within_the_recorded_deviation(orc, name):
    """The oracle restates NumPy's pairwise sum: it is the reference's recorded output in every bit.  The restatement is the correctly
    rounded value: NaN and inf where the reference has them, and no further from it than the generator recorded."""
    c = MANIFEST[name]
    ref = H.call("rv", case_input(name), c["args"], mod=orc)
    assert holds_reference(name, ref), name
    own = restated(name)
    assert np.array_equal(np.isnan(own), np.isnan(ref)) and np.array_equal(np.isinf(own), np.isinf(ref)), name
    assert H.sha256(H.nan_canonical(own)) == c["restatement_sha256"], name
    assert relative_deviation(ref, own) == c["reference_deviation"] <= NOTES["reference_deviation_max"] < 1e-14, name


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_raise_without_a_device(name):
    c = MANIFEST[name]
    with pytest.raises(ValueError) as e:
        H.call(c["fn"], case_input(name), c["args"])
    assert str(e.value) == c["message"]
    if c["fn"] == "lr":                  # the reference's own message; the package checks before it needs a device
        from finmlkit_amd.feature.core.utils import comp_lagged_returns
        assert c["message"] == "The return window must be greater than zero." and c["reference"] == "raises ValueError"
        with pytest.raises(ValueError, match="^The return window must be greater than zero.$"):
            comp_lagged_returns(*case_input(name), *c["args"])


def test_empty_series():
    e = np.empty(0)
    ts = np.empty(0, np.int64)
    for r in (H.comp_lagged_returns(ts, e, 1.0, False), H.ewmst(ts, e, 5.0), H.ewmst_mean0(ts, e, 5.0), H.ewms(e, 20), H.realized_vol(e, 3, True)):
        assert r.dtype == np.float64 and r.shape == (0,)
