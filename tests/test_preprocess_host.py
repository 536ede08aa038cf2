"""The cases of tests/_preprocess_ref.py without a device: the sequential restatements (merge_split_trades, comp_trade_side_vector,
TimeBarReader._resample per group) against the recording of the untouched reference (tools/gen_preprocess_edges_golden.py ->
tests/golden/preprocess_edges.{json,npz}), the C oracle against the restatement on every case, the 2.1 M-tick and 70 000-group ones
included, and the structural assertions that prove a case reaches what it claims to reach (the second trip of the one-block scans, a
tile without a head, heads at the emit's row and wave edges, a cumulative weight that equals the cutoff ...).  Every comparison is on
dtype, length and every element, NaN at the same places; outputs of more than 2 100 elements are held to the recorded sha256."""
import json
import os

import numpy as np
import pytest

from tests import _golden as G
from tests import _preprocess_ref as H


@pytest.fixture(scope="module")
def rec():
    with open(os.path.join(G.GOLDEN_DIR, "preprocess_edges.json")) as fh:
        return json.load(fh), G.load("preprocess_edges")


def _against_recording(rec, entry, key, got, what):
    manifest, arrays = rec
    assert str(got.dtype) == entry["dtype"] and got.size == entry["len"], (what, got.dtype, got.size, entry)
    if key in arrays:
        H.same(got, arrays[key], what + ": recording")
    else:
        assert entry["len"] > H.HASH_ABOVE
    assert H.sha256(got) == entry["sha256"], what + ": sha256 of the recording"


def test_the_recording_holds_the_case_table(rec):
    manifest, arrays = rec
    assert sorted(manifest) == sorted(list(H.TICK_CASES) + list(H.MERGE_CASES) + list(H.REFUSED_CASES) + list(H.RESAMPLE_CASES))
    for k, a in arrays.items():
        assert a.size <= H.HASH_ABOVE and k.split("__")[0] in manifest
    assert {n for n in manifest if manifest[n]["n"] > H.TRIP_N - 2} == set(H.LARGE)
    assert {manifest[n]["kind"] for n in manifest} == {"tick", "merge", "resample"}


@pytest.mark.parametrize("name", list(H.TICK_CASES))
def test_tick_rule_case(rec, orc, name):
    entry = rec[0][name]
    px = H.inputs(name)
    assert entry["kind"] == "tick" and entry["n"] == len(px) and entry["input_sha256"] == H.sha256(px), name + ": the generator drifted"
    want = H.expected(name)
    _against_recording(rec, entry["out"], name + "__out", want, name)
    H.same(orc.comp_trade_side_vector(px), want, name + ": oracle against the restatement")
    info = H.check_structure(name, want)
    assert {k: int(v) for k, v in info.items()} == entry["structure"]


@pytest.mark.parametrize("name", list(H.MERGE_CASES))
def test_merge_case(rec, orc, name):
    entry = rec[0][name]
    ts, px, am, ibm = H.inputs(name)
    assert entry["kind"] == "merge" and entry["n"] == len(ts) and entry["input_sha256"] == H.sha256(ts, px, am, ibm), name
    wants = {}
    for tag, flag in (("side", ibm), ("noside", None)):
        want = wants[tag] = H.expected(name, flag is not None)
        assert len(want[0]) == entry[tag]["m"]
        got = orc.merge_split_trades(ts, px, am, flag)
        for k, w, g in zip(H.MERGE_KEYS, want, got):
            _against_recording(rec, entry[tag][k], f"{name}__{tag}_{k}", w, f"{name} ({tag}) {k}")
            H.same(g, w, f"{name} ({tag}) {k}: oracle against the restatement")
    info = H.check_structure(name, wants["side"], wants["noside"])
    assert {k: int(v) for k, v in info.items()} == entry["structure"]


@pytest.mark.parametrize("name", list(H.REFUSED_CASES))
def test_empty_input_is_refused(rec, orc, name):
    """The reference reads element 0 of an empty input (IndexError); the restatement raises the same, the oracle returns its
    argument error."""
    entry = rec[0][name]
    kind, make = H.REFUSED_CASES[name]
    assert entry["refused"] and entry["raises"] == "IndexError" and entry["kind"] == kind
    args = make()
    with pytest.raises(IndexError):
        H.comp_trade_side_vector(args) if kind == "tick" else H.merge_split_trades(*args)
    with pytest.raises(Exception):
        orc.comp_trade_side_vector(args) if kind == "tick" else orc.merge_split_trades(*args)


@pytest.mark.parametrize("name", list(H.RESAMPLE_CASES))
def test_resample_case(rec, orc, name):
    """The recording holds the frame the reference returned (groups without an open dropped) and which groups it kept."""
    entry = rec[0][name]
    seg, cols = H.rs_inputs(name)
    assert entry["kind"] == "resample" and entry["groups"] == len(seg) - 1 and entry["input_sha256"] == H.sha256(seg, *cols), name
    want = H.rs_expected(name)
    _against_recording(rec, entry["out"]["valid"], f"{name}__out_valid", want[8], name + " valid")
    keep = want[8] == 1
    assert keep.sum() == entry["kept"]
    for k, w in zip(H.RS_COLS, want):
        _against_recording(rec, entry["out"][k], f"{name}__out_{k}", w[keep], f"{name} {k}")
    for k, g, w in zip(H.RS_OUT, orc.resample_bars(seg, *cols), want):
        H.same(g, w, f"{name} {k}: oracle against the restatement")
    assert {k: int(v) for k, v in H.rs_check_structure(name, want).items()} == entry["structure"]


def test_resample_cases_reach_the_four_dtype_combinations():
    seen = {(H.rs_inputs(n)[1][4].dtype.name, H.rs_inputs(n)[1][6].dtype.name) for n in H.RESAMPLE_CASES if ".sizes." in n}
    assert seen == {(v, w) for v in ("float32", "float64") for w in ("float32", "float64")}


def test_thresholds_as_this_machine_computes_them():
    """The two facts the epsilon cases rest on, in IEEE double arithmetic."""
    assert not (1e-12 - 0.0 > 1e-12) and np.nextafter(1e-12, 1.0) - 0.0 > 1e-12
    assert not (abs(1e-8 - 0.0) < 1e-8) and abs(np.nextafter(1e-8, 0.0) - 0.0) < 1e-8
    for b in (1.0, 27000.0):
        x = b + np.arange(4) * H.CHAIN_STEP
        assert [bool(abs(v - x[0]) < 1e-8) for v in x] == [True, True, False, False] and (np.abs(np.diff(x)) < 1e-8).all()
    assert np.float32(2.0 ** 24) + np.float32(1.0) == np.float32(2.0 ** 24)
