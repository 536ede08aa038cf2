"""The rolling volume profile on hand-built footprints, host side: the restatement (tests/_vp_ref.py) against what the reference
recorded on them (tests/golden/vp_edges.npz, made by tools/gen_vp_edges_golden.py), and the C oracle (oracle/fmk_oracle.c) against the
restatement on every case of the table -- exact, rounding (lognormal) and NaN / inf volumes -- bit for bit.  No GPU."""
import json
import os

import numpy as np
import pytest

from tests import _vp_ref as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("poc", "hva", "lva", "pct")


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLD, "vp_edges.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLD, "vp_edges.npz")) as z:
        return {k: z[k] for k in KEYS}


def test_manifest_covers_the_table_and_hashes_match(manifest):
    """Every kind-1 case is recorded, every kind-3 case is recorded or named as left out, and the inputs built here are the ones the
    reference saw."""
    cases = manifest["cases"]
    assert set(H.names(kind=1)) <= set(cases)
    assert set(H.names(kind=3)) == (set(cases) - set(H.names(kind=1))) | set(manifest["left_out"])
    assert len(manifest["left_out"]) <= 4 and len(cases) >= 420
    for name, m in cases.items():
        c = H.CASES[name]
        assert m["input_sha256"] == H.input_hash(name), name
        assert (m["window"], m["n_bins"], m["tick"], m["va"], m["kind"]) == (c["window"], c["n_bins"], c["tick"], c["va"], c["kind"]), name
    for name, r in manifest["refused"].items():
        if "input_sha256" in r:
            assert r["input_sha256"] == H.sha256(*H.REFUSALS[name]["inputs"]), name


def test_restatement_equals_the_recorded_reference(manifest, recorded):
    n = 0
    for name, m in manifest["cases"].items():
        (own, _info) = H.expected(name)
        for k, a in zip(KEYS, own):
            H.same(a, recorded[k][m["at"]:m["at"] + m["n"]], f"{name}:{k}")
            n += len(a)
        if "stages_sha256" in m:
            c = H.CASES[name]
            assert H.stages_hash(H.stage_outputs(H, H.inputs(name), c["n_bins"], c["tick"], c["va"])) == m["stages_sha256"], name
    assert n == 4 * sum(m["n"] for m in manifest["cases"].values()) >= 9000


def test_recorded_walks_sit_on_or_clear_of_the_threshold(manifest):
    """What the generator's gate left behind: a recorded exact case either meets its threshold exactly somewhere or stays further
    from it than float32 rounds; some cases do meet it exactly with va_pct 25, 50, 75 and 100."""
    gaps = [m["walk_gap"] for m in manifest["cases"].values() if m["kind"] == 1 and m["walk_gap"] is not None]
    assert len(gaps) > 300 and min(gaps) > 0.0
    for va in (25.0, 50.0, 75.0, 100.0):
        name = f"walk.exact8.va{va}"
        trace = []
        ts, hi, lo, off, lv, bv, sv = H.inputs(name)
        levels, ab, as_ = H.aggregate_footprint(ts, hi, lo, off, lv, bv, sv, int(ts[0]), int(ts[0]), 1.0)
        H.comp_poc_hva_lva(levels, ab + as_, va, trace=trace)
        assert trace[-1][1] == 8.0 * va / 100.0
        assert (trace[-1][0] == trace[-1][1]) == (va in (50.0, 75.0, 100.0)), (va, trace)


def _oracle_same(orc, args, want, what):
    got = orc.volume_profile_rolling(*args)
    for k, a, b in zip(KEYS, got, want):
        H.same(a, b, f"{what}:{k}")
    return 4 * len(want[0])


@pytest.mark.parametrize("kind", (1, 2, 3))
def test_oracle_equals_the_restatement(orc, kind):
    n = 0
    for name in H.names(kind=kind):
        (want, _info) = H.expected(name)
        n += _oracle_same(orc, H.args(name), want, name)
        c = H.CASES[name]
        if c["one"]:                                             # the oracle's one stand-alone stage, on the same profile
            out = H.stage_outputs(H, H.inputs(name), c["n_bins"], c["tick"], c["va"])
            levels, tot = (out[3], out[4]) if c["n_bins"] is not None else (out[0], out[1] + out[2])
            share = H.calc_volume_percentage_above_poc(levels, tot, int(out[-2][0]))
            got = orc.calc_volume_percentage_above_poc(levels, tot, int(out[-2][0]))
            H.same(np.float64(got), np.float64(share), name + ":share")
    assert n >= {1: 6000, 2: 1500, 3: 100}[kind]


@pytest.mark.parametrize("wide", (1024, 1025, 4097, 8193))
def test_oracle_equals_the_restatement_on_the_reuse_footprints(orc, wide):
    """The footprints of the grid-stride cases as a device of ONE compute unit would get them."""
    cls = H.capacity_class(wide)
    waves = H.waves_per_launch(cls, 1)
    for n_bins in (None, 3):
        data = H.reuse(waves, wide)
        info = {}
        want = H.volume_profile_rolling(*data, 1.0, n_bins, 1.0, 68.34, info=info)
        assert max(info["L"]) == wide and len(info["L"]) > waves and sorted(set(info["L"])) == [5, wide]
        _oracle_same(orc, data + (1.0, n_bins, 1.0, 68.34), want, f"reuse.{wide}.{n_bins}")


def test_capacity_classes():
    assert [H.capacity_class(n) for n in (1, 1024, 1025, 4096, 4097, 8192, 8193, 1 << 24, (1 << 24) + 1)] == \
        [1024, 1024, 4096, 4096, 8192, 8192, "scratch", "scratch", "refused"]
    assert (H.waves_per_launch(1024, 256), H.waves_per_launch(4096, 256), H.waves_per_launch("scratch", 256)) == (32768, 8192, 2048)


def test_table_reaches_its_edges():
    """The window lengths, levels per bar and levels per window the table is meant to sit on are really there."""
    for k in (1, 2, 62, 63, 64, 65, 125, 126, 127, 190):
        (_, info) = H.expected(f"winlen.{k}.k1")
        lens = np.array(info["e"]) - np.array(info["s"])
        assert info["first"] == k - 1 and lens[0] == k and lens[-1] == k and info["e"][-1] == k + 6, k
    off = H.inputs("bar_widths.k1")[3]
    assert set(np.diff(off)) >= {0, 1, 63, 64, 65, 127, 128, 129, 200}
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 20_000):
        assert H.expected(f"levels.{n}.raw")[1]["L"] == [n]
    for wide in (1025, 8193):
        assert sorted(set(H.expected(f"one_wide.{wide}.raw")[1]["L"])) == [5, wide]
    (_, info) = H.expected("place.gaps.w5.k1")
    assert 1 in set(np.array(info["e"]) - np.array(info["s"]))
    (out, info) = H.expected("place.regular.w100.k1")
    assert info["first"] == 40 and not any(a.any() for a in out)
    (_, info) = H.expected("place.dup.w0.k1")                      # three bars a stamp: every window holds all three
    assert set(np.array(info["e"][:36]) - np.array(info["s"][:36])) == {3} and info["first"] == 0
    (_, info) = H.expected("place.edge.w5.k1")                     # gaps 2, 3: the bar at end - 5 s is in the window
    assert set(np.array(info["e"]) - np.array(info["s"])) == {3}
    (_, info) = H.expected("chunk_empties.k1")
    assert set(np.array(info["e"]) - np.array(info["s"])) == {130}
    for tick in (1.0, 0.5, 0.25):                                # ties go to the even level: (10.5, 13.5) -> 10 .. 14, (11.5, 14.5) -> 12 .. 14
        assert H.expected(f"half_tick.{tick}.w0")[1]["L"][:2] == [5, 3]
    assert H.level_of(-0.5, 1.0) == 0 and H.level_of(-3.5, 1.0) == -4 and H.level_of(2.5, 1.0) == 2
    (_, info) = H.expected("near_half_cent.w0")
    assert info["L"] == [1211 - 1203 + 1, 1211 - 1205 + 1, 1215 - 1207 + 1, 1215 - 1207 + 1], info["L"]   # below .5 down, above up


def test_bins_of_the_table():
    """Widths raised from 0, 2 and 4 and an odd one, with and without the leftover bin; bin counts at the 64-lane stride; a last bin
    whose centre lies above the maximum."""
    assert H.bin_layout(0, 4, 5) == (1, 4) and H.bin_layout(0, 10, 5) == (3, 4) and H.bin_layout(0, 20, 5) == (5, 4)
    assert H.bin_layout(0, 15, 5) == (3, 5) and H.bin_layout(0, 16, 5) == (3, 6)
    seen = set()
    for name in H.names():
        c = H.CASES[name]
        if c["one"] and c["n_bins"] is not None and c["build"][0] == "three_bars":
            n = c["build"][1]["n_levels"]
            lv, tot = H.bucket_price_levels(np.arange(n, dtype=np.int32), np.ones(n, np.float32), c["n_bins"])
            width, nb = H.bin_layout(0, n - 1, c["n_bins"])
            leftover = len(lv) == nb + 1
            assert leftover == ((n - 1) % width == 0) and np.all(np.diff(lv) > 0)
            seen.add((width, leftover, len(lv)))
            if lv[-1] > n - 1:
                seen.add("centre above the maximum")
            if leftover:
                assert lv[-1] == n - 1 and tot[-1] == 1.0
    assert {w for w, *_ in seen - {"centre above the maximum"}} >= {1, 3, 5, 7}
    assert {k for _, _, k in seen - {"centre above the maximum"}} >= {63, 64, 65, 129} and "centre above the maximum" in seen
    assert {lo for _, lo, _ in seen - {"centre above the maximum"}} == {True, False}


def test_refusals(orc, manifest):
    """The restatement and the oracle refuse what the table says; what the reference itself did is on record."""
    ref = manifest["refused"]
    assert set(ref) == set(H.REFUSALS)
    for name, c in H.REFUSALS.items():
        a = c["inputs"] + (c["window"], c["n_bins"], c["tick"], c["va"])
        if name == "above_16m_levels":
            continue                                             # the product's capacity: neither restated nor in the oracle
        with pytest.raises(c["error"]):
            H.volume_profile_rolling(*a)
        with pytest.raises(c["error"]):
            orc.volume_profile_rolling(*a)
    # the reference: raises for a NaN low or high and for a level above the range; folds a level below onto the lowest one; in its
    # interpreted mode NumPy's integer division by zero gives 0 (the typed function raises ZeroDivisionError) and a one-level window
    # comes back as one bin (include/fmk.h keeps refusing it)
    assert all(ref[k]["reference"] == "ValueError" and "NaN" in ref[k]["message"] for k in ref if k.startswith("nan_"))
    assert ref["level_above.first64"]["reference"] == ref["level_above.rest"]["reference"] == "IndexError"
    assert ref["level_below.first64"]["reference"] == ref["level_below.rest"]["reference"] == "returns"
    assert ref["tick_0"]["reference"] == "OverflowError" and ref["tick_nan"]["reference"] == "ValueError"
    with pytest.raises(AssertionError):
        H.volume_profile_rolling(*(a[:0] for a in H.three_bars(5, 1, 1)[:3]), np.zeros(1, np.int64), *(a[:0] for a in H.three_bars(5, 1, 1)[4:]),
                                 1.0, None, 1.0)
    want = H.volume_profile_rolling(*H.NAN_UNUSED, 2.0, None, 1.0)   # a NaN low that no computed window holds is not looked at
    for k, x, y in zip(KEYS, orc.volume_profile_rolling(*H.NAN_UNUSED, 2.0, None, 1.0), want):
        H.same(x, y, "nan_unused:" + k)
    assert want[0][0] == 0 and want[0][1:].all()
