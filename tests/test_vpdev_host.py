"""The developing volume profile on hand-built footprints, host side: the restatement (tests/_vpdev_ref.py) against what the
reference recorded on them (tests/golden/vpdev_edges.npz, made by tools/gen_vpdev_golden.py), the float32 rounding emulation against
np.round, and the package's trim_trailing_zeros against the recorded reference outputs.  No GPU."""
import json
import os

import numpy as np
import pytest

from tests import _vp_ref as H
from tests import _vpdev_ref as D

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("poc", "hva", "lva")


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLD, "vpdev_edges.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLD, "vpdev_edges.npz")) as z:
        return {k: z[k] for k in z.files}


def test_manifest_covers_the_table_and_hashes_match(manifest):
    """Every exact-volume case is recorded, every other case is recorded or named as left out (at most 5 % of them), and the inputs
    built here are the ones the reference saw."""
    cases = manifest["cases"]
    assert set(D.names(kind=1)) <= set(cases)
    inexact = set(D.names(kind=2)) | set(D.names(kind=3))
    assert inexact == (set(cases) - set(D.names(kind=1))) | set(manifest["left_out"])
    assert len(manifest["left_out"]) <= 0.05 * len(inexact) and len(cases) >= 280
    assert sorted(n for g in D.GROUPS for n in D.group(g)) == sorted(D.CASES)
    for name, m in cases.items():
        c = D.CASES[name]
        assert m["input_sha256"] == D.input_hash(name), name
        assert (m["n_bins"], m["tick"], m["va"], m["kind"]) == (c["n_bins"], c["tick"], c["va"], c["kind"]), name
        assert m["lens"] == [e - s for s, e in D.bar_ranges(name)], name
    for name, r in manifest["refused"].items():
        if "input_sha256" in r:
            assert r["input_sha256"] == H.sha256(*{**D.REFUSALS, **D.RETURNS}[name]["inputs"]), name
    assert os.path.getsize(os.path.join(GOLD, "vpdev_edges.npz")) <= 4768      # what vp_edges.npz took when this file was added


def test_restatement_equals_the_recorded_reference(manifest, recorded):
    n = 0
    for name, m in manifest["cases"].items():
        own, _info = D.expected(name)
        at = m["at"]
        for (ts, *out), ln, (s, e) in zip(own, m["lens"], D.bar_ranges(name)):
            H.same(ts, D.inputs(name)[0][s:e], name + ":ts")
            for k, a in zip(KEYS, out):
                H.same(a, recorded[k][at:at + ln], f"{name}:{k}")
                n += ln
            at += ln
    assert n == 3 * sum(sum(m["lens"]) for m in manifest["cases"].values()) >= 8000


def test_recorded_walks_clear_the_threshold(manifest):
    gaps = [m["walk_gap"] for m in manifest["cases"].values() if m["kind"] == 1 and m["walk_gap"] is not None]
    assert len(gaps) > 150 and min(gaps) > 0.0


def test_table_reaches_its_edges():
    """Range lengths round the forced chunk lengths, levels per bar, all capacity classes, the trim's cases and the one-level rule."""
    lens = {e - s for n in D.group("chunk") for s, e in D.bar_ranges(n)}
    assert lens >= {k + d for k in (1, 2, 7, 64) for d in (-1, 0, 1) if k + d >= 1} | {2 * k + 1 for k in (1, 2, 7, 64)} | {200}
    assert set(np.diff(D.inputs("bar_widths.raw.k1")[3])) >= {0, 1, 63, 64, 65, 127, 128, 129, 200}
    empty = np.flatnonzero(np.diff(D.inputs("empties.raw.k1")[3]) == 0)
    assert {int(x) % 7 for x in empty} >= {0, 3, 6} and {int(x) % 2 for x in empty} == {0, 1} and 0 in empty
    classes = {D.capacity_class(max(D.expected(n)[1]["L"])) for n in D.group("levels")}
    assert classes == {1024, 4096, 8192, "scratch"}
    assert [D.expected(f"levels.{n}.raw")[1]["L"] for n in (1, 8193, 20_000)] == [[1], [8193], [20_000]]
    tiny = D.round8(np.array([3e-9, 5e-9, 1.5e-8], np.float32))
    assert tiny[0] == 0 and tiny[1] == 0 and tiny[2] == np.float32(2e-8)
    ts, hi, lo, off, lv, bv, sv = D.inputs("trim.by_one.5")
    widths = []
    ab = np.zeros(40, np.float32)
    for t in range(len(ts)):
        ab[lv[off[t]:off[t + 1]] - 100] += bv[off[t]:off[t + 1]]
        widths.append(len(D.trim_trailing_zeros(np.arange(100, 140), ab)[0]))
    assert widths == list(range(1, 13))
    (_, poc, hva, lva), = D.expected("trim.lowest.5")[0]
    assert set(poc) == set(hva) == set(lva) == {100}
    (_, poc, hva, lva), = D.expected("one_level.several.b27")[0]
    assert (poc[:3] == 120).all() and (hva[:3] == 120).all() and (lva[:3] == 120).all() and hva[3] > lva[3]
    assert D.bar_ranges("ranges.between_bars") == [(4, 20)] and D.bar_ranges("ranges.duplicate_stamps") == [(3, 12)]
    assert len(D.bar_ranges("ranges.fifty")) == 50 and {e - s for s, e in D.bar_ranges("ranges.fifty")} <= set(range(1, 10))


def test_rounding_emulation_is_np_round_bit_for_bit():
    x = D.round_probe()
    assert x.dtype == np.float32 and len(x) > 25000
    with np.errstate(over="ignore", invalid="ignore"):
        want = np.round(x, 8)
    assert want.dtype == np.float32
    H.same(D.round8(x), want, "round8")
    assert (want != x).sum() > 0.2 * len(x)                       # it is no identity: it cannot be skipped


def test_trim_trailing_zeros_equals_the_recorded_reference(manifest, recorded):
    from finmlkit_amd.feature.core.volume import trim_trailing_zeros
    at = 0
    flat = recorded["trim"]
    assert len(manifest["trims"]) == len(D.TRIM_PROFILES)
    for j, v in enumerate(D.TRIM_PROFILES):
        m = manifest["trims"][f"trim{j}"]
        assert (m["n_in"], m["dtype"]) == (len(v), v.dtype.name)
        H.same(flat[at:at + m["n_in"]].astype(v.dtype), v, f"trim{j}: input")
        at += m["n_in"]
        levels, vols = flat[at:at + m["n_out"]].astype(np.int32), flat[at + m["n_out"]:at + 2 * m["n_out"]].astype(v.dtype)
        at += 2 * m["n_out"]
        got = trim_trailing_zeros(np.arange(100, 100 + len(v), dtype=np.int32), v)
        H.same(got[0], levels, f"trim{j}: levels")
        H.same(got[1], vols, f"trim{j}: volumes")
        if v.dtype == np.float32:
            own = D.trim_trailing_zeros(np.arange(100, 100 + len(v), dtype=np.int32), v)
            H.same(own[0], levels, f"trim{j}: restated levels")
            H.same(own[1], vols, f"trim{j}: restated volumes")
    assert at == len(flat)


def test_refusals_of_the_restatement_and_the_reference_on_record(manifest):
    ref = manifest["refused"]
    assert set(ref) == set(D.REFUSALS) | set(D.RETURNS)
    for name, c in D.REFUSALS.items():
        if name == "above_16m_levels":
            continue                                             # the product's capacity, not restated
        with pytest.raises(c["error"], match=c["message"] if c["code"] in ("E_LEVEL", "E_ZERODIV") or name == "empty_range" else None):
            D.volume_profile_developing(*c["inputs"], *D.refusal_stamps(c), c["n_bins"], c["tick"], c["va"])
    for name in ("empty_range", "nan_low", "nan_high", "tick_nan", "all_zero_first_bar.bins", "all_zero_later_start.bins"):
        assert ref[name]["reference"] == "ValueError", name
    for name, c in D.RETURNS.items():
        assert ref[name]["reference"] == "returns"
        s, e = c["span"]
        own = D.developing_range(*c["inputs"][1:], s, e, c["n_bins"], c["tick"], c["va"])
        for k, a in zip(KEYS, own):
            H.same(a, np.array(ref[name][k], np.int32), f"{name}:{k}")
    lowest = H.level_of(np.min(D.RETURNS["all_zero_first_bar.raw"]["inputs"][2]), 1.0)
    assert ref["all_zero_first_bar.raw"]["poc"][0] == lowest       # the argmax of zeros is 0
