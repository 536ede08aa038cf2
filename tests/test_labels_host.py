"""CPU-only checks of the label feature: the NumPy helper the GPU tests compare with reproduces the reference's recorded outputs
(tests/golden/labels.npz), the C ABI declares and exports the new entry points, finmlkit_amd.label imports and refuses to work
without a device, and the O(events) host functions compute what finmlkit/label/weights.py does."""
import json
import os
import re

import numpy as np
import pytest

from tests import _label_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ["fmk_triple_barrier_dev", "fmk_triple_barrier", "fmk_label_concurrency_dev", "fmk_label_concurrency",
           "fmk_label_weights_dev", "fmk_label_weights"]


def load_cases():
    z = np.load(os.path.join(GOLD, "labels.npz"))
    man = json.load(open(os.path.join(GOLD, "labels.json")))
    cases = {}
    for name, m in man.items():
        c = {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(name + ".")}
        c.update(seed=m["seed"], n=m["n"], hb=(float(m["horizontal_barriers"][0]), float(m["horizontal_barriers"][1])),
                 vb=float(m["vertical_barrier"]), mc=m["min_close_time_sec"], min_ret=m["min_ret"])
        c.setdefault("side", None)
        cases[name] = c
    return cases


CASES = load_cases()


def load_odd():
    """tests/golden/labels_odd.*: planted tapes (stored), label cases and weights cases recorded from the reference."""
    z = np.load(os.path.join(GOLD, "labels_odd.npz"))
    man = json.load(open(os.path.join(GOLD, "labels_odd.json")))
    tapes = {k[5:-3]: (z[k], z[k[:-3] + ".close"]) for k in z.files if k.startswith("tape_") and k.endswith(".ts")}
    cases, weights = {}, {}
    for name, m in man.items():
        if name.startswith("_"):
            continue
        c = {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(name + ".")}
        c["ts"], c["close"] = tapes[m["tape"]]
        if m.get("weights"):
            weights[name] = c
            continue
        c.update(hb=(float(m["horizontal_barriers"][0]), float(m["horizontal_barriers"][1])), vb=float(m["vertical_barrier"]),
                 mc=m["min_close_time_sec"], min_ret=m["min_ret"], meta=m["meta"], n_skipped=m["skipped"],
                 made_for_skipping=m["made_for_skipping"])
        c.setdefault("side", None)
        cases[name] = c
    return cases, weights, man


ODD, ODD_WEIGHTS, ODD_MANIFEST = load_odd()
# the least the odd-value fixture has to exercise, over all its recorded events
ODD_MINIMA = {"base_minus_inf": 8, "base_plus_inf": 8, "base_nan": 8, "nan_inside_path": 50, "touch_at_infinite_return": 20,
              "side_zero": 20, "target_nan": 10, "target_zero": 10, "target_negative": 10, "target_infinite": 10,
              "two_whole_blocks_in_window": 100}


def same_bits(got, want):
    """bit for bit, the sign of an infinity and of a zero included; every NaN equals every NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind == "f":
        return bool(np.all((got.view("u8") == want.view("u8")) | (np.isnan(got) & np.isnan(want))))
    return bool(np.array_equal(got, want))


def rel_close(got, want, rtol):
    got, want = np.asarray(got), np.asarray(want)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all(both_nan | (np.abs(got - want) <= rtol * np.abs(want))))


def test_fixture_covers_the_cases_of_the_issue():
    assert {"symmetric", "meta", "upper_disabled", "vertical_inf", "tight", "wide", "unsorted", "concurrent"} <= set(CASES)
    for name, c in CASES.items():
        assert len(c["event_idx"]) >= 1000 and c["n"] >= 200_000, name
        assert c["skipped"].sum() * 100 < len(c["event_idx"]), name
    c = CASES["tight"]
    assert (c["touch_idx"] == c["event_idx"] + 1).sum() * 2 > len(c["event_idx"])     # most touch at their first tick
    assert (CASES["wide"]["ratios"] != 1.0).sum() * 2 > len(CASES["wide"]["ratios"])
    assert np.any(np.diff(CASES["unsorted"]["event_idx"]) < 0)
    assert set(np.unique(CASES["meta"]["side"])) == {-1, 0, 1}
    conc = CASES["concurrent"]["concurrency"]
    assert np.median(conc[conc > 0]) >= 50


@pytest.mark.parametrize("name", sorted(CASES))
def test_helper_reproduces_the_reference(orc, name):
    c = CASES[name]
    ts, px, _, _ = orc.synth(c["seed"], 0, c["n"])
    lab, tch, ret, rat, skipped = H.triple_barrier(ts, px, c["event_idx"], c["targets"], c["hb"], c["vb"], c["mc"], c["side"],
                                                   c["min_ret"])
    ok = ~c["skipped"]
    assert np.array_equal(skipped, c["skipped"])
    assert np.array_equal(lab[ok], c["labels"][ok]) and np.array_equal(tch[ok], c["touch_idx"][ok])
    tol = 4 * 2.0 ** -52 * np.abs(np.log(px)).max()
    d = np.abs(ret[ok] - c["returns"][ok])
    print(name, "max |ret - ref|", d.max(), "tol", tol)
    assert d.max() <= tol
    assert rel_close(rat[ok], c["ratios"][ok], 1e-12)
    avg, conc = H.average_uniqueness(ts, c["event_idx"], c["touch_idx"])
    assert np.array_equal(conc, c["concurrency"]) and conc.dtype == np.int16
    assert rel_close(avg, c["avg_uniqueness"], 1e-12)
    att, bound = H.return_attribution(c["event_idx"], c["touch_idx"], px, conc, False)
    assert np.all(np.abs(att - c["return_attribution"]) <= bound)
    attn, _ = H.return_attribution(c["event_idx"], c["touch_idx"], px, conc, True)
    scale = len(att) / att.sum()
    assert np.all(np.abs(attn - c["return_attribution_norm"]) <= bound * scale + 1e-12 * attn)


def test_host_log_is_the_hosts_log_extended():
    import math
    assert H.host_log(0.0) == -math.inf and H.host_log(-0.0) == -math.inf and H.host_log(math.inf) == math.inf
    assert math.isnan(H.host_log(-5.0)) and math.isnan(H.host_log(-math.inf)) and math.isnan(H.host_log(math.nan))
    assert H.host_log(5e-324) == math.log(5e-324) and H.host_log(101.25) == math.log(101.25)
    col = H.log_column(np.array([0.0, -1.0, 2.0, math.inf]))
    assert col[0] == -math.inf and math.isnan(col[1]) and col[2] == math.log(2.0) and col[3] == math.inf


@pytest.mark.parametrize("which", ["scalar", "vectorised"])
@pytest.mark.parametrize("name", sorted(ODD))
def test_odd_fixture_against_the_yardstick(name, which):
    """Every event of the fixture, all four outputs and the skipped mask, bit for bit: the events recorded from the reference
    and the ones it cannot answer (side=None with a NaN final return), which the fixture holds by the project's definition."""
    c = ODD[name]
    fn = H.triple_barrier_scalar if which == "scalar" else H.triple_barrier
    got = fn(c["ts"], c["close"], c["event_idx"], c["targets"], c["hb"], c["vb"], c["mc"], c["side"], c["min_ret"])
    assert same_bits(got[4], c["skipped"]) and int(got[4].sum()) == c["n_skipped"]
    for g, k in zip(got, ("labels", "touch_idx", "returns", "ratios")):
        assert same_bits(g, c[k]), f"{name}/{which}/{k}"
    rec = c["recorded"]
    assert c["meta"] and rec.all() or not c["meta"] and (~rec).sum() * 10 <= len(rec)
    assert np.all(np.isnan(c["returns"][~rec])) and np.all(c["labels"][~rec] == 1)         # the project's definition
    assert c["made_for_skipping"] or c["n_skipped"] * 100 <= len(rec)


def test_odd_fixture_covers_the_cases_of_the_issue():
    totals = dict.fromkeys(ODD_MINIMA, 0)
    for name, m in ODD_MANIFEST.items():
        if not name.startswith("_") and not m.get("weights"):
            for k in totals:
                totals[k] += m["counts"][k]
    print(totals)
    assert totals == ODD_MANIFEST["_totals"]
    assert not {k: v for k, v in totals.items() if v < ODD_MINIMA[k]}
    # what can be counted from the arrays alone, counted again
    side_zero = targets = 0
    for c in ODD.values():
        live = c["recorded"] & ~c["skipped"]
        side_zero += int((c["side"][live] == 0).sum()) if c["side"] is not None else 0
        targets += int(np.isnan(c["targets"][live]).sum())
    assert side_zero == totals["side_zero"] and targets == totals["target_nan"]
    assert {c["hb"] for c in ODD.values()} >= {(1.0, 1.0), (0.0, 0.0), (np.inf, 1.0), (1.0, np.inf)}
    assert any(min(c["hb"]) < 0 for c in ODD.values()) and {c["mc"] == 0 for c in ODD.values()} == {True, False}
    assert {np.isinf(c["vb"]) for c in ODD.values()} == {True, False}
    for ts, px in {id(c["ts"]): (c["ts"], c["close"]) for c in ODD.values()}.values():
        assert len(ts) == 6 * 1024 + 37 and ts[0] > 1.6e18 and (np.diff(ts) == 0).sum() > 10 and np.all(np.diff(ts) >= 0)
        assert np.any(ts.astype(np.float64).astype(np.int64) != ts)                        # float64(ts) rounds
        assert np.isnan(px).any() and (px == 0).any() and (px < 0).any() and np.isinf(px).any()
    zero = ODD["zero_sym"]["close"]
    assert np.signbit(zero[zero == 0]).any() and ((zero > 0) & (zero < 2.3e-308)).any()   # -0.0 and a subnormal
    for name, w in ODD_WEIGHTS.items():
        whole = (w["touch_idx"] + 1) // 1024 - (w["event_idx"] + 1023) // 1024
        assert {0, 1, 2, 3, 4, 5} <= set(np.maximum(whole, 0).tolist()), name
        hand = w["hand_concurrency"]
        for k in range(1, 6):                                    # runs of 0 or of negative counts across every block boundary
            assert np.all(hand[k * 1024 - 2:k * 1024 + 2] <= 0), name
        assert (hand == 0).any() and (hand < 0).any()


@pytest.mark.parametrize("name", sorted(ODD_WEIGHTS))
def test_odd_weights_fixture_against_the_yardstick(name):
    w = ODD_WEIGHTS[name]
    avg, conc = H.average_uniqueness(w["ts"], w["event_idx"], w["touch_idx"])
    assert same_bits(conc, w["concurrency"]) and same_bits(avg, w["avg_uniqueness"])
    for cc, key in ((w["concurrency"], "return_attribution"), (w["hand_concurrency"], "return_attribution_hand")):
        att, bound = H.return_attribution(w["event_idx"], w["touch_idx"], w["close"], cc, False)
        fin = np.isfinite(w[key])
        assert fin.sum() >= 20 and (~fin).sum() >= 20
        assert np.all(np.abs(att[fin] - w[key][fin]) <= bound[fin]) and same_bits(att[~fin], w[key][~fin])


def test_header_declares_and_library_exports_the_label_entry_points():
    from finmlkit_amd import _ffi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmk.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fmk_[a-z0-9_]+)\s*\(", txt))
    assert not [s for s in SYMBOLS if s not in declared]
    assert not [s for s in SYMBOLS if not hasattr(_ffi.lib(), s)]
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmk_diag.h")).read(), flags=re.S)
    assert "fmk_diag_label_last" in diag and hasattr(_ffi.lib(), "fmk_diag_label_last")
    assert _ffi.lib().fmk_abi_version() == 1


def test_label_package_has_the_reference_names():
    from finmlkit_amd import label
    for name in ("triple_barrier", "average_uniqueness", "return_attribution", "time_decay", "class_balance_weights", "TBMLabel",
                 "SampleWeights"):
        assert hasattr(label, name)


def test_label_package_has_no_cpu_fallback():
    from finmlkit_amd import _ffi, label
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is present")
    ts = np.arange(10, dtype=np.int64) * 10 ** 9
    px = np.linspace(100.0, 101.0, 10)
    with pytest.raises(_ffi.FmkError):
        label.triple_barrier(ts, px, np.array([0]), np.array([0.01]), (1.0, 1.0), 5.0, 0.0, None, 0.0)
    with pytest.raises(_ffi.FmkError):
        label.average_uniqueness(ts, np.array([0]), np.array([3]))


def test_reference_test_calls_on_the_host():
    """tests/golden/label_refcalls.*: time_decay, class_balance_weights, compute_final_weights (values 1e-12 relative) and every
    argument check (exception type and message) of the calls the reference's own tests/labels make; the rest needs the device
    (tests/test_gpu_labels.py)."""
    from finmlkit_amd import label
    from tests import _label_refcalls as L
    c = L.replay(label, only_host=True)
    print(c)
    assert c["calls_total"] >= 120 and c["calls_raising"] == 10
    assert c["calls_replayed"] >= 23 + 12 + 1 + 10                # time_decay (one of its 24 raises), class balance, final, checks


def test_argument_checks_come_before_the_device():
    from finmlkit_amd import label
    ts = np.arange(10, dtype=np.int64)
    px = np.ones(10)
    ev, tg = np.array([1, 2]), np.array([0.1, 0.1])
    for kw, msg in ((dict(vertical_barrier=0.0), "The vertical barrier must be greater than zero."),
                    (dict(min_ret=-1.0), "The minimum return must be non-negative."),
                    (dict(close=px[:5]), "The lengths of timestamps and close must match."),
                    (dict(targets=tg[:1]), "The lengths of event_idxs and targets must match."),
                    (dict(event_idxs=ev[:0], targets=tg[:0]), "The event_idxs array must not be empty."),
                    (dict(side=np.array([1], np.int8)), "The length of event_idxs must match the length of side.")):
        args = dict(timestamps=ts, close=px, event_idxs=ev, targets=tg, horizontal_barriers=(1.0, 1.0), vertical_barrier=1.0,
                    min_close_time_sec=0.0, side=None, min_ret=0.0)
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(msg)):
            label.triple_barrier(**args)
    with pytest.raises(ValueError, match="must have the same length"):
        label.average_uniqueness(ts, ev, ev[:1])
    w, c = label.average_uniqueness(ts, ev[:0], ev[:0])          # an empty event list is legal: no device needed
    assert w.shape == (0,) and c.dtype == np.int16 and not c.any() and len(c) == 10


def test_time_decay_and_class_balance():
    from finmlkit_amd.label import class_balance_weights, time_decay
    u = np.array([0.5, 0.25, 0.25, 1.0])
    np.testing.assert_allclose(time_decay(u, 1.0), np.ones(4), rtol=1e-12)
    w = time_decay(u, 0.5)                                       # linear in the cumulated uniqueness, newest = 1
    cum = np.cumsum(u)
    np.testing.assert_allclose(w, 0.5 + 0.5 * cum / cum[-1], rtol=1e-12)
    w = time_decay(u, -0.5)                                      # the oldest half of the cumulated uniqueness is erased
    np.testing.assert_allclose(w, np.maximum(0.0, 1 - (cum[-1] - cum) / (0.5 * cum[-1])), rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError, match=re.escape("last_weight must lie in [-1, 1]")):
        time_decay(u, 1.5)
    with pytest.raises(ValueError, match="must be grater than 0"):
        time_decay(np.zeros(3), 0.5)
    labels = np.array([1, -1, 1, 1, -1], np.int8)
    base = np.array([1.0, 2.0, 3.0, 4.0, 2.0])
    classes, cw, size, final = class_balance_weights(labels, base)
    assert classes.tolist() == [-1, 1] and classes.dtype == np.int8
    np.testing.assert_allclose(size, [4.0, 8.0], rtol=1e-12)
    np.testing.assert_allclose(cw, [12.0 / (2 * 4.0), 12.0 / (2 * 8.0)], rtol=1e-12)
    np.testing.assert_allclose(final, base * np.where(labels == -1, 1.5, 0.75), rtol=1e-12)


def test_product_does_not_import_the_test_helper():
    bad = []
    for dp, _, fns in os.walk(os.path.join(ROOT, "finmlkit_amd")):
        for fn in fns:
            if fn.endswith(".py") and re.search(r"_label_ref|^\s*(from|import)\s+(oracle|tests)\b",
                                                open(os.path.join(dp, fn)).read(), flags=re.M):
                bad.append(fn)
    assert not bad, bad
