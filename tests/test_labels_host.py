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
