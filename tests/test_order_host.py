"""CPU-only: the windowed order statistics (comp_burst_ratio, stoch_k, roc, pct_change).  Both forms of the plain restatement
(tests/_order_ref.py) against the reference's recorded outputs (tests/golden/order_stats.npz, written by tools/gen_order_golden.py
from the untouched reference), the regenerated series against their recorded hashes, the argument checks of the host layer, which
need no device, the signatures, and the library's symbols.  Every comparison is bit for bit, NaN positions included, and for burst
ratio, roc and pct_change in the sign of every zero.  Cases of more than 2100 elements record the hash of the reference's output
instead of the output: the vector form is held against the hash at full size (expected())."""
import inspect
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _order_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "order_stats.json")))
_NPZ = np.load(os.path.join(GOLD, "order_stats.npz"))

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)
GENERATORS = {"grid_walk": H.grid_walk, "tie_sizes": H.tie_sizes, "distinct_sizes": H.distinct_sizes, "ohlc_walk": H.ohlc_walk,
              "signed_sizes": H.signed_sizes, "alternating_sizes": H.alternating_sizes, "signed_ohlc_walk": H.signed_ohlc_walk}
VALUE_CLASS_CASES = [k for k in OK_CASES if k.split(".")[0] in ("signed", "alt", "hostile")]
SCALAR_MAX = 4000                      # above this window the scalar form is slow: the vector form alone is gated (as at generation)
_HASHED = {}
ENTRIES = ("fmk_burst_ratio", "fmk_stoch_k", "fmk_roc", "fmk_pct_change")


def product():
    """The package's four functions under the reference's names."""
    from finmlkit_amd.feature.core.momentum import roc, stoch_k
    from finmlkit_amd.feature.core.utils import comp_burst_ratio, pct_change
    return SimpleNamespace(comp_burst_ratio=comp_burst_ratio, stoch_k=stoch_k, roc=roc, pct_change=pct_change)


def case_input(name):
    """The inputs of a fixture case: stored, or regenerated from the case's seed.  One series, or (close, low, high) for %K."""
    c = MANIFEST[name]
    src = c.get("source")
    if src is None:
        ins = tuple(_NPZ[f"{name}.in{k}"] for k in range(3 if c["fn"] == "stoch" else 1))
    else:
        made = GENERATORS[src["gen"]](*src["args"])
        ins = tuple(made) if isinstance(made, tuple) else (made,)
    return ins if c["fn"] == "stoch" else ins[0]


def expected(name):
    """The reference's recorded output, or, for a case that records its hash alone, the vector form of the restatement after its
    hash has been found equal to the recorded one."""
    if name + ".out" in _NPZ.files:
        return _NPZ[name + ".out"]
    if name not in _HASHED:
        c = MANIFEST[name]
        out = H.call(c["fn"], case_input(name), c["arg"], form="vector")
        assert H.sha256(H.nan_canonical(out)) == c["output_sha256"], name
        out.setflags(write=False)
        _HASHED[name] = out
    return _HASHED[name]


def call(name, **kw):
    c = MANIFEST[name]
    return H.call(c["fn"], case_input(name), c["arg"], **kw)


def same(got, want):
    return np.asarray(got).dtype == np.float64 and np.array_equal(got, want, equal_nan=True)


def same_bits(got, want):
    """same(), and every zero has the sign of its counterpart."""
    return same(got, want) and np.array_equal(np.signbit(got) | np.isnan(got), np.signbit(want) | np.isnan(want))


def test_fixture_holds_what_it_should():
    assert {c["fn"] for c in MANIFEST.values()} == {"burst", "stoch", "roc", "pct"}
    burst = {k: c for k, c in MANIFEST.items() if c["fn"] == "burst" and k in OK_CASES}
    for group, windows in (("walk.", {1, 2, 3, 7, 8, 50, 51, 200, 1000}), ("ties.", {1, 2, 3, 4, 50, 51, 64, 65, 200, 1000}),
                           ("distinct.", {1, 2, 5, 50, 101})):
        assert windows <= {c["arg"] for k, c in burst.items() if k.startswith(group)}, group
    assert len(set(H.tie_sizes(1200, 530))) == 8 and len(set(H.distinct_sizes(1200, 550))) == 1200
    assert len([k for k in MANIFEST if k.startswith("refcall.")]) == 4 and len(REFUSED) == 7
    # NaN runs shorter and longer than the window: 3 + 40 NaN, and every window that touches one gives NaN
    x = case_input("odd.burst_w20")
    assert np.isnan(x).sum() == 43 and np.isinf(x).sum() == 5 and (x == 0).sum() == 2 and (x < 0).sum() >= 2
    for w in (20, 21):
        out = expected(f"odd.burst_w{w}")
        assert np.isnan(out[50:52 + w]).all() and np.isnan(out[150:189 + w]).all() and np.isfinite(out[120:150]).all()
    assert np.isnan(expected("odd.burst_w3")[502]) and expected("odd.burst_w2")[301] == 0.0         # inf / inf, x / inf
    assert np.isnan(expected("refcall.burst_zero_median")[2]) and MANIFEST["zero.burst_w9"]["nan"] > 100
    for n, finite in ((0, 0), (1, 0), (9, 0), (10, 1), (11, 2)):
        assert MANIFEST[f"length.n{n}.burst"]["finite"] == finite and len(expected(f"length.n{n}.burst")) == n
        assert MANIFEST[f"length.n{n}.stoch"]["finite"] == finite
        assert MANIFEST[f"length.n{n}.burst_w11"]["finite"] == max(0, n - 10)
    assert MANIFEST["held.stoch_l2"]["nan"] > 500 and MANIFEST["walk.stoch_l14"]["nan"] == 13
    for k in OK_CASES:
        if MANIFEST[k]["fn"] == "stoch":
            assert not any(np.isnan(a).any() for a in case_input(k)[1:]), k
    assert os.path.getsize(os.path.join(GOLD, "order_stats.npz")) < 1_000_000


def test_regenerated_series_hash_to_the_recorded_ones():
    seen = 0
    for name, c in MANIFEST.items():
        if "source" in c:
            ins = case_input(name)
            ins = ins if isinstance(ins, tuple) else (ins,)
            assert [H.sha256(a) for a in ins] == c["input_sha256"], name
            assert all(len(a) == c["n"] for a in ins)
            seen += 1
    assert seen > 50


@pytest.mark.parametrize("name", OK_CASES)
def test_both_forms_equal_the_reference(name):
    want = expected(name)                                        # (a hashed case: the vector form itself, checked against the hash)
    eq = same if MANIFEST[name]["fn"] == "stoch" else same_bits  # %K: the sign of a zero is not the reference's to give
    assert eq(call(name, form="vector"), want), name
    if MANIFEST[name]["arg"] <= SCALAR_MAX:
        assert eq(call(name, form="scalar"), want), name


def test_value_class_series_are_what_they_claim():
    x = H.signed_sizes(20_000, 640)
    mags = np.abs(x[np.isfinite(x) & (np.abs(x) > 1e-300) & (x != H.HOSTILE[6])])
    assert not np.isnan(x).any() and len(set(mags)) == len(mags) > 18_000
    assert 0.40 < (np.signbit(x)).mean() < 0.50
    for v in H.HOSTILE:
        hit = (x == v) & (np.signbit(x) == np.signbit(v))
        assert 100 < hit.sum() < 320, v                         # about 1 % each
    a = H.alternating_sizes(9001, 5)
    assert (a[0::2] < 0).all() and (a[1::2] > 0).all() and len(set(np.abs(a))) == 9001
    assert np.array_equal(np.abs(a), np.abs(H.alternating_sizes(9001, 5))) and np.isfinite(a).all()
    c, lo, hi = H.signed_ohlc_walk(8756, 662)
    assert (c < 0).sum() > 500 and (c > 0).sum() > 500 and (lo <= c).all() and (c <= hi).all()
    assert lo[40] == -np.inf and hi[-41] == np.inf and np.isinf(lo).sum() == np.isinf(hi).sum() == 1
    c, lo, hi = H.signed_ohlc_walk(526, 21, True)
    assert (lo <= hi).all() and not any(np.isnan(v).any() for v in (c, lo, hi))
    for v in H.HOSTILE:
        assert ((lo == v) | (hi == v)).any(), v


def test_value_class_cases_check_something():
    """Shares that the reference's outputs alone decide: an alternating series gives a quarter and more of finite and of NaN outputs
    among the full windows at every window (an even window's median changes sign with the seed), %K cases are finite in more than
    half of them, and the signed sizes give infinite, zero and negative-zero outputs."""
    assert len(VALUE_CLASS_CASES) == 31
    for name in VALUE_CLASS_CASES:
        c = MANIFEST[name]
        out = expected(name)[c["arg"] - 1 if c["fn"] in ("burst", "stoch") else c["arg"]:]
        finite, nan = np.isfinite(out).sum(), np.isnan(out).sum()
        assert len(out) in (257, 513, 1025, 2000, 1999, 1700), name
        if name.startswith("alt."):
            assert 4 * finite >= len(out) and 4 * nan >= len(out), (name, finite, nan)
            if c["arg"] % 2 and c["arg"] > 21:
                assert len(set(out[np.isfinite(out)])) == finite, name       # distinct quotients: a shifted output shows
        elif c["fn"] == "stoch":
            assert 2 * finite > len(out), (name, finite)
        elif c["fn"] == "burst":
            assert 2 * finite > len(out) and np.isinf(out).any() and (out == 0).any() and (out < 0).any(), name
    zeros = np.concatenate([expected(k)[expected(k) == 0] for k in VALUE_CLASS_CASES if MANIFEST[k]["fn"] != "stoch"])
    assert np.signbit(zeros).sum() > 20 and (~np.signbit(zeros)).sum() > 20
    for k in ("signed.roc_p1", "signed.roc_p300", "signed.pct_p1"):
        assert np.isinf(expected(k)).any(), k


def test_vector_form_in_several_chunks(monkeypatch):
    monkeypatch.setattr(H, "CHUNK", 1000)
    for name in ("ties.burst_w50", "ties.burst_w1000", "walk.stoch_l14", "walk.stoch_l1000"):
        assert same(call(name, form="vector"), expected(name)), name


def test_documented_nan_rule_of_stoch_k():
    """A NaN in `low` or `high` gives NaN for every window that holds it, in both forms (the reference is path-dependent there)."""
    c, lo, hi = (np.array(a) for a in H.ohlc_walk(200, 41))
    lo[50], hi[120:124] = np.nan, np.nan
    for form in ("scalar", "vector"):
        out = H.stoch_k(c, lo, hi, 14, form=form)
        nan_at = set(np.nonzero(np.isnan(out[13:]))[0] + 13)
        assert nan_at >= set(range(50, 64)) | set(range(120, 137)) and len(nan_at) < 40
    assert same(H.stoch_k(c, lo, hi, 14, form="scalar"), H.stoch_k(c, lo, hi, 14, form="vector"))


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_raise_without_a_device(name):
    c = MANIFEST[name]
    for kw in ({"form": "scalar"}, {"form": "vector"}, {"mod": product()}):
        with pytest.raises(ValueError) as e:
            call(name, **kw)
        assert str(e.value) == c["message"]
    if c["fn"] == "burst":
        from finmlkit_amd.feature.core.ma import WINDOW_MESSAGE
        assert c["message"] == WINDOW_MESSAGE


def test_empty_series_need_no_device():
    P = product()
    e = np.empty(0)
    for mod, kw in ((H, {"form": "scalar"}), (H, {}), (P, {})):
        for r in (mod.comp_burst_ratio(e, 3, **kw), mod.stoch_k(e, e, e, 3, **kw), mod.roc(e, 3, **kw), mod.pct_change(e, 3, **kw)):
            assert r.dtype == np.float64 and r.shape == (0,)


def test_signatures_equal_the_references():
    P = product()
    assert list(inspect.signature(P.comp_burst_ratio).parameters) == ["series", "window"]
    assert list(inspect.signature(P.pct_change).parameters) == ["x", "periods"]
    assert list(inspect.signature(P.roc).parameters) == ["price", "period"]
    assert list(inspect.signature(P.stoch_k).parameters) == ["close", "low", "high", "length"]
    from finmlkit_amd.feature import transforms as T
    assert list(inspect.signature(T.BurstRatio.__init__).parameters) == ["self", "window", "input_col"]
    for cls, first in ((T.ROC, "periods"), (T.PctChange, "window")):
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters) == ["self", first, "input_col"] and sig.parameters["input_col"].default == "close"
    sig = inspect.signature(T.StochK.__init__)
    assert list(sig.parameters) == ["self", "length", "input_cols"]
    assert (sig.parameters["length"].default, sig.parameters["input_cols"].default) == (14, None)


def test_transform_names_and_defaults():
    from finmlkit_amd.feature.transforms import ROC, BurstRatio, Compose, MISOTransform, PctChange, StochK
    b, r, p, s = BurstRatio(50, "amount"), ROC(5), PctChange(3), StochK()
    assert (b.requires, b.produces, b.output_name) == (["amount"], ["burst50"], "amount_burst50")
    assert (r.requires, r.produces, r.periods, r.output_name) == (["close"], ["roc5"], 5, "close_roc5")
    assert (p.requires, p.produces, p.periods, p.output_name) == (["close"], ["pctc3"], 3, "close_pctc3")
    assert isinstance(s, MISOTransform) and (s.requires, s.produces, s.length, s.output_name) == (["high", "low", "close"], ["stochk14"], 14, "stochk14")
    assert StochK(5, ["h", "l", "c"]).requires == ["h", "l", "c"]
    assert Compose(PctChange(3, "amount"), BurstRatio(50, "pctc3")).output_name == "amount_pctc3_burst50"
    import pandas as pd
    with pytest.raises(ValueError, match="not found"):
        s(pd.DataFrame({"high": [1.0], "low": [1.0]}))
    with pytest.raises(TypeError):
        s(np.zeros(3))


def test_device_trades_methods_check_before_the_device():
    from finmlkit_amd import engine
    t = engine.DeviceTrades.__new__(engine.DeviceTrades)               # no context: the checks come first
    y = SimpleNamespace(dtype=np.dtype(np.float64), n=10)
    f32 = SimpleNamespace(dtype=np.dtype(np.float32), n=10)
    short = SimpleNamespace(dtype=np.dtype(np.float64), n=9)
    with pytest.raises(ValueError, match=r"^window must be at least 1\.$"):
        t.burst_ratio(y, 0)
    with pytest.raises(ValueError, match=r"^roc: period must not be negative\.$"):
        t.roc(y, -1)
    with pytest.raises(ValueError, match=r"^pct_change: periods must not be negative\.$"):
        t.pct_change(y, -1)
    with pytest.raises(ValueError, match=r"^stoch_k: length must be at least 1\.$"):
        t.stoch_k(y, y, y, 0)
    with pytest.raises(ValueError, match="same length"):
        t.stoch_k(y, short, y, 3)
    for fn in (lambda: t.burst_ratio(f32, 3), lambda: t.roc(f32, 3), lambda: t.pct_change(f32, 3), lambda: t.stoch_k(y, f32, y, 3)):
        with pytest.raises(TypeError, match="float64"):
            fn()


def test_library_exports_and_header_declares_the_entries():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "fmk.h")).read()
    for s in ENTRIES:
        for name in (s, s + "_dev"):
            assert hasattr(lib, name), name
            assert re.search(r"^int %s\(fmk_ctx \*ctx, " % name, header, re.M), name
