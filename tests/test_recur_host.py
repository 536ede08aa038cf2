"""CPU-only: the recursive indicators (ewma, rsi_wilder, true_range, atr, adx_core).  The plain restatement (tests/_recur_ref.py)
against the reference's recorded outputs (tests/golden/recur.npz, written by tools/gen_recur_golden.py from the untouched
reference), the regenerated series against their recorded hashes, the argument checks of the host layer, which need no device, the
signatures and transform names, and the library's symbols.  Every comparison is bit for bit, NaN positions and the sign of every zero
included: the restatement is sequential.  Cases of more than 2100 elements record the hash of the reference's output instead of the
output: the restatement is held against the hash at full size (expected())."""
import inspect
import json
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _recur_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "recur.json")))
_NPZ = np.load(os.path.join(GOLD, "recur.npz"))

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)
GENERATORS = {"grid_walk": lambda *a: (H.grid_walk(*a),), "hlc_walk": H.hlc_walk}
N_INPUTS = {"ewma": 1, "rsi": 1, "tr": 3, "atr": 3, "adx": 3}
_HASHED = {}
ENTRIES = ("fmk_ewma", "fmk_rsi_wilder", "fmk_true_range", "fmk_atr", "fmk_adx")


def product():
    """The package's five functions under the reference's names."""
    from finmlkit_amd.feature.core.ma import ewma
    from finmlkit_amd.feature.core.momentum import rsi_wilder
    from finmlkit_amd.feature.core.trend import adx_core
    from finmlkit_amd.feature.core.volatility import atr, true_range
    return SimpleNamespace(ewma=ewma, rsi_wilder=rsi_wilder, true_range=true_range, atr=atr, adx_core=adx_core)


def case_input(name):
    """The inputs of a fixture case as a tuple of series: stored, or regenerated from the case's seed."""
    c = MANIFEST[name]
    src = c.get("source")
    if src is None:
        return tuple(_NPZ[f"{name}.in{k}"] for k in range(N_INPUTS[c["fn"]]))
    return tuple(GENERATORS[src["gen"]](*src["args"]))


def expected(name):
    """The reference's recorded output, or, for a case that records its hash alone, the restatement after its hash has been found
    equal to the recorded one."""
    if name + ".out" in _NPZ.files:
        return _NPZ[name + ".out"]
    if name not in _HASHED:
        c = MANIFEST[name]
        out = H.call(c["fn"], case_input(name), c["args"])
        assert H.sha256(H.nan_canonical(out)) == c["output_sha256"], name
        out.setflags(write=False)
        _HASHED[name] = out
    return _HASHED[name]


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True) and \
        np.array_equal(np.signbit(got) | np.isnan(got), np.signbit(want) | np.isnan(want))


def test_fixture_holds_what_it_should():
    assert {c["fn"] for c in MANIFEST.values()} == set(N_INPUTS)
    for fn, key in (("ewma", "walk.ewma_s"), ("rsi", "walk.rsi_w"), ("atr", "walk.atr_sma_w"), ("atr", "walk.atr_ema_w"), ("adx", "walk.adx_l")):
        assert {MANIFEST[k]["args"][0] for k in OK_CASES if k.startswith(key)} == {1, 2, 3, 14, 100}, key
    assert len(REFUSED) == 6 and len(OK_CASES) > 100
    # NaN rules: rsi all NaN with a NaN in the first window, finite around a later one; ewma and the EMA mode NaN for good
    assert MANIFEST["nan.rsi_seed_w14"]["finite"] == 0
    out = expected("nan.rsi_after_w14")
    assert np.isnan(out[:14]).all() and np.isfinite(out[14:]).all()
    out = expected("nan.ewma_s14")
    assert np.isfinite(out[:300]).all() and np.isnan(out[300:]).all()
    out = expected("nan.atr_ema_w14")
    assert np.isfinite(out[13:50]).all() and np.isnan(out[50:]).all()
    assert np.isfinite(expected("nan.atr_ema_seed_w14")[13:]).all()
    # the SMA mode: NaN runs shorter (3) and longer (40) than the window of 14
    out = expected("nan.atr_sma_w14")
    assert np.isfinite(out[13:150]).all() and np.isnan(out[150 + 13:190]).all() and np.isfinite(out[190:]).all()
    # the NaN at bar 2: only when all three prices of bar 2 are NaN, and only where bar 2 has an output
    assert np.isnan(expected("quirk.atr_sma_w3")[2]) and np.isfinite(expected("quirk.atr_sma_close_w3")[2])
    assert np.isnan(expected("quirk.atr_sma_w2")[2]) and np.isfinite(expected("quirk.atr_sma_w2")[4])
    # adx: all zeros with a NaN in the seed window; zeros before 2 L - 1; a later NaN makes dx 0.0, the ADX decays
    assert MANIFEST["nan.adx_seed_l14"]["zeros"] == 600
    out = expected("walk.adx_l14")
    assert (out[:27] == 0).all() and (out[27:] > 0).all()
    out = expected("nan.adx_after_l14")
    assert (out[27:] > 0).all() and np.isfinite(out).all()
    for n, first in ((0, None), (1, None), (19, None), (20, 19), (21, 19)):
        out = expected(f"length.n{n}.adx")
        assert len(out) == n and ((out == 0).all() if first is None else (out[first] > 0 and (out[:first] == 0).all()))
    for n, finite in ((1, 0), (9, 0), (10, 0), (11, 1), (20, 10)):
        assert MANIFEST[f"length.n{n}.rsi"]["finite"] + MANIFEST[f"length.n{n}.rsi"]["nan"] == n
        assert MANIFEST[f"length.n{n}.atr_sma"]["finite"] == MANIFEST[f"length.n{n}.atr_ema"]["finite"] == max(0, n - 9)
    assert MANIFEST["window0.atr_sma"]["nan"] == MANIFEST["window0.atr_ema"]["nan"] == 40
    assert os.path.getsize(os.path.join(GOLD, "recur.npz")) + os.path.getsize(os.path.join(GOLD, "recur.json")) < 1_000_000


def test_inputs_stay_inside_the_contract():
    """No infinities, and the longest run without a loss far below the steps after which a smoothed loss underflows."""
    for name in OK_CASES:
        c, ins = MANIFEST[name], case_input(name)
        assert not any(np.isinf(a).any() for a in ins), name
        if c["fn"] == "rsi" and c["args"][0] > 1:
            w = c["args"][0]
            assert H.longest_loss_free_run(ins[0]) * 20 < math.log(1e-300) / math.log((w - 1) / w), name


def test_regenerated_series_hash_to_the_recorded_ones():
    seen = 0
    for name, c in MANIFEST.items():
        if "source" in c:
            ins = case_input(name)
            assert [H.sha256(a) for a in ins] == c["input_sha256"], name
            assert all(len(a) == c["n"] for a in ins)
            seen += 1
    assert seen > 30


@pytest.mark.parametrize("name", OK_CASES)
def test_restatement_equals_the_reference(name):
    c = MANIFEST[name]
    assert same_bits(H.call(c["fn"], case_input(name), c["args"]), expected(name)), name


@pytest.mark.parametrize("name", REFUSED)
def test_refused_arguments_raise_without_a_device(name):
    c = MANIFEST[name]
    for mod in (None, product()):
        with pytest.raises(ValueError) as e:
            H.call(c["fn"], case_input(name), c["args"], mod=mod)
        if "unequal" not in name or mod is None:
            assert str(e.value) == c["message"]
    if c["fn"] == "ewma":                # the reference's own message
        assert c["message"] == "span size is less than or equal to 1. Please provide a span size greater than 1."
    if name == "refused.tr_unequal":
        assert c["message"] == "The length of high, low, and close prices must be the same."


def test_unequal_lengths_are_refused_by_the_package():
    P = product()
    a, b = np.ones(5), np.ones(4)
    for fn in (lambda: P.true_range(a, b, a), lambda: P.atr(a, a, b, 3), lambda: P.adx_core(b, a, a, 2)):
        with pytest.raises(ValueError, match="same"):
            fn()


def test_empty_series_need_no_device():
    P = product()
    e = np.empty(0)
    for mod in (H, P):
        for r in (mod.ewma(e, 3), mod.rsi_wilder(e, 3), mod.true_range(e, e, e), mod.atr(e, e, e, 3), mod.atr(e, e, e, 3, True, True),
                  mod.adx_core(e, e, e, 3)):
            assert r.dtype == np.float64 and r.shape == (0,)


def test_signatures_equal_the_references():
    P = product()
    assert list(inspect.signature(P.ewma).parameters) == ["y", "span"]
    assert list(inspect.signature(P.rsi_wilder).parameters) == ["close", "window"]
    assert list(inspect.signature(P.true_range).parameters) == ["high", "low", "close"]
    sig = inspect.signature(P.atr)
    assert list(sig.parameters) == ["high", "low", "close", "window", "ema_based", "normalize"]
    assert (sig.parameters["ema_based"].default, sig.parameters["normalize"].default) == (False, False)
    assert list(inspect.signature(P.adx_core).parameters) == ["high", "low", "close", "length"]
    from finmlkit_amd.feature.core import adx_core
    assert adx_core is P.adx_core
    from finmlkit_amd.feature import transforms as T
    sig = inspect.signature(T.EWMA.__init__)
    assert list(sig.parameters) == ["self", "span", "input_col"] and sig.parameters["input_col"].default is None
    sig = inspect.signature(T.RSIWilder.__init__)
    assert list(sig.parameters) == ["self", "window", "input_col"]
    assert (sig.parameters["window"].default, sig.parameters["input_col"].default) == (14, "close")
    sig = inspect.signature(T.ATR.__init__)
    assert list(sig.parameters) == ["self", "window", "ema_based", "normalize", "input_cols"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [14, False, False, None]
    sig = inspect.signature(T.ADX.__init__)
    assert list(sig.parameters) == ["self", "length", "input_cols"]
    assert (sig.parameters["length"].default, sig.parameters["input_cols"].default) == (14, None)


def test_transform_names_and_defaults():
    from finmlkit_amd.feature.transforms import ADX, ATR, EWMA, Compose, MISOTransform, PctChange, ReturnT, RSIWilder, SISOTransform
    e, r = EWMA(20, "close"), RSIWilder()
    assert isinstance(e, SISOTransform) and (e.requires, e.produces, e.span, e.output_name) == (["close"], ["ewma20"], 20, "close_ewma20")
    assert (r.requires, r.produces, r.window, r.output_name) == (["close"], ["rsiw14"], 14, "close_rsiw14")
    a = ATR()
    assert isinstance(a, MISOTransform) and (a.requires, a.produces, a.output_name) == (["high", "low", "close"], ["atr14"], "atr14")
    assert ATR(7, True).output_name == "atr7_ema" and ATR(7, False, True).output_name == "atr7_norm"
    assert ATR(7, True, True, ["h", "l", "c"]).output_name == "atr7_ema_norm" and ATR(7, input_cols=["h", "l", "c"]).requires == ["h", "l", "c"]
    d = ADX()
    assert isinstance(d, MISOTransform) and (d.requires, d.produces, d.length, d.output_name) == (["high", "low", "close"], ["adx_14"], 14, "adx_14")
    assert ADX(5, ["h", "l", "c"]).requires == ["h", "l", "c"]
    import pandas as pd
    assert Compose(ReturnT(pd.Timedelta(seconds=5), input_col="price"), EWMA(10, "ret5.0s")).output_name == "price_ret5.0s_ewma10"
    assert Compose(PctChange(3, "close"), RSIWilder(14, "pctc3")).output_name == "close_pctc3_rsiw14"
    with pytest.raises(ValueError, match="not found"):
        a(pd.DataFrame({"high": [1.0], "low": [1.0]}))
    with pytest.raises(TypeError):
        d(np.zeros(3))
    # the transforms refuse their arguments before a device is needed
    frame = pd.DataFrame({"high": [2.0, 3.0], "low": [1.0, 2.0], "close": [1.5, 2.5]})
    for t, message in ((EWMA(0, "close"), "span size"), (RSIWilder(0), "rsi_wilder: window"), (ATR(-1), "atr: window"),
                       (ADX(0), "adx_core: length")):
        with pytest.raises(ValueError, match=message):
            t(frame)
    ts = SimpleNamespace(ctx=None)
    for t, message in ((EWMA(0, "close"), "span size"), (RSIWilder(0), "rsi_wilder: window")):
        with pytest.raises(ValueError, match=message):
            t._dev(ts, SimpleNamespace(n=2))


def test_device_trades_methods_check_before_the_device():
    from finmlkit_amd import engine
    t = engine.DeviceTrades.__new__(engine.DeviceTrades)               # no context: the checks come first
    y = SimpleNamespace(dtype=np.dtype(np.float64), n=10)
    f32 = SimpleNamespace(dtype=np.dtype(np.float32), n=10)
    short = SimpleNamespace(dtype=np.dtype(np.float64), n=9)
    with pytest.raises(ValueError, match=r"^span size is less than or equal to 1\. Please provide a span size greater than 1\.$"):
        t.ewma(y, 0)
    with pytest.raises(ValueError, match=r"^rsi_wilder: window must be at least 1\.$"):
        t.rsi_wilder(y, 0)
    with pytest.raises(ValueError, match=r"^atr: window must not be negative\.$"):
        t.atr(y, y, y, -1)
    with pytest.raises(ValueError, match=r"^adx_core: length must be at least 1\.$"):
        t.adx(y, y, y, 0)
    for fn in (lambda: t.true_range(y, short, y), lambda: t.atr(y, y, short, 3), lambda: t.adx(short, y, y, 3)):
        with pytest.raises(ValueError, match="same"):
            fn()
    for fn in (lambda: t.ewma(f32, 3), lambda: t.rsi_wilder(f32, 3), lambda: t.true_range(y, f32, y), lambda: t.atr(f32, y, y, 3),
               lambda: t.adx(y, y, f32, 3)):
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
