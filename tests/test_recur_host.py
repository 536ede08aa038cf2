"""CPU-only: the recursive indicators (ewma, rsi_wilder, true_range, atr, adx_core).  The plain restatement (tests/_recur_ref.py)
against the reference's recorded outputs (tests/golden/recur.npz, written by tools/gen_recur_golden.py from the untouched
reference), the regenerated series against their recorded hashes, the argument checks of the host layer, which need no device, the
signatures and transform names, and the library's symbols.  Every comparison is bit for bit, NaN positions and the sign of every zero
included: the restatement is sequential.  Cases of more than 2100 elements record the hash of the reference's output instead of the
output: the restatement is held against the hash at full size (expected()).

The cases runs.* (runs without a loss, a gain, a range or a term, where the state carried from element to element is all there is;
memories of several tiles) are no part of OK_CASES: past the step at which a decaying state leaves the normal range the kernels are
not held to the reference, so they have tests of their own, here and in tests/test_gpu_recur_runs.py.  Here: the
restatement against the recorded hash, the long-double evaluation (index ranges to compare, elements left out, the restatement's own
deviation) against the record, and what the reference really does past that step."""
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

RUN_CASES = sorted(k for k in MANIFEST if k.startswith("runs."))
OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v and not k.startswith("runs."))
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)
GENERATORS = {"grid_walk": lambda *a: (H.grid_walk(*a),), "hlc_walk": H.hlc_walk,
              "run_close": lambda *a: (H.run_series(*a)[2],), "run_hlc": H.run_series}
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


# ---------------------------------------------------------------------------------------------- runs.*
TILE = 2048


def run_of(name):
    """(start, length) of the run of a case runs.b.* / runs.c.*."""
    kind, n, _, start, length = MANIFEST[name]["source"]["args"][:5]
    assert start + length + 1500 == n == MANIFEST[name]["n"]
    return start, length


def test_horizon_figures():
    assert [H.horizon((w - 1) / w) for w in (2, 3, 5, 14)] == [969, 1657, 3010, 9063]
    assert H.horizon(1 - 2 / (27 + 1)) == H.horizon(13 / 14)          # ewma's span 2 w - 1 has the a of window w
    for w in (2, 3, 5, 14):                                           # a state from 1.0 is still 2^-969 there, and within two steps below
        a = (w - 1) / w
        assert a ** (H.horizon(a) - 1) >= 2.0 ** -969 > a ** (H.horizon(a) + 1)


def test_run_series_kinds():
    n, start, length = 700, 200, 300
    run = slice(start, start + length)
    plain = H.run_series("flat", n, 5, start, 0)
    for kind in ("flat", "rising", "falling", "zeros"):
        h, lo, c = H.run_series(kind, n, 5, start, length)
        again = H.run_series(kind, n, 5, start, length)
        assert all(same_bits(a, b) for a, b in zip((h, lo, c), again))
        assert all(same_bits(a[:start], b[:start]) for a, b in zip((h, lo, c), plain))       # the walk in front of the run
        assert (h >= c).all() and (c >= lo).all() and np.isfinite(h).all()
        d = np.diff(c)[start - 1:start + length - 1]                   # the moves of the run's bars
        if kind == "zeros":
            assert (c[run] == 0).all() and (h[run] == 0).all() and (lo[run] == 0).all() and c[start + length] > 50
            continue
        assert {"flat": (d == 0).all(), "rising": (d >= 0).all() and (d == 0).any() and (d > 0).any(),
                "falling": (d <= 0).all() and (d == 0).any() and (d < 0).any()}[kind]
        assert ((h[run] == lo[run]).all() and (h[run] == c[run]).all()) == (kind == "flat")
        tr = H.true_range(h, lo, c)
        assert ((tr[run] == 0).all()) == (kind == "flat") and (tr[:start] > 0).sum() > start * 0.9
        assert np.abs(np.diff(c)[start + length:]).max() > 0.02        # the walk goes on from the held level
        assert abs(c[start + length] - c[start + length - 1]) <= 0.35 + 1e-9
    h, lo, c = H.run_series("from_start", n, 6, 0, 50)
    assert (c[:50] == c[0]).all() and (h[:50] == lo[:50]).all() and len(set(c[49:60])) > 3
    assert H.run_series("rising", n, 6, 0, 50, after=-7)[2][50] == pytest.approx(H.run_series("rising", n, 6, 0, 50)[2][49] - 0.07)
    with pytest.raises(ValueError):
        H.run_series("from_start", n, 6, 1, 50)
    with pytest.raises(ValueError):
        H.run_series("flat", n, 6, 600, 101)
    with pytest.raises(ValueError):
        H.run_series("level", n, 6, 0, 50)


def test_runs_hold_the_cases_they_should():
    names = set(RUN_CASES)
    b = {k for k in names if k.startswith("runs.b.")}
    assert len(b) == 96 and all(MANIFEST[k]["left_out"] == 0 for k in b)
    for w, lengths in ((2, (100, 870)), (3, (1490,)), (5, (TILE + 8, 2700)), (14, (TILE + 8, 2 * TILE + 100, 8156)), (100, (3 * TILE,))):
        for length in lengths:
            for tag in ("rsi_flat", "rsi_rising", "atr_ema", "atr_ema_norm", "adx", "ewma_zeros"):
                assert f"runs.b.{tag}.w{w}.s{TILE}.l{length}" in names
                assert (f"runs.b.{tag}.w{w}.s{TILE + 1003}.l{length}" in names) == (length != TILE + 8)
            if w > 2:
                assert length <= 0.9 * H.horizon((w - 1) / w) + 1
    c = {k for k in names if k.startswith("runs.c.")}
    assert len(c) == 14 and {MANIFEST[k]["fn"] for k in c} == {"rsi", "atr", "adx"}
    for k in c:
        w = MANIFEST[k]["args"][0]
        assert run_of(k)[1] == int(1.3 * math.log(2.0 ** -1074) / math.log((w - 1) / w)) > 1.3 * H.horizon((w - 1) / w)
        assert 0 < MANIFEST[k]["left_out"] < 0.35 * MANIFEST[k]["n"]
    e = {k: MANIFEST[k] for k in names if k.startswith("runs.e.")}
    assert sorted((v["fn"], v["args"][0]) for v in e.values()) == sorted(
        [("rsi", 3 * TILE + 1), ("rsi", 10 * TILE - 1), ("atr", 3 * TILE + 1), ("atr", 10 * TILE - 1), ("adx", 2 * TILE + 1), ("adx", 5 * TILE),
         ("ewma", 4097), ("ewma", 200_001)])
    assert all(v["left_out"] == 0 and v["n"] <= 22_600 for v in e.values()) and len(names) == len(b) + len(c) + len(e)
    # the tolerance the GPU tests derive from the record stays ten times and more below the contract's ceiling
    for k in names:
        ceiling = 1e-9 if MANIFEST[k]["fn"] in ("ewma", "atr") else 1e-7
        assert 0 < 16 * MANIFEST[k]["ref_dev"] * 10 <= ceiling, k


@pytest.mark.parametrize("name", RUN_CASES)
def test_run_case_record(name):
    """The restatement hashes to the reference's recorded output; index ranges, the count left out and the restatement's deviation
    come out of the long-double evaluation as recorded."""
    c, ins = MANIFEST[name], case_input(name)
    own = expected(name)
    assert "output_sha256" in c and len(own) == c["n"] > 2100
    states, exact = H.exact_states(c["fn"], ins, c["args"])
    assert states.dtype == np.longdouble and states.shape[1] == c["n"]
    mask = H.compare_mask(c["fn"], c["args"], states)
    assert H.mask_ranges(mask) == c["compare"] and int((~mask).sum()) == c["left_out"]
    assert np.array_equal(H.ranges_mask(c["compare"], c["n"]), mask)
    assert H.deviation(c["fn"], own, exact, mask) == c["ref_dev"]
    e64 = exact.astype(np.float64)
    assert np.array_equal(np.isnan(own)[mask], np.isnan(e64)[mask])
    floor = np.longdouble(2.0) ** -969
    live = np.abs(states[:, mask])
    assert ((live == 0) | (live >= floor)).all()
    if not name.startswith("runs.e."):
        start, length = run_of(name)
        if c["left_out"]:                                             # compared up to the horizon, and again behind the run
            (a0, a1), (b0, b1) = c["compare"]
            w = c["args"][0]
            assert a0 == 0 and b1 == c["n"] and start + 0.85 * H.horizon((w - 1) / w) < a1 < start + 1.1 * H.horizon((w - 1) / w)
            assert start + length <= b0 < start + length + 700


@pytest.mark.parametrize("name", [k for k in RUN_CASES if k.startswith("runs.c.")])
def test_past_the_horizon_the_reference_stalls(name):
    """What the reference does with a state far below 2^-969: for windows of 3 and more ((w - 1) * 5e-324) / w rounds back to
    5e-324, so an average that has nothing to add stays at the smallest subnormals for good and rsi_wilder reads 50.0 off two of
    them; at window 2 it halves to 0.0 and rsi_wilder is NaN until the next loss."""
    c = MANIFEST[name]
    fn, w = c["fn"], c["args"][0]
    tiny = 5e-324
    assert ((w - 1) * tiny) / w == (tiny if w >= 3 else 0.0)
    own = expected(name)
    start, length = run_of(name)
    tail = own[start + length - 200:start + length]                   # the last bars of the run
    left = ~H.ranges_mask(c["compare"], c["n"])
    assert left[start + length - 200:start + length].all()
    if fn == "rsi":
        assert np.isnan(tail).all() if w == 2 else (tail == 50.0).all()
        assert np.isfinite(own[start:start + H.horizon((w - 1) / w)]).all()
    elif fn == "atr":
        assert (tail == tail[0]).all() and 0 < tail[0] <= (w // 2 + 1) * tiny and ((w - 1) * tail[0] + 0.0) / w == tail[0]
    else:
        assert np.isfinite(own).all() and (own >= 0).all() and (own <= 100).all()


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
