"""CPU-only: the running-sum indicators (bollinger_percent_b, vwap_distance, comp_flow_acceleration, vpin, parkinson_range).  The
plain restatement (tests/_runsum_ref.py) against the reference's recorded outputs (tests/golden/runsum.npz, written by
tools/gen_runsum_golden.py from the reference), the regenerated series against their recorded hashes, the argument checks of the host
layer, which need no device, the signatures and transform names, the library's symbols, and the share of flat Bollinger windows in
the recorded inputs.  Every comparison is bit for bit, NaN positions and the sign of every zero included: the restatement is
sequential.  Cases of more than 2100 elements record the hash of the reference's output instead of the output: the restatement is
held against the hash at full size (expected())."""
import inspect
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _runsum_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "runsum.json")))
_NPZ = np.load(os.path.join(GOLD, "runsum.npz"))

OK_CASES = sorted(k for k, v in MANIFEST.items() if "raises" not in v)
REFUSED = sorted(k for k, v in MANIFEST.items() if "raises" in v)
_HASHED = {}
ENTRIES = ("fmk_bollinger_percent_b", "fmk_vwap_distance", "fmk_flow_acceleration", "fmk_vpin", "fmk_parkinson_range")
EXACT_GENERATORS = {"grid64_walk", "int_volumes"}      # exactly summable: the order of addition cannot matter
FLAT_SHARE = 0.02
ZERO_SHARE = 0.01                      # all-zero vwap windows of volumes that are not exactly summable: at most this share of a case
TILE = 2048                            # elements per workgroup of the scan (csrc/fmk_recur_core.h: RC_TILE)
# zero-volume runs in a thread's first elements, up to and over the first tile edge, inside a tile, over the second edge, to the third
MANY = [[3, 30], [TILE - 21, 21], [TILE + 500, 19], [2 * TILE - 1, 22], [3 * TILE - 10, 60]]
FLOW_ARGS = ((1, 0), (2, 1), (3, 0), (20, 1), (20, 5), (100, 99))


def product():
    """The package's five functions under the reference's names."""
    from finmlkit_amd.feature.core.reversion import vwap_distance
    from finmlkit_amd.feature.core.volatility import bollinger_percent_b, parkinson_range
    from finmlkit_amd.feature.core.volume import comp_flow_acceleration, vpin
    return SimpleNamespace(bollinger_percent_b=bollinger_percent_b, parkinson_range=parkinson_range, vwap_distance=vwap_distance,
                           comp_flow_acceleration=comp_flow_acceleration, vpin=vpin)


def case_input(name):
    """The inputs of a fixture case as a tuple of series: stored, or regenerated from the case's seeds."""
    c = MANIFEST[name]
    src = c.get("source")
    if src is None:
        return tuple(_NPZ[f"{name}.in{k}"] for k in range(H.N_INPUTS[c["fn"]]))
    return H.generate(src)


def exactly_summable(name):
    """Whether every input of the case comes from a generator whose sums are exact in any order."""
    src = MANIFEST[name].get("source")
    return src is not None and all(g in EXACT_GENERATORS for g, _ in src)


def expected(name):
    """The reference's recorded output, or, for a case that records its hash alone, the restatement after its hash has been found
    equal to the recorded one."""
    if name + ".out" in _NPZ.files:
        return _NPZ[name + ".out"]
    if name not in _HASHED:
        c = MANIFEST[name]
        out = H.call(c["fn"], case_input(name), c["args"])
        assert str(out.dtype) == c["dtype"]
        assert H.sha256(H.nan_canonical(out.astype(np.float64))) == c["output_sha256"], name
        out.setflags(write=False)
        _HASHED[name] = out
    return _HASHED[name]


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True) and \
        np.array_equal(np.signbit(got) | np.isnan(got), np.signbit(want) | np.isnan(want))


def test_fixture_holds_what_it_should():
    assert {c["fn"] for c in MANIFEST.values()} == set(H.N_INPUTS)
    for key in ("walk.boll_cent_w", "walk.boll_g64_w", "walk.boll_hlc_w", "walk.vwap_lot_log_w", "walk.vwap_lot_simple_w",
                "walk.vwap_exact_log_w", "walk.vwap_exact_simple_w", "walk.vpin_lot_w", "walk.vpin_int_w"):
        assert {MANIFEST[k]["args"][0] for k in OK_CASES if k.startswith(key)} == {1, 2, 3, 20, 100}, key
    for key in ("walk.flow_lot_w", "walk.flow_int_w"):
        got = {tuple(MANIFEST[k]["args"]) for k in OK_CASES if k.startswith(key)}
        assert got == {(1, 0), (2, 0), (2, 1), (3, 0), (3, 2), (20, 0), (20, 5), (20, 19), (100, 0), (100, 5), (100, 99)}, key
    assert len(REFUSED) == 7 and len(OK_CASES) > 120
    assert all(MANIFEST[k]["dtype"] == ("float32" if MANIFEST[k]["fn"] == "vpin" else "float64") for k in OK_CASES)
    # window 1 of Bollinger: NaN everywhere; a NaN price: NaN from there on
    assert all(MANIFEST[f"walk.boll_{g}_w1"]["finite"] == 0 for g in ("cent", "g64", "hlc"))
    out = expected("nan.boll_after_w20")
    assert np.isnan(out[:19]).all() and np.isfinite(out[19:300]).all() and np.isnan(out[300:]).all()
    assert MANIFEST["nan.boll_first_w20"]["finite"] == 0
    # vwap: a NaN volume holds for good; zero runs hold only when they cover a window; over the first window: NaN until the first
    # window with volume; the first window is the simple form in log mode too
    out, c = expected("nan.vwap_volume_after_w20"), MANIFEST["nan.vwap_volume_after_w20"]
    assert c["held"] == 300 and np.isfinite(out[19:]).all() and (out[300:] == out[299]).all()
    assert MANIFEST["nan.vwap_volume_first_w20"]["finite"] == 0 and MANIFEST["nan.vwap_volume_first_w20"]["held"] == 581
    assert MANIFEST["zeros.vwap_short_w20"]["held"] == 0 and MANIFEST["zeros.vwap_exact_w20"]["held"] > 0
    assert MANIFEST["zeros.vwap_long_w20"]["held"] == (75 - 19) + (21 - 19) + 1
    out = expected("zeros.vwap_first_w20")
    assert np.isnan(out[:33]).all() and np.isfinite(out[33:]).all() and MANIFEST["zeros.vwap_first_w20"]["held"] == 14
    assert MANIFEST["zeros.vwap_all_w3"]["finite"] == 0
    a, b = expected("walk.vwap_lot_log_w20"), expected("walk.vwap_lot_simple_w20")
    assert a[19] == b[19] and (a[20:] != b[20:]).all()
    assert MANIFEST["long.vwap_exact_log_w20"]["held"] == (100 - 19) + (30 - 19)
    # flow: recent_periods 0 is valid; recent_periods >= window and window 0 give NaN everywhere
    assert MANIFEST["walk.flow_lot_w20_r0"]["finite"] == 581
    assert MANIFEST["walk.flow_recent_is_window"]["finite"] == MANIFEST["walk.flow_window0"]["finite"] == 0
    # vpin: NaN while a NaN bar is in the window, and where the window holds no volume
    out = expected("nan.vpin_buy_after_w20")
    assert np.isnan(out[300:320]).all() and np.isfinite(out[320:]).all() and np.isfinite(out[19:300]).all()
    assert MANIFEST["zeros.vpin_w20"]["nan"] == 19 + 21 and MANIFEST["window0.vpin"]["nan"] == 40
    # zero bars among volumes that are not exactly summable: flow has a number at every window, vpin NaN on the 41 all-zero ones
    assert MANIFEST["zerolot.flow_w20_r1"]["nan"] == MANIFEST["zerolot.flow_w20_r5"]["nan"] == 19
    assert MANIFEST["zerolot.vpin_kilo_w20"]["nan"] == 19 + 41 and MANIFEST["zerolot.vwap_log_w20"]["zero_windows"] == 42
    assert not any(exactly_summable(k) for k in OK_CASES if k.startswith("zerolot."))
    # a NaN in element 5 in front of them: NaN from there on, the windows of zero bars included
    assert MANIFEST["zerolot.flow_nan_w1_r0"]["nan"] == 2100 - 5 and np.isnan(expected("zerolot.flow_nan_w1_r0")[5:]).all()
    assert MANIFEST["zerolot.flow_nan_w20_r1"]["finite"] == MANIFEST["zerolot.flow_nan_w20_r5"]["finite"] == 0
    # parkinson: inf at a zero low and at a zero high, NaN at a negative ratio and at 0 / 0
    out = expected("edge.park")
    assert np.isinf(out[3]) and np.isnan(out[4]) and np.isinf(out[5]) and np.isnan(out[6]) and np.isfinite(out[7:]).all()
    for n, finite in ((0, 0), (1, 0), (9, 0), (10, 1), (11, 2)):
        for fn in ("boll", "vwap", "flow", "vpin"):
            c = MANIFEST[f"length.n{n}.{fn}"]
            assert (c["n"], c["finite"], c["nan"]) == (n, finite, n - finite), (n, fn)
        assert MANIFEST[f"length.n{n}.park"]["finite"] == n
    assert os.path.getsize(os.path.join(GOLD, "runsum.npz")) + os.path.getsize(os.path.join(GOLD, "runsum.json")) < 1_000_000


def test_flat_bollinger_windows_are_rare_in_the_recorded_inputs():
    """A window of equal prices has a true variance of zero: on prices that are not exactly summable the reference's NaN-or-number
    there is rounding noise, and the device test leaves such windows out.  They must stay a small share of what is compared."""
    seen = 0
    for name in OK_CASES:
        c = MANIFEST[name]
        if c["fn"] != "boll" or c["args"][0] < 2 or exactly_summable(name):
            continue
        flat = H.flat_windows(case_input(name)[0], c["args"][0])
        assert int(flat.sum()) == c["flat"]
        outputs = max(c["n"] - (c["args"][0] - 1), 1)
        assert flat.sum() <= FLAT_SHARE * outputs, (name, int(flat.sum()), outputs)
        seen += 1
    assert seen >= 10
    assert MANIFEST["walk.boll_held_w3"]["flat"] > 100 and exactly_summable("walk.boll_held_w3")


def test_inputs_stay_inside_the_contract():
    for name in OK_CASES:
        assert not any(np.isinf(a).any() for a in case_input(name)), name


def test_exactly_summable_generators_are_exact():
    """Prices on the 1/64 grid and integer volumes: every product, square and sum of the functions is an integer multiple of 2^-12
    far below 2^53 of them."""
    c, v = H.grid64_walk(6444, 872), H.int_volumes(6444, 873, [[700, 100]])
    assert (c * 64 == np.round(c * 64)).all() and (v == np.round(v)).all() and v.max() < 64 and (v[700:800] == 0).all()
    assert float(np.sum(c * c * 4096.0)) < 2.0 ** 52 and c.max() < 1024


def test_zero_lot_volumes_are_what_the_device_tests_take_them_for():
    v = H.zero_lot_volumes(6444, 818, MANY)
    plain = H.zero_lot_volumes(6444, 818, share=0)
    assert np.array_equal(plain, H.lot_volumes(6444, 818) + 1.0) and plain.min() >= 1.01 and plain.max() <= 51.0
    assert ((v == 0.0) | (v == plain)).all() and 0.28 < (v == 0.0).mean() < 0.33
    assert all((v[s:s + m] == 0.0).all() for s, m in MANY)
    assert not (plain * 64 == np.round(plain * 64)).all()                          # not exactly summable
    assert np.array_equal(H.zero_lot_kilo(6444, 818, MANY), v * 1024.0)
    z = H.zero_windows(v, 20)
    assert not z[:19].any() and z[22:33].all() and not z[21] and not z[33]         # the run [3, 33)
    assert np.array_equal(z, np.array([i >= 19 and (v[i - 19:i + 1] == 0.0).all() for i in range(len(v))]))
    assert not H.zero_windows(v, 7000).any() and np.array_equal(H.zero_windows(v, 1), v == 0.0)


def test_flow_over_zero_volume_bars_has_exactly_zero_sums_in_the_restatement():
    """Adding 0.0 leaves a prefix sum as it is, bit for bit: the recent sum of a window whose recent bars are all zero is exactly
    0.0, whatever the total in front of it, and the output is log((0.0 + EPS) / (past + EPS)), never the NaN of a negative sum.
    The device tests ask the kernels for the same on volumes whose prefix sums depend on the order of addition."""
    v = H.zero_lot_volumes(6444, 818, MANY)
    s = [0.0]
    for x in v.tolist():
        s.append(s[-1] + x)
    for w, r in FLOW_ARGS:
        out = H.comp_flow_acceleration(v, w, r)
        at = np.nonzero(H.zero_windows(v, r)[w - 1:] if r else np.ones(len(v) - (w - 1), bool))[0] + (w - 1)
        want = np.array([H._log(H._div(0.0 + H.EPS, (s[i + 1 - r] - s[i + 1 - w]) + H.EPS)) for i in at])
        assert same_bits(out[at], want), (w, r)
        assert not np.isnan(out[w - 1:]).any(), (w, r)
        if (w, r) == (20, 1):
            assert len(at) >= 1600                                                 # (2014 here)
        # the past part too: all zero -> exactly 0.0 -> log((recent + EPS) / EPS)
        past = np.nonzero(H.zero_windows(v, w - r)[w - 1 - r:len(v) - r])[0] + (w - 1)
        want = np.array([H._log(H._div((s[i + 1] - s[i + 1 - r]) + H.EPS, 0.0 + H.EPS)) for i in past])
        assert same_bits(out[past], want) and (len(past) > 0 or w - r > 30), (w, r)


def flow_windows_of_zero_bars(v, w, r):
    """Where both parts of the flow window that ends at i, the recent r bars and the w - r in front of them, hold zeros only."""
    v = np.asarray(v, np.float64)
    both = np.zeros(len(v), bool)
    both[w - 1:] = H.zero_windows(v, w)[w - 1:] if w else False
    return both


def test_flow_behind_a_nan_is_nan_on_windows_of_zero_bars_too():
    """A NaN volume makes every later prefix sum NaN, and NaN - NaN is NaN: behind it the restatement has NaN at every output, also
    where the whole window is zero bars and both of its sums would be exactly 0.0 (log(EPS / EPS) = 0.0) without the NaN in front."""
    for at in (5, TILE - 1, TILE):
        v = H.zero_lot_volumes(6444, 802, MANY)
        clean = v.copy()
        v[at] = np.nan
        for (w, r), least in (((1, 0), 1000), ((20, 1), 40), ((20, 5), 40)):
            out, before = H.comp_flow_acceleration(v, w, r), H.comp_flow_acceleration(clean, w, r)
            first = max(at, w - 1)
            assert np.isnan(out[first:]).all() and same_bits(out[:at], before[:at]) and np.isfinite(out[w - 1:at]).all(), (at, w, r)
            zero = flow_windows_of_zero_bars(v, w, r)
            zero[:first] = False
            assert zero.sum() >= least and (before[zero] == 0.0).all(), (at, w, r, int(zero.sum()))


def test_vpin_over_zero_volume_bars_is_nan_in_the_restatement():
    """A window in which both series are zero throughout has a total of exactly 0.0, which is not above 1e-9: NaN.  Elsewhere the
    total is at least 1.01 x 1024."""
    for share, windows in ((0, (1, 2, 20)), (0.3, (1,))):
        b, s = H.zero_lot_kilo(6444, 802, MANY, share), H.zero_lot_kilo(6444, 803, MANY, share)
        for w in windows:
            out = H.vpin(b, s, w)
            zero = H.zero_windows(b, w) & H.zero_windows(s, w)
            assert zero.sum() >= 50 and np.isnan(out[zero]).all(), (share, w)
            assert np.isfinite(out[w - 1:][~zero[w - 1:]]).all() and np.isnan(out[:w - 1]).all(), (share, w)
    # one bar with equal sides, neither zero: |buy - sell| adds 0.0 and the window-1 output there is exactly 0.0
    assert b[6208] == s[6208] != 0.0 and out[6208] == 0.0 and 6208 % 8 == 0


def test_vwap_on_all_zero_windows_is_the_references_own_residue():
    """On volumes that are not exactly summable the sliding vsum of an all-zero window is what the earlier additions and
    subtractions left behind, of either sign: the reference holds, computes a number of order 1 or takes the log of a negative
    number there, by chance.  The device tests leave those outputs out; off them every output from the seed on is finite."""
    c, w = H.grid_walk(6444, 801), 20
    seen = set()
    for runs in ([[TILE - 40, 40]], [[TILE - 30, 60]], [[TILE, 40]], [[2 * TILE - 30, 60]], MANY):
        v = H.zero_lot_volumes(6444, 802, runs)
        zero = H.zero_windows(v, w)
        assert 0 < zero.sum() <= ZERO_SHARE * (len(v) - (w - 1))
        for lg in (False, True):
            out, held = H.vwap_distance(c, v, w, lg, sums=True)
            assert np.isfinite(out[w - 1:][~zero[w - 1:]]).all() and not held[~zero].any()
            seen |= {"held"} if held[zero].any() else set()
            seen |= {"computed"} if np.isfinite(out[zero & ~held]).any() else set()
            seen |= {"nan"} if np.isnan(out[zero]).any() else set()
            seen |= {"near 2"} if (np.abs(out[zero & ~held]) > 1.5).any() else set()
    assert seen == {"held", "computed", "nan", "near 2"}


def test_regenerated_series_hash_to_the_recorded_ones():
    seen = 0
    for name, c in MANIFEST.items():
        if "source" in c:
            ins = case_input(name)
            assert [H.sha256(a) for a in ins] == c["input_sha256"], name
            assert all(len(a) == c["n"] for a in ins)
            seen += 1
    assert seen > 80


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
        assert str(e.value) == c["message"]
    assert c["message"] in (H.BOLLINGER_MESSAGE, H.VWAP_MESSAGE, H.FLOW_MESSAGE, H.VPIN_MESSAGE, H.VWAP_SHAPE_MESSAGE,
                            H.VPIN_SHAPE_MESSAGE, H.PARKINSON_MESSAGE)


def test_the_messages_are_the_contracts():
    assert H.BOLLINGER_MESSAGE == "bollinger_percent_b: window must be at least 1."
    assert H.VWAP_MESSAGE == "vwap_distance: n_periods must be at least 1."
    assert H.FLOW_MESSAGE == "comp_flow_acceleration: recent_periods must not be negative."
    assert H.VPIN_MESSAGE == "vpin: window must not be negative."
    assert {MANIFEST[k]["message"] for k in REFUSED if "unequal" not in k} == {H.BOLLINGER_MESSAGE, H.VWAP_MESSAGE, H.FLOW_MESSAGE,
                                                                              H.VPIN_MESSAGE}


def test_empty_series_need_no_device():
    P = product()
    e = np.empty(0)
    for mod in (H, P):
        for r, dtype in ((mod.bollinger_percent_b(e, 3, 2.0), np.float64), (mod.vwap_distance(e, e, 3, True), np.float64),
                         (mod.comp_flow_acceleration(e, 3, 1), np.float64), (mod.vpin(e, e, 3), np.float32),
                         (mod.parkinson_range(e, e), np.float64)):
            assert r.dtype == dtype and r.shape == (0,)


def test_signatures_equal_the_references():
    P = product()
    assert list(inspect.signature(P.bollinger_percent_b).parameters) == ["close", "window", "num_std"]
    assert list(inspect.signature(P.parkinson_range).parameters) == ["high", "low"]
    assert list(inspect.signature(P.vwap_distance).parameters) == ["close", "volume", "n_periods", "is_log"]
    assert list(inspect.signature(P.comp_flow_acceleration).parameters) == ["volumes", "window", "recent_periods"]
    assert list(inspect.signature(P.vpin).parameters) == ["volume_buy", "volume_sell", "window"]
    assert all(p.default is inspect.Parameter.empty for f in vars(P).values() for p in inspect.signature(f).parameters.values())
    from finmlkit_amd.feature import transforms as T
    sig = inspect.signature(T.BollingerPercentB.__init__)
    assert list(sig.parameters) == ["self", "window", "num_std", "input_col"]
    assert (sig.parameters["num_std"].default, sig.parameters["input_col"].default) == (2.0, "close")
    sig = inspect.signature(T.VWAPDistance.__init__)
    assert list(sig.parameters) == ["self", "periods", "is_log", "input_cols"]
    assert (sig.parameters["is_log"].default, sig.parameters["input_cols"].default) == (False, None)
    sig = inspect.signature(T.ParkinsonRange.__init__)
    assert list(sig.parameters) == ["self", "input_cols"] and sig.parameters["input_cols"].default is None
    sig = inspect.signature(T.FlowAcceleration.__init__)
    assert list(sig.parameters) == ["self", "window", "recent_periods", "input_col"]
    assert sig.parameters["input_col"].default == "volume" and sig.parameters["recent_periods"].default is inspect.Parameter.empty
    sig = inspect.signature(T.VPIN.__init__)
    assert list(sig.parameters) == ["self", "window", "input_cols"]
    assert (sig.parameters["window"].default, sig.parameters["input_cols"].default) == (32, None)


def test_transform_names_and_defaults():
    import pandas as pd

    from finmlkit_amd.feature.transforms import (SMA, BollingerPercentB, Compose, FlowAcceleration, MISOTransform, ParkinsonRange,
                                                 SISOTransform, VPIN, VWAPDistance)
    b = BollingerPercentB(20)
    assert isinstance(b, SISOTransform) and (b.requires, b.produces, b.window, b.num_std, b.output_name) == \
        (["close"], ["bollb20"], 20, 2.0, "close_bollb20")
    f = FlowAcceleration(20, 5)
    assert isinstance(f, SISOTransform) and (f.requires, f.produces, f.output_name) == (["volume"], ["flowacc_20_5"], "volume_flowacc_20_5")
    v = VWAPDistance(12)
    assert isinstance(v, MISOTransform) and (v.requires, v.produces, v.periods, v.is_log, v.output_name) == \
        (["close", "volume"], ["vwapd12"], 12, False, "vwapd12")
    p = ParkinsonRange()
    assert isinstance(p, MISOTransform) and (p.requires, p.produces, p.output_name) == (["high", "low"], ["parkrange"], "parkrange")
    q = VPIN()
    assert isinstance(q, MISOTransform) and (q.requires, q.produces, q.window, q.output_name) == \
        (["volume_buy", "volume_sell"], ["vpin_32"], 32, "vpin_32")
    assert VPIN(8, ["b", "s"]).requires == ["b", "s"] and VWAPDistance(3, True, ["c", "v"]).requires == ["c", "v"]
    assert Compose(SMA(5, "close"), BollingerPercentB(20, 2.0, "sma5")).output_name == "close_sma5_bollb20"
    with pytest.raises(ValueError, match="not found"):
        v(pd.DataFrame({"close": [1.0]}))
    with pytest.raises(TypeError):
        p(np.zeros(3))
    # the transforms refuse their arguments before a device is needed
    frame = pd.DataFrame({"close": [2.0, 3.0], "volume": [1.0, 2.0], "volume_buy": [1.0, 1.0], "volume_sell": [0.0, 1.0]})
    for t, message in ((BollingerPercentB(0), "bollinger_percent_b: window"), (VWAPDistance(0), "vwap_distance: n_periods"),
                       (FlowAcceleration(5, -1), "comp_flow_acceleration: recent_periods"), (VPIN(-1), "vpin: window")):
        for backend in ("nb", "pd"):
            with pytest.raises(ValueError, match=message):
                t(frame, backend=backend)
    ts = SimpleNamespace(ctx=None)
    for t, message in ((BollingerPercentB(0), "bollinger_percent_b: window"), (FlowAcceleration(5, -1), "recent_periods")):
        with pytest.raises(ValueError, match=message):
            t._dev(ts, SimpleNamespace(n=2))


def test_device_trades_methods_check_before_the_device():
    from finmlkit_amd import engine
    t = engine.DeviceTrades.__new__(engine.DeviceTrades)               # no context: the checks come first
    y = SimpleNamespace(dtype=np.dtype(np.float64), n=10)
    f32 = SimpleNamespace(dtype=np.dtype(np.float32), n=10)
    short = SimpleNamespace(dtype=np.dtype(np.float64), n=9)
    with pytest.raises(ValueError, match=r"^bollinger_percent_b: window must be at least 1\.$"):
        t.bollinger_percent_b(y, 0)
    with pytest.raises(ValueError, match=r"^vwap_distance: n_periods must be at least 1\.$"):
        t.vwap_distance(y, y, 0)
    with pytest.raises(ValueError, match=r"^comp_flow_acceleration: recent_periods must not be negative\.$"):
        t.flow_acceleration(y, 5, -1)
    with pytest.raises(ValueError, match=r"^vpin: window must not be negative\.$"):
        t.vpin(y, y, -1)
    for fn in (lambda: t.vwap_distance(y, short, 3), lambda: t.parkinson_range(short, y), lambda: t.vpin(y, short, 3)):
        with pytest.raises(ValueError, match="same length"):
            fn()
    for fn in (lambda: t.bollinger_percent_b(f32, 3), lambda: t.vwap_distance(y, f32, 3), lambda: t.parkinson_range(f32, y),
               lambda: t.flow_acceleration(f32, 3, 1), lambda: t.vpin(f32, y, 3)):
        with pytest.raises(TypeError, match="float64"):
            fn()
    sig = inspect.signature(engine.DeviceTrades.bollinger_percent_b)
    assert list(sig.parameters) == ["self", "y", "window", "num_std"] and sig.parameters["num_std"].default == 2.0
    sig = inspect.signature(engine.DeviceTrades.vwap_distance)
    assert list(sig.parameters) == ["self", "close", "volume", "n_periods", "is_log"] and sig.parameters["is_log"].default is False


def test_library_exports_and_header_declares_the_entries():
    from finmlkit_amd import _ffi
    lib = _ffi.lib()
    header = open(os.path.join(ROOT, "include", "fmk.h")).read()
    for s in ENTRIES:
        for name in (s, s + "_dev"):
            assert hasattr(lib, name), name
            assert re.search(r"^int %s\(fmk_ctx \*ctx, " % name, header, re.M), name
    assert lib.fmk_abi_version() == 1
