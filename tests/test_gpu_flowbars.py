"""GPU: imbalance and run bars with a fixed threshold against the loops that define them (tests/_flowbars_ref.py).  Every case runs
under the library's own choice of rung and with FMK_FLOWBARS_SERIAL set; both answers equal the loops exactly (every output is an
index, so there is no tolerance), and the diagnostics say which rung answered and why the tables declined."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _flowbars_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 16 * 4096 + 1, (1 << 20) + 1)
# (rule, kind, threshold) of the size sweep
SWEEP = (("imbalance", "tick", 16.0), ("imbalance", "volume", 8.0), ("run", "tick", 16.0), ("run", "volume", 8.0),
         ("run", "volume", 64.0))


@functools.lru_cache(maxsize=None)
def want_recipe(rule, kind, thr, n, lots="dyadic"):
    w = R.closes(rule, kind, *R.recipe(n, lots), thr)
    w.setflags(write=False)
    return w


def device_trades(cols, f64=False):
    from finmlkit_amd.engine import DeviceTrades
    px, am, sd = cols
    am = np.asarray(am, np.float64) if f64 else am
    return DeviceTrades.from_numpy(np.arange(len(px), dtype=np.int64), px, am, sd)


def index(t, rule, kind, thr):
    from finmlkit_amd import _ffi
    got = (t.imbalance_bar_index if rule == "imbalance" else t.run_bar_index)(thr, kind=kind)
    assert got.dtype == np.int64
    return got.to_host(), _ffi.flow_bars_last()


def check_both(monkeypatch, t, rule, kind, thr, want, rung=0, code=0, ls=None):
    """The library's own choice (rung / code as given), then the forced serial walk: both equal `want`."""
    monkeypatch.delenv("FMK_FLOWBARS_SERIAL", raising=False)
    got, d = index(t, rule, kind, thr)
    print(f"{rule}/{kind} thr {thr} n {t.n}: {len(got)} indices, {d}")
    np.testing.assert_array_equal(got, want, err_msg=f"{rule}/{kind} thr {thr} own choice {d}")
    assert (d["rung"], d["code"]) == (rung, code), d
    if ls is not None:
        assert d["ls"] == ls, d
    monkeypatch.setenv("FMK_FLOWBARS_SERIAL", "1")
    got, d = index(t, rule, kind, thr)
    np.testing.assert_array_equal(got, want, err_msg=f"{rule}/{kind} thr {thr} serial")
    assert (d["rung"], d["code"]) == (1, 0), d
    monkeypatch.delenv("FMK_FLOWBARS_SERIAL")


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", SIZES)
def test_sizes(monkeypatch, n):
    t = device_trades(R.recipe(n))
    for rule, kind, thr in SWEEP:
        want = want_recipe(rule, kind, thr, n)
        check_both(monkeypatch, t, rule, kind, thr, want)
        if n == (1 << 20) + 1:
            assert len(want) > 1000                                                     # 257 blocks of S = 4096: a three-level tree


def test_milli_lots(monkeypatch):
    n = (1 << 20) + 1
    cols = R.recipe(n, "milli")
    predicted = 0 if R.certifies("imbalance", "volume", *cols, 5.0) else 1
    check_both(monkeypatch, device_trades(cols), "imbalance", "volume", 5.0, want_recipe("imbalance", "volume", 5.0, n, "milli"),
               rung=predicted, code=0 if predicted == 0 else 4)


@pytest.mark.parametrize("rule", ["imbalance", "run"])
def test_float64_amounts(monkeypatch, rule):
    n = 16 * 4096 + 1
    check_both(monkeypatch, device_trades(R.recipe(n), f64=True), rule, "volume", 8.0, want_recipe(rule, "volume", 8.0, n))


# ---------------------------------------------------------------------------------------------- long bars
@pytest.mark.parametrize("rule,thr", [("imbalance", 8.0), ("run", 64.0)])
@pytest.mark.parametrize("stretch,ls", [(5000, 13), (70000, 17)])
def test_ls_hand_offs(monkeypatch, rule, thr, stretch, ls):
    n = (1 << 17) + 1 - stretch
    at = n // 2
    cols = R.with_quiet_stretch(R.recipe(n), at, stretch)
    assert len(cols[0]) == (1 << 17) + 1
    want = R.shifted(want_recipe(rule, "volume", thr, n), at, stretch)                 # tests/test_flowbars_host.py: the identity
    check_both(monkeypatch, device_trades(cols), rule, "volume", thr, want, ls=ls)


@pytest.mark.parametrize("rule,thr", [("imbalance", 8.0), ("run", 64.0)])
def test_beyond_the_tables(monkeypatch, rule, thr):
    n, stretch, at = 4097, (1 << 22) + 8, 2000
    cols = R.with_quiet_stretch(R.recipe(n), at, stretch)
    want = R.shifted(want_recipe(rule, "volume", thr, n), at, stretch)
    check_both(monkeypatch, device_trades(cols), rule, "volume", thr, want, rung=1, code=1)


# ---------------------------------------------------------------------------------------------- declines
@pytest.mark.parametrize("rule", ["imbalance", "run"])
def test_bad_amounts_decline(monkeypatch, rule):
    n = 3 * 512 + 100
    px, am, sd = R.recipe(n)
    for bad in (np.nan, -0.5, np.inf):
        for pos in (3, 800, n - 1):                                                     # the first, a middle and the last block
            a = am.copy()
            a[pos] = bad
            want = R.closes(rule, "volume", px, a, sd, 8.0)
            check_both(monkeypatch, device_trades((px, a, sd)), rule, "volume", 8.0, want, rung=1, code=2)


@pytest.mark.parametrize("rule", ["imbalance", "run"])
def test_thresholds_outside_the_domain_decline(monkeypatch, rule):
    cols = R.recipe(4097)
    t = device_trades(cols)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        check_both(monkeypatch, t, rule, "volume", thr, R.closes(rule, "volume", *cols, thr), rung=1, code=2)


@pytest.mark.parametrize("rule", ["imbalance", "run"])
def test_uncertified_tape_declines(monkeypatch, rule):
    """The certificate is global (one quantum for the tape): one amount of 2^-40 beside lots of 2^20 and nothing certifies."""
    n = 2000
    px, _, sd = R.recipe(n)
    am = np.full(n, 2.0 ** 20, np.float32)
    am[777] = 2.0 ** -40
    assert not R.certifies(rule, "volume", px, am, sd, 2.0 ** 23)
    check_both(monkeypatch, device_trades((px, am, sd)), rule, "volume", 2.0 ** 23, R.closes(rule, "volume", px, am, sd, 2.0 ** 23),
               rung=1, code=4)


@pytest.mark.parametrize("rule", ["imbalance", "run"])
def test_no_closes_at_all(monkeypatch, rule):
    n = 70_000
    px, am, _ = R.recipe(n)
    t = device_trades((px, am, np.zeros(n, np.int8)))
    for kind in ("tick", "volume"):
        check_both(monkeypatch, t, rule, kind, 1e9, np.zeros(1, np.int64))
    sd = R.recipe(n)[2]
    want = R.closes(rule, "volume", px, am, sd, 1e9)                                    # sides, but a threshold beyond the tape's total
    assert want.tolist() == [0]
    check_both(monkeypatch, device_trades((px, am, sd)), rule, "volume", 1e9, want)


@pytest.mark.parametrize("rule", ["imbalance", "run"])
def test_ties(monkeypatch, rule):
    n = 100_000
    cols = R.recipe(n, "unit")
    want = want_recipe(rule, "volume", 7.0, n, "unit")
    assert len(want) > 100
    check_both(monkeypatch, device_trades(cols), rule, "volume", 7.0, want)
    check_both(monkeypatch, device_trades(cols), rule, "tick", 7.0, want)               # lots of 1.0: the same bars


# ---------------------------------------------------------------------------------------------- dollar
@pytest.mark.parametrize("rule,thr", [("imbalance", 800.0), ("run", 6400.0)])
def test_dollar_kind(monkeypatch, rule, thr):
    n = 16 * 4096 + 1
    px, am, sd = R.recipe(n)                                                            # prices in quarters, lots in 64ths: certifies
    assert R.certifies(rule, "dollar", px, am, sd, thr)
    want = want_recipe(rule, "dollar", thr, n)
    assert len(want) > 50
    check_both(monkeypatch, device_trades((px, am, sd)), rule, "dollar", thr, want)
    walk = 100.0 * np.exp(np.cumsum(1e-4 * np.random.default_rng(11).standard_normal(n)))
    assert not R.certifies(rule, "dollar", walk, am, sd, thr)                           # full-mantissa products: the serial walk
    check_both(monkeypatch, device_trades((walk, am, sd)), rule, "dollar", thr, R.closes(rule, "dollar", walk, am, sd, thr),
               rung=1, code=4)


# ---------------------------------------------------------------------------------------------- the NumPy-level functions
def test_tick_rule_sides(monkeypatch):
    from finmlkit_amd.bar import logic as L
    from finmlkit_amd.bar.utils import comp_trade_side_vector
    n = 4097
    rng = np.random.default_rng(5)
    px = 100.0 + np.cumsum(rng.integers(-1, 2, n)) * 0.01                               # a third of the moves are zero: the side repeats
    am = (rng.integers(1, 65, n) / 64).astype(np.float32)
    ts = np.arange(n, dtype=np.int64)
    sd = comp_trade_side_vector(px)
    assert sd[0] == 0 and (np.diff(px) == 0).sum() > n // 5
    monkeypatch.delenv("FMK_FLOWBARS_SERIAL", raising=False)
    for f, rule in ((L._imbalance_bar_indexer, "imbalance"), (L._run_bar_indexer, "run")):
        for kind, thr in (("volume", 4.0), ("tick", 9.0), ("dollar", 400.0)):
            want = R.closes(rule, kind, px, am, sd, thr)
            assert len(want) > 3
            got = f(ts, px, am, thr, kind=kind)
            assert got.dtype == np.int64
            np.testing.assert_array_equal(got, want, err_msg=f"{rule}/{kind} tick rule")
            np.testing.assert_array_equal(f(ts, px, am, thr, kind=kind, sides=sd), want, err_msg=f"{rule}/{kind} given sides")
    np.testing.assert_array_equal(L._imbalance_bar_indexer(ts, px, am, 4.0), R.closes("imbalance", "volume", px, am, sd, 4.0))


def test_overwritten_column_is_read_again(monkeypatch):
    from finmlkit_amd._ffi import ptr
    n = 16 * 4096 + 1
    px, am, sd = R.recipe(n)
    t = device_trades((px, am, sd))
    monkeypatch.delenv("FMK_FLOWBARS_SERIAL", raising=False)
    for rule in ("imbalance", "run"):
        first, _ = index(t, rule, "volume", 8.0)
        np.testing.assert_array_equal(first, want_recipe(rule, "volume", 8.0, n))
    am2 = np.ascontiguousarray(am[::-1] * np.float32(0.5))
    t.ctx.call("fmk_h2d", t.amount.p, ptr(am2), C.c_size_t(am2.nbytes))                # in place: same pointer, same arguments
    for rule in ("imbalance", "run"):
        second, d = index(t, rule, "volume", 8.0)
        want = R.closes(rule, "volume", px, am2, sd, 8.0)
        assert not np.array_equal(want, want_recipe(rule, "volume", 8.0, n))
        np.testing.assert_array_equal(second, want)
        assert d["rung"] == 0


# ---------------------------------------------------------------------------------------------- the kits
def test_kits(monkeypatch):
    from finmlkit_amd.bar import ImbalanceBarKit, RunBarKit
    from finmlkit_amd.bar.base import comp_bar_ohlcv
    from finmlkit_amd.bar.data_model import TradesData
    n = 50_000
    px, am, sd = R.recipe(n)
    ts = 1_700_000_000_000_000_000 + np.arange(n, dtype=np.int64) * 50_000_000
    monkeypatch.delenv("FMK_FLOWBARS_SERIAL", raising=False)
    for cls, rule, thr, kind in ((ImbalanceBarKit, "imbalance", 8.0, "volume"), (RunBarKit, "run", 64.0, "volume"),
                                 (ImbalanceBarKit, "imbalance", 16.0, "tick")):
        kit = cls(TradesData(ts, px, am, np.arange(n), side=sd), thr, kind=kind)
        want = R.closes(rule, kind, px, am, sd, thr)
        df = kit.build_ohlcv()
        np.testing.assert_array_equal(kit.bar_close_indices, want[1:])
        np.testing.assert_array_equal(df.index.values.astype(np.int64), ts[want][1:])
        o = comp_bar_ohlcv(px, am, want)
        for k, w in zip(["open", "high", "low", "close", "volume", "vwap", "trades", "median_trade_size"], o):
            np.testing.assert_array_equal(df[k].values, w, err_msg=f"{rule} {k}")
    with pytest.raises(ValueError, match="side column"):
        ImbalanceBarKit(TradesData(ts, px, am, np.arange(n)), 8.0).build_ohlcv()
