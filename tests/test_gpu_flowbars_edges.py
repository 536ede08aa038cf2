"""GPU: imbalance and run bars at the hand-offs of the tables rung (csrc/fmk_flowbars.hip), against the loops that define them or
a closed form that tests/test_flowbars_host.py proves equal to the loops.  Every comparison goes through check_both of
tests/test_gpu_flowbars.py: the library's own choice of rung with the expected (rung, code), then the forced serial walk, both
array_equal to the reference.  Groups, as the sections below:
  A  thresholds between two multiples of the quantum, and below one lot (fb_certificate's ceil and its c < 1 -> 1)
  B  a tape one quantum inside and one exactly on sum |x| + T = 2^53 q
  C  links of exactly K ticks on one-sided tapes: closes on the last tick of a block, the first of the next, destination blocks
     63 / 64 / 65 of the link search, table spans 2^12 / 2^12 + 1; `longest` and `ls` of the diagnostics
  D  the table-span limit: a longest link of 2^22 (tables) and 2^22 + 1 (declined with code 1, found in the last search round)
  E  links across dozens to hundreds of blocks whose summaries all move
  F  a close on every tick
  G  biased and one-sided flow with sides of 0 and lots of 0, all kinds; sign and power-of-two scaling symmetries
  H  the hand-written tapes of tests/_flowbars_ref.py, alone and in front of a second, short block
  I  dollar kind with float64 amounts, dollar kind with unusable prices, tick kind beside an unusable amount column"""
import math

import numpy as np
import pytest

from tests import _flowbars_ref as R
from tests import test_gpu_flowbars as G
from tests.test_gpu_flowbars import check_both, device_trades, index, want_recipe

pytestmark = pytest.mark.gpu

RULES = ("imbalance", "run")
BIG = (1 << 20) + 1


def check_links(monkeypatch, t, rule, kind, thr, want, longest, rung=0, code=0, ls=None):
    """check_both, and the longest link that its first call (the library's own choice) reported in the diagnostics."""
    seen = []

    def recording(*args):
        got, d = index(*args)
        seen.append(d)
        return got, d

    monkeypatch.setattr(G, "index", recording)
    check_both(monkeypatch, t, rule, kind, thr, want, rung=rung, code=code, ls=ls)
    monkeypatch.setattr(G, "index", index)
    assert len(seen) == 2 and seen[0]["longest"] == longest, (rule, kind, thr, t.n, seen)


# ---------------------------------------------------------------------------------------------- A: threshold rounding
@pytest.mark.parametrize("rule", RULES)
def test_threshold_rounds_up_to_the_quantum(monkeypatch, rule):
    n = 65537
    cols = R.recipe(n)
    t = device_trades(cols)
    below, eight, above, next_lot, lot, sub_lot = R.ROUNDING_THR
    w8, w8n = want_recipe(rule, "volume", eight, n), want_recipe(rule, "volume", next_lot, n)
    assert np.array_equal(R.closes(rule, "volume", *cols, below), w8)
    assert np.array_equal(R.closes(rule, "volume", *cols, above), w8n) and not np.array_equal(w8, w8n)
    for thr, want in ((below, w8), (eight, w8), (above, w8n), (next_lot, w8n)):
        check_both(monkeypatch, t, rule, "volume", thr, want)
    for thr in (lot, sub_lot):                                      # every lot is at least 1 / 64: every tick closes
        want = R.closes(rule, "volume", *cols, thr)
        assert len(want) == n
        check_both(monkeypatch, t, rule, "volume", thr, want)


@pytest.mark.parametrize("rule", RULES)
def test_a_threshold_that_vanishes_against_the_quantum(monkeypatch, rule):
    """Lots of 2^100 and the smallest positive threshold: thr / q underflows to zero, and T must become one quantum, not zero."""
    n, thr = 3 * 512 + 5, 5e-324
    assert thr > 0.0 and math.ldexp(thr, -100) == 0.0
    for sign in (1, -1):
        cols = R.one_sided(n, sign, lot=2.0 ** 100)
        want = R.closes(rule, "volume", *cols, thr)
        assert np.array_equal(want, np.arange(n)) and R.certifies(rule, "volume", *cols, thr)
        check_links(monkeypatch, device_trades(cols), rule, "volume", thr, want, longest=1, ls=12)


# ---------------------------------------------------------------------------------------------- B: the certificate's edge
@pytest.mark.parametrize("rule", RULES)
def test_certificate_edge(monkeypatch, rule):
    thr, want = R.CERT_EDGE_THR, np.array(R.CERT_EDGE_CLOSES, np.int64)
    for X, certified in zip(R.CERT_EDGE_X, (True, False)):
        cols = R.certificate_edge(X)
        assert cols[1].dtype == np.float64 and R.certifies(rule, "volume", *cols, thr) == certified
        assert np.array_equal(R.closes(rule, "volume", *cols, thr), want)
        check_both(monkeypatch, device_trades(cols), rule, "volume", thr, want, rung=0 if certified else 1, code=0 if certified else 4)


# ---------------------------------------------------------------------------------------------- C: block and round hand-offs
# K = 512: every close is the last tick of a block (r = 511) and its link lands on the same offset one block on; 513: r = 0.
# 32768 / 33280: the link lands 64 / 65 blocks on, the last summary of the first search round (i = 63) and the first of the
# second (r = 1, i = 0).  4096 / 4097: the table span goes from 2^12 to 2^13.
LINKS = (1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32767, 32768, 32769, 33280)


@pytest.mark.parametrize("K", LINKS)
def test_links_of_exactly_k_ticks(monkeypatch, K):
    ls = max(12, math.ceil(math.log2(K)))
    assert (1 << ls) >= K and (ls == 12 or (1 << (ls - 1)) < K)
    for n in (3 * K + 5, 3 * K, 3 * K - 1):                         # an open last bar, a close on tick n - 1, one tick fewer
        want = R.closes_one_sided(n, K)                             # equal to the loops: tests/test_flowbars_host.py
        assert (want[-1] == n - 1) == (n == 3 * K or K == 1)
        for sign in (1, -1):
            t = device_trades(R.one_sided(n, sign))
            for rule in RULES:
                for kind in ("tick", "volume"):
                    check_links(monkeypatch, t, rule, kind, float(K), want, longest=K, ls=ls)


# ---------------------------------------------------------------------------------------------- D: the table-span limit
SPAN = 1 << 22


@pytest.fixture(scope="module")
def span_tape():
    """one_sided(2^22 + 600, +1) on the device, uploaded once for the cases of D and given back behind them."""
    t = device_trades(R.one_sided(SPAN + 600, 1))
    yield t
    for col in (t.ts, t.price, t.amount, t.side, t.price_k):
        if col is not None:
            col.free()


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("rule", RULES)
def test_the_longest_link_the_tables_take(monkeypatch, span_tape, rule, over):
    """A link of 2^22 ticks lands 8192 blocks on, the last summary of search round 127: the tables answer with a span of 2^22.  One
    of 2^22 + 1 that starts on the last tick of a block (tick 511 closes at 2^22 + 512 < n) lands 8193 blocks on, in round 128, the
    last: found, reported, and too long for any table (code 1).  The reference is the closed form (tests/test_flowbars_host.py)."""
    want = np.array([0, SPAN - 1 + over], np.int64)
    assert np.array_equal(want, R.closes_one_sided(span_tape.n, SPAN + over))
    if over:
        check_links(monkeypatch, span_tape, rule, "tick", float(SPAN + 1), want, longest=SPAN + 1, rung=1, code=1)
    else:
        check_links(monkeypatch, span_tape, rule, "tick", float(SPAN), want, longest=SPAN, ls=22)


# ---------------------------------------------------------------------------------------------- E: long bars with live flow
@pytest.mark.parametrize("rule,thr,longest", R.LONG_BARS)
def test_long_bars_with_live_flow(monkeypatch, rule, thr, longest):
    want = want_recipe(rule, "volume", thr, BIG)
    assert np.diff(want).max() == longest
    if (rule, thr) == R.LONG_BARS[0][:2]:
        assert longest > 65 * 512                                   # beyond the first round of 64 block summaries
    t = device_trades(R.recipe(BIG))
    check_both(monkeypatch, t, rule, "volume", thr, want)
    monkeypatch.delenv("FMK_FLOWBARS_SERIAL", raising=False)
    _, d = index(t, rule, "volume", thr)                            # `longest` is over the links of ALL ticks, on the chain or not
    assert d["rung"] == 0 and d["longest"] >= longest and (1 << d["ls"]) >= d["longest"] and (1 << (d["ls"] - 1)) < d["longest"], d


# ---------------------------------------------------------------------------------------------- F: dense closes
@pytest.mark.parametrize("kind,thr", [("volume", 1.0 / 64), ("tick", 1.0)])
@pytest.mark.parametrize("rule", RULES)
def test_a_close_on_every_tick(monkeypatch, rule, kind, thr):
    want = want_recipe(rule, kind, thr, BIG)
    assert np.array_equal(want, np.arange(BIG))
    check_links(monkeypatch, device_trades(R.recipe(BIG)), rule, kind, thr, want, longest=1, ls=12)


# ---------------------------------------------------------------------------------------------- G: one-sided and biased flow
@pytest.mark.parametrize("p_up", [0.5, 0.7, 1.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_biased_flow_and_its_symmetries(monkeypatch, seed, p_up):
    n = 16 * 4096 + 1
    px, am, sd = R.biased(n, seed, p_up, 0.1, 0.05)
    t = device_trades((px, am, sd))
    neg = device_trades((px, am, -sd))                              # buys and sells swapped: the same closes
    scaled = {e: device_trades((px, am * np.float32(2.0 ** e), sd)) for e in (-20, 30)}
    for rule in RULES:
        for kind, thr in (("volume", 8.0), ("tick", 16.0), ("dollar", 800.0)):
            want = R.closes(rule, kind, px, am, sd, thr)
            assert len(want) > 100
            check_both(monkeypatch, t, rule, kind, thr, want)
            assert np.array_equal(R.closes(rule, kind, px, am, -sd, thr), want)
            check_both(monkeypatch, neg, rule, kind, thr, want)
            if kind == "tick":
                continue                                            # the amounts play no part
            for e, ts in scaled.items():                            # a power of two: every sum scales exactly, float32 amounts stay exact
                a2, thr2 = am * np.float32(2.0 ** e), thr * 2.0 ** e
                assert a2.dtype == np.float32 and np.array_equal(a2.astype(np.float64), am.astype(np.float64) * 2.0 ** e)
                assert np.array_equal(R.closes(rule, kind, px, a2, sd, thr2), want)
                check_both(monkeypatch, ts, rule, kind, thr2, want)


# ---------------------------------------------------------------------------------------------- H: the hand-written tapes
@pytest.mark.parametrize("group", sorted(R.HAND_TAPES))
def test_hand_written_tapes(monkeypatch, group):
    from finmlkit_amd.bar import logic as L
    for sides, sizes, thr, written in R.HAND_TAPES[group]:
        for pad in (0, 600):                                        # alone; with a second block and a short last one behind it
            cols = R.hand_tape_columns(sides, sizes, pad)
            n = len(cols[0])
            for rule in RULES:
                want = R.closes(rule, "volume", *cols, thr)
                if not (len(sides) == 1 and pad):                   # (tick 0 alone at thr closes on the first tick behind it)
                    assert want.tolist() == written.get(rule, want.tolist())
                if n == 0:                                          # the C entry point refuses an empty tape; the NumPy level answers [0]
                    f = L._imbalance_bar_indexer if rule == "imbalance" else L._run_bar_indexer
                    got = f(np.zeros(0, np.int64), cols[0], cols[1], thr, kind="volume", sides=cols[2])
                    assert got.dtype == np.int64 and got.tolist() == [0] == want.tolist()
                    continue
                if group == "nan_amount":
                    check_both(monkeypatch, device_trades(cols), rule, "volume", thr, want, rung=1, code=2)
                    check_both(monkeypatch, device_trades(cols, f64=True), rule, "volume", thr, want, rung=1, code=2)
                    continue
                assert R.certifies(rule, "volume", *cols, thr)
                check_both(monkeypatch, device_trades(cols), rule, "volume", thr, want)
                # the written sizes as float64: 0.999 has a quantum of 2^-53 or less and cannot certify beside a total of 3
                c64 = (cols[0], np.concatenate([np.asarray(sizes, np.float64), np.ones(pad)]), cols[2])
                ok = R.certifies(rule, "volume", *c64, thr)
                assert ok == (0.999 not in sizes)
                check_both(monkeypatch, device_trades(c64), rule, "volume", thr, R.closes(rule, "volume", *c64, thr),
                           rung=0 if ok else 1, code=0 if ok else 4)


# ---------------------------------------------------------------------------------------------- I: untested instantiations
@pytest.mark.parametrize("rule,thr", [("imbalance", 800.0), ("run", 6400.0)])
def test_dollar_kind_with_float64_amounts(monkeypatch, rule, thr):
    n = 16 * 4096 + 1
    want = want_recipe(rule, "dollar", thr, n)
    assert len(want) > 50
    check_both(monkeypatch, device_trades(R.recipe(n), f64=True), rule, "dollar", thr, want)


@pytest.mark.parametrize("rule", RULES)
def test_bad_prices_decline(monkeypatch, rule):
    n = 3 * 512 + 100
    px, am, sd = R.recipe(n)
    for bad, amount in ((np.nan, None), (-1.0, None), (np.inf, None), (1e300, 1e10)):
        for pos in (3, 800, n - 1):                                 # the first, a middle and the last block
            p = px.copy()
            p[pos] = bad
            a = am if amount is None else am.astype(np.float64)
            if amount is not None:
                a[pos] = amount                                     # both finite; their float64 product is not
                assert np.isfinite(p).all() and np.isfinite(a).all()
            with np.errstate(over="ignore", invalid="ignore"):
                want = R.closes(rule, "dollar", p, a, sd, 800.0)
            check_both(monkeypatch, device_trades((p, a, sd)), rule, "dollar", 800.0, want, rung=1, code=2)


@pytest.mark.parametrize("rule", RULES)
def test_tick_kind_leaves_the_amounts_alone(monkeypatch, rule):
    n = 16 * 4096 + 1
    px, am, sd = R.recipe(n)
    for f64 in (False, True):
        a = am.astype(np.float64) if f64 else am.copy()
        a[5], a[n // 2] = np.nan, -3.0
        check_both(monkeypatch, device_trades((px, a, sd)), rule, "tick", 16.0, want_recipe(rule, "tick", 16.0, n))
