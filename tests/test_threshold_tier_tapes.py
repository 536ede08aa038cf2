"""Host side of tests/test_gpu_threshold_tiers.py (no GPU): every tape of tests/_tier_tapes.py regenerates bit for bit (amounts,
threshold, the oracle's closes, the fsum estimates), sits inside the band of the rung it was built for, and a host model of the
ladder of fmk_volume_bar_indexer_dev lands on the tier and the tried mask the case table states."""
import numpy as np
import pytest

from tests import _tier_tapes as T

VOL = T.volume_cases()
DOL = T.dollar_cases()


def test_case_names_are_unique_and_every_tier_is_aimed_at():
    names = [c.name for c in VOL] + [c.name for c in DOL]
    assert len(set(names)) == len(names)
    assert {c.tier for c in VOL} == {T.E1024, T.E1536, T.E2048, T.LDS, T.LDS_TOTAL, T.GLOBAL, T.CHAIN, T.SERIAL}
    assert {(c.path, c.closed_form) for c in DOL} >= {(0, T.ONEPASS), (0, T.TWOPASS), (1, T.ONEPASS), (2, T.TWOPASS), (3, T.NEITHER)}


@pytest.mark.parametrize("case", VOL, ids=lambda c: c.id)
def test_volume_tape_is_the_one_the_table_describes(orc, case):
    a, thr = case.make()
    b, thr2 = case.make()
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes() and repr(thr) == repr(thr2)
    assert len(a) <= 1 << 21
    want = orc._volume_bar_indexer(a, thr)
    np.testing.assert_array_equal(want, orc._volume_bar_indexer(b, thr2))
    if not case.serial and not case.bad_anywhere:
        est, mean = T.estimates(a, thr)
        assert (est, mean) == T.estimates(b, thr2)
        if case.est_band:
            lo, hi = case.est_band
            assert lo <= est < hi, f"est_len {est} outside {case.est_band}"
        if case.mean_band:
            lo, hi = case.mean_band
            assert lo <= mean < hi, f"mean_len {mean} outside {case.mean_band}"
    if case.model_skips:
        return
    tier, tried = T.model(a, thr, case.certifies, case.bad_in_sample, case.bad_anywhere, case.serial)
    if case.also and tier != case.tier:
        assert tier in case.also
    else:
        assert (T.TIER_NAMES[tier], tried) == (T.TIER_NAMES[case.tier], case.tried)


@pytest.mark.parametrize("name,longest", [(c.name, int(c.name.rsplit("_", 1)[1])) for c in VOL if c.name.startswith("limit_")]
                         + [(c.name, int(c.name.split("_")[1])) for c in VOL if c.name.startswith("handoff_")])
def test_quiet_stretch_makes_the_longest_bar_the_table_names(orc, name, longest):
    case = next(c for c in VOL if c.name == name)
    a, thr = case.make()
    closes = orc._volume_bar_indexer(a, thr)
    bars = np.diff(closes)
    bars[0] += 1                                               # the first bar counts tick 0
    assert int(bars.max()) == longest


@pytest.mark.parametrize("case", DOL, ids=lambda c: c.id)
def test_dollar_tape_is_the_one_the_table_describes(orc, case):
    if case.make is None:
        px, am, thr = T.block_trade_tape(orc)
        px2, am2, thr2 = T.block_trade_tape(orc)
        d = px * am.astype(np.float64)
        big = d[d >= thr] / thr
        assert len(big) >= 150 and big.min() >= 1.19 and big.max() <= 9.01
    else:
        px, am, thr = case.make()
        px2, am2, thr2 = case.make()
    assert px.tobytes() == px2.tobytes() and am.tobytes() == am2.tobytes() and am.dtype == am2.dtype and repr(thr) == repr(thr2)
    assert len(px) <= 1 << 21
    np.testing.assert_array_equal(orc._dollar_bar_indexer(px, am, thr), orc._dollar_bar_indexer(px2, am2, thr2))
    d = px * am.astype(np.float64)
    if case.certain:
        whales = d[d >= thr] / thr
        assert case.closed_form == (T.TWOPASS if len(whales) or len(px) < 2 else T.ONEPASS)
        assert T.margin_of_certain_tape(px, am, thr, float(np.sum(whales)) ** 2) > 50.0
    if case.path in (1, 2) and case.closed_form == T.ONEPASS:
        assert float(d.max()) < thr and float(d.min()) >= 0.0
    if case.name.startswith("path1_tenths"):
        assert T.exact_decimal_ties(px, am, thr) >= 10
    if case.name == "path3_whale_of_600_thresholds":
        assert float(d.max()) == 600 * thr and T.exact_decimal_ties(px, am, thr) >= 10


def test_decimal_tape_has_more_fragile_ticks_than_the_global_tables_replay():
    """vol_global_tables returns 3 when (fragile ticks, estimated from every 64th 512-tick block) x mean_len > 24 000 n.  Every tick
    whose bar closes is fragile here -- those in front of the last mean_len ticks -- and mean_len is 60 000: twice the limit."""
    case = next(c for c in VOL if c.name == "serial_replay_dearer_than_the_walk")
    a, thr = case.make()
    n = len(a)
    _, mean = T.estimates(a, thr)
    fragile = T.ticks_whose_bar_hits_the_threshold_exactly(a, thr)
    assert fragile >= n - mean - 2 and fragile * mean > 2.0 * 24000.0 * n
