"""GPU: WHICH rung of the volume / dollar bar ladders answers, and every hand-off between rungs.

The indexers are ladders of kernels whose last rung, the serial walk, is always right: a rung that wrongly declines every tape, or
that no tape reaches, changes no close.  Every case here is a tape built for ONE rung (tests/_tier_tapes.py: the tape, the tier and
the tried mask are literals of the case table, checked on the host by tests/test_threshold_tier_tapes.py) and asserts
  1. the closes equal the sequential oracle's exactly,
  2. n_uncertified == 0 in the default mode,
  3. in the fast mode the closes are equal or n_uncertified > 0,
  4. the answering tier (fmk_diag_volume_last / fmk_diag_dollar_last + fmk_diag_dollar_source) is the one the tape was built for,
  5. the tried mask and the return code of every declining tier are the documented way there,
and that est_len / mean_len of the diagnostic agree with math.fsum on the host to n x 2^-53 relative (the bound of a float64 sum
of n positive terms): the tape on the device is the tape of the table.  Every call is a count call (null output) followed by its
fill, so every case also checks that the fill answers from the one-shot cache and tries nothing."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _counts
from tests import _tier_tapes as T

pytestmark = pytest.mark.gpu

c_i64, c_f64 = C.c_int64, C.c_double


def _ctx():
    from finmlkit_amd import _ffi
    return _ffi.default_context()


def _upload(a):
    from finmlkit_amd._ffi import DeviceArray
    return DeviceArray.from_host(_ctx(), a)


def _vol_diag():
    from finmlkit_amd import _ffi
    return T.read_volume_diag(_ffi.lib())


def _dol_diag():
    from finmlkit_amd import _ffi
    return T.read_dollar_diag(_ffi.lib())


def _count(fn, cols, n, thr):
    m, unc = c_i64(), c_i64(-1)
    _ctx().call(fn, *cols, c_i64(n), c_f64(thr), None, c_i64(0), C.byref(m), C.byref(unc))
    return m.value, unc.value


def _fill(fn, cols, n, thr, count):
    from finmlkit_amd._ffi import DeviceArray
    m, unc = c_i64(), c_i64(-1)
    out = DeviceArray(_ctx(), count, np.int64)
    _ctx().call(fn, *cols, c_i64(n), c_f64(thr), out.p, c_i64(count), C.byref(m), C.byref(unc))
    assert m.value == count
    return out.to_host(), unc.value


VOL_FN, DOL_FN = "fmk_volume_bar_indexer_dev", "fmk_dollar_bar_indexer_dev"


def _vol_cols(d_am):
    return (d_am.p, C.c_int(1 if d_am.dtype == np.float64 else 0))


def _dol_cols(d_px, d_am):
    return (d_px.p, d_am.p, C.c_int(1 if d_am.dtype == np.float64 else 0))


def _pair(fn, cols, n, thr, diag):
    """count call, its diagnostic, fill call, its diagnostic"""
    count, _ = _count(fn, cols, n, thr)
    d_count = diag()
    closes, unc = _fill(fn, cols, n, thr, count)
    return closes, unc, d_count, diag()


def _fast(fn, cols, n, thr):
    ctx = _ctx()
    ctx.set_fast_threshold(True)
    try:
        count, _ = _count(fn, cols, n, thr)
        return _fill(fn, cols, n, thr, count)
    finally:
        ctx.set_fast_threshold(False)


def _close_to(got, want, n):
    """n x 2^-53 relative: a float64 sum of n positive terms against the correctly rounded one"""
    return abs(got - want) <= n * 2.0 ** -53 * abs(want)


# ------------------------------------------------------------------------------------------------------------------------------
# volume bars
# ------------------------------------------------------------------------------------------------------------------------------
VOL = T.volume_cases()


@pytest.mark.parametrize("case", VOL, ids=lambda c: c.id)
def test_volume_tier(orc, monkeypatch, case):
    if case.env:
        monkeypatch.setenv(*case.env)
    a, thr = case.make()
    n = len(a)
    want = orc._volume_bar_indexer(a, thr)
    d_am = _upload(a)
    cols = _vol_cols(d_am)
    got, unc, d, d_fill = _pair(VOL_FN, cols, n, thr, _vol_diag)
    print(f"{case.name}: tier {T.TIER_NAMES[d['tier']]} tried {d['tried']:#x} codes {d['codes']} est_len {d['est_len']!r} "
          f"mean_len {d['mean_len']!r} listed {d['listed']} closes {len(want)}")
    _counts.record(f"tiers::volume::{case.name}", tier=T.TIER_NAMES[d["tier"]] if d["tier"] >= 0 else "none", tried=d["tried"],
                   est_len=d["est_len"], mean_len=d["mean_len"], listed=d["listed"], closes=len(want), n=n)
    np.testing.assert_array_equal(got, want)                                                    # 1
    assert unc == 0                                                                             # 2
    fast, unc_fast = _fast(VOL_FN, cols, n, thr)
    assert np.array_equal(fast, want) or unc_fast > 0                                           # 3
    if case.fast_reports:
        assert unc_fast > 0, "the tape puts a decision on a knife edge: the parallel mode must list it"
    if case.listed:
        assert case.listed[0] <= d["listed"] <= case.listed[1], d["listed"]
    if case.also and d["tier"] != case.tier:                                                    # 4, at the limit W itself: this class or the next
        assert d["tier"] in case.also, T.TIER_NAMES[d["tier"]]
    else:
        assert T.TIER_NAMES[d["tier"]] == T.TIER_NAMES[case.tier]                               # 4
        assert d["tried"] == T.mask(case.tried) and d["codes"] == T.codes(case.tried)           # 5
    # the fill half: the serial walk keeps its own result (fmk_threshold.hip), every other tier's closes come from the one-shot cache
    assert d_fill["tier"] == (T.SERIAL if d["tier"] == T.SERIAL else T.CACHED)
    if d_fill["tier"] == T.CACHED:
        assert d_fill["tried"] == 0 and not any(d_fill["codes"]) and math.isnan(d_fill["est_len"]) and math.isnan(d_fill["mean_len"])
    # the two estimates: the tape on the device is the tape of the table
    if case.serial:
        assert math.isnan(d["est_len"]) and math.isnan(d["mean_len"])
    elif case.bad_in_sample == "nan":
        assert d["est_len"] == 1e300 and math.isnan(d["mean_len"])
    else:
        finite = np.nan_to_num(np.asarray(a, np.float64), nan=0.0) if case.bad_anywhere else a
        est, mean = T.estimates(finite, thr)
        if not (case.bad_anywhere and np.isnan(np.asarray(a[:T.SAMPLE], np.float64)).any()):
            assert _close_to(d["est_len"], est, min(n, T.SAMPLE)), (d["est_len"], est)
        total_pass_ran = bool(case.tried.get(T.LDS) or case.tried.get(T.P_TOTAL) or d["est_len"] >= T.EST_LDS) and d["tier"] == case.tier
        if total_pass_ran and not case.bad_anywhere:
            assert _close_to(d["mean_len"], mean, n), (d["mean_len"], mean)
        elif d["tier"] == case.tier:
            assert math.isnan(d["mean_len"])
    if case.tier in T.CLASSES and d["tier"] == case.tier:
        assert d["listed"] == 0                                 # exact sums: no tie zone, nothing to replay


def test_volume_cache_is_one_shot_and_sees_an_overwrite_after_the_pair(orc):
    """include/fmk.h makes count (d_close_idx == NULL) and fill the two phases of ONE call on ONE tape and promises nothing for a tape
    that is overwritten in place BETWEEN them (the cache is keyed on the pointer), so that is not tested.  What the code promises
    ("one-shot cache: the inputs may change behind the same pointers"): after a COMPLETED pair the same call on the same DeviceArray
    with new amounts is a miss and gives the new tape's closes."""
    n, thr = 200_000, 100.0
    a = T.dyadic_lots(301, n, False)
    b = T.dyadic_lots(302, n, False)
    d_am = _upload(a)
    cols = _vol_cols(d_am)
    got, unc, d, d_fill = _pair(VOL_FN, cols, n, thr, _vol_diag)
    np.testing.assert_array_equal(got, orc._volume_bar_indexer(a, thr))
    assert d["tier"] == T.E1024 and d_fill["tier"] == T.CACHED and d_fill["tried"] == 0
    _ctx().call("fmk_h2d", d_am.p, b.ctypes.data_as(C.c_void_p), C.c_size_t(b.nbytes))         # in place, same pointer
    got2, unc2, d2, d2_fill = _pair(VOL_FN, cols, n, thr, _vol_diag)
    assert d2["tier"] == T.E1024, "the call after a completed pair must compute again"
    want2 = orc._volume_bar_indexer(b, thr)
    assert not np.array_equal(want2, got)
    np.testing.assert_array_equal(got2, want2)
    assert unc == 0 and unc2 == 0 and d2_fill["tier"] == T.CACHED
    _counts.record("tiers::volume::cache_overwrite_after_pair", tier="cached", closes=len(got) + len(got2), n=n)


def test_volume_cache_misses_when_the_block_was_freed_and_handed_out_again(orc):
    """Between a count and its fill the amounts are freed and another tape of the same size is allocated: the pool hands out the same
    block, so pointer, n and threshold all match -- the stale flag fmk_free sets on the cache is what makes the fill a miss."""
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ctx()
    ctx.trim()                                                   # an empty free list: the next block of this size is the one just freed
    n, thr = 77_771, 100.0
    a = T.dyadic_lots(303, n, True)
    b = T.dyadic_lots(304, n, True)
    d_am = _upload(a)
    p0 = d_am.ptr
    count, _ = _count(VOL_FN, _vol_cols(d_am), n, thr)
    assert _vol_diag()["tier"] == T.E1024 and count == len(orc._volume_bar_indexer(a, thr))
    d_am.free()
    d_b = _upload(b)
    assert d_b.ptr == p0, "construction: the pool should hand the freed block out again"
    want = orc._volume_bar_indexer(b, thr)
    assert not np.array_equal(want, orc._volume_bar_indexer(a, thr))
    m, unc = c_i64(), c_i64(-1)
    out = DeviceArray(ctx, max(count, len(want)), np.int64)
    ctx.call(VOL_FN, *_vol_cols(d_b), c_i64(n), c_f64(thr), out.p, c_i64(out.n), C.byref(m), C.byref(unc))
    d = _vol_diag()
    assert d["tier"] == T.E1024, f"the fill answered from a stale cache ({T.TIER_NAMES[d['tier']]})"
    np.testing.assert_array_equal(out.to_host()[:m.value], want)
    assert unc.value == 0
    _counts.record("tiers::volume::cache_stale_after_free", tier=T.TIER_NAMES[d["tier"]], closes=len(want), n=n)


# ------------------------------------------------------------------------------------------------------------------------------
# dollar bars
# ------------------------------------------------------------------------------------------------------------------------------
DOL = T.dollar_cases()
FORM = {T.ONEPASS: "one-pass", T.TWOPASS: "two-pass", T.NEITHER: "neither"}


@pytest.mark.parametrize("case", DOL, ids=lambda c: c.id)
def test_dollar_path(orc, monkeypatch, case):
    if case.env:
        monkeypatch.setenv(*case.env)
    px, am, thr = T.block_trade_tape(orc) if case.make is None else case.make()
    n = len(px)
    want = orc._dollar_bar_indexer(px, am, thr)
    d_px, d_am = _upload(px), _upload(am)
    cols = _dol_cols(d_px, d_am)
    got, unc, d, d_fill = _pair(DOL_FN, cols, n, thr, _dol_diag)
    print(f"{case.name}: path {d['path']} closed form {FORM[d['closed_form']]} closes {len(want)}")
    _counts.record(f"tiers::dollar::{case.name}", path=d["path"], closed_form=FORM[d["closed_form"]], closes=len(want), n=n)
    np.testing.assert_array_equal(got, want)                                                    # 1
    assert unc == 0                                                                             # 2
    fast, unc_fast = _fast(DOL_FN, cols, n, thr)
    assert np.array_equal(fast, want) or unc_fast > 0                                           # 3
    if case.fast_reports:
        assert unc_fast > 0, "the tape was built so that the exact tier has something to do"
    assert (d["path"], FORM[d["closed_form"]]) == (case.path, FORM[case.closed_form])           # 4, 5
    assert d["cached"] == 0
    # the fill half leaves the path alone (include/fmk_diag.h) and says that it copied
    assert d_fill["path"] == case.path
    assert d_fill["cached"] == (0 if case.path == 3 else 1)


def test_dollar_cache_is_one_shot_and_sees_an_overwrite_after_the_pair(orc):
    """As for volume bars: only what holds after a COMPLETED pair is promised."""
    n = 100_000
    px, am = T.integer_tape(311, n)
    px2, am2 = T.integer_tape(312, n)
    thr = 10_000.0 + T.CERTAIN_FRAC        # < 256 closes: no multiple of thr is an integer
    d_px, d_am = _upload(px), _upload(am)
    cols = _dol_cols(d_px, d_am)
    got, unc, d, d_fill = _pair(DOL_FN, cols, n, thr, _dol_diag)
    np.testing.assert_array_equal(got, orc._dollar_bar_indexer(px, am, thr))
    assert (d["path"], d["closed_form"], d["cached"], d_fill["cached"]) == (0, T.ONEPASS, 0, 1)
    _ctx().call("fmk_h2d", d_am.p, am2.ctypes.data_as(C.c_void_p), C.c_size_t(am2.nbytes))
    _ctx().call("fmk_h2d", d_px.p, px2.ctypes.data_as(C.c_void_p), C.c_size_t(px2.nbytes))
    got2, unc2, d2, d2_fill = _pair(DOL_FN, cols, n, thr, _dol_diag)
    assert d2["cached"] == 0 and d2_fill["cached"] == 1
    want2 = orc._dollar_bar_indexer(px2, am2, thr)
    assert not np.array_equal(want2, got)
    np.testing.assert_array_equal(got2, want2)
    assert unc == 0 and unc2 == 0
    _counts.record("tiers::dollar::cache_overwrite_after_pair", path=d2["path"], closes=len(got) + len(got2), n=n)


def test_dollar_cache_misses_when_the_block_was_freed_and_handed_out_again(orc):
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ctx()
    ctx.trim()
    n = 77_773
    px, am = T.integer_tape(313, n)
    _, am2 = T.integer_tape(314, n)
    thr = 10_000.0 + T.CERTAIN_FRAC        # < 256 closes: no multiple of thr is an integer
    d_px, d_am = _upload(px), _upload(am)
    p0 = d_am.ptr
    count, _ = _count(DOL_FN, _dol_cols(d_px, d_am), n, thr)
    assert _dol_diag()["cached"] == 0 and count == len(orc._dollar_bar_indexer(px, am, thr))
    d_am.free()
    d_b = _upload(am2)
    assert d_b.ptr == p0, "construction: the pool should hand the freed block out again"
    want = orc._dollar_bar_indexer(px, am2, thr)
    assert not np.array_equal(want, orc._dollar_bar_indexer(px, am, thr))
    m, unc = c_i64(), c_i64(-1)
    out = DeviceArray(ctx, max(count, len(want)), np.int64)
    ctx.call(DOL_FN, *_dol_cols(d_px, d_b), c_i64(n), c_f64(thr), out.p, c_i64(out.n), C.byref(m), C.byref(unc))
    d = _dol_diag()
    assert d["cached"] == 0, "the fill answered from a stale cache"
    np.testing.assert_array_equal(out.to_host()[:m.value], want)
    assert unc.value == 0 and (d["path"], d["closed_form"]) == (0, T.ONEPASS)
    _counts.record("tiers::dollar::cache_stale_after_free", path=d["path"], closes=len(want), n=n)
