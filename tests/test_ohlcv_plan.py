"""CPU-only: the decision table of comp_bar_ohlcv's first pass (ohlcv_plan, finmlkit_amd/csrc/fmk_ohlcv.hip) through
fmk_diag_ohlcv_plan -- plain numbers in, the schedule out, no device.  Every boundary is walked from both sides; all values exact."""
import itertools

import pytest

from finmlkit_amd import _ffi

N_CU = 256
ROW_WAVES = 4                     # OHR_WAVES: waves per workgroup of the rows kernels


def cdiv(a, b):
    return -(-a // b)


def capped(blocks, per_cu, n_cu=N_CU):
    return max(1, min(blocks, n_cu * per_cu))


def expected(n, nb, f64, median, fused, min_stage=4096, n_cu=N_CU):
    """the table, written down independently of the C++ cascade: float32 rules 1..7 in order, float64 only 5..7"""
    mean = n // nb
    z = dict(kind="small", tile=0, lanes=0, nch=0, grid=0, block=256, long_min=0, first_stage=0)
    if not f64:
        if fused and mean > 600 and nb // 8 >= min_stage and min_stage >= 256:
            first = (nb // 8) & ~255
            return dict(z, kind="pipelined", nch=21, grid=capped(cdiv(first, 4), 64, n_cu), long_min=1344, first_stage=first)
        if median and nb >= 64 and 33 <= mean < 64:
            return dict(z, kind="rows", lanes=8, grid=capped(cdiv(cdiv(nb, 8), ROW_WAVES), 32, n_cu), block=64 * ROW_WAVES, long_min=128)
        if nb >= 64 and mean <= (32 if median else 56):
            return dict(z, kind="lanes", tile=2048 if mean > 44 else 1024, grid=capped(cdiv(cdiv(nb, 64), 2), 96, n_cu), block=128,
                        long_min=64)
        if nb >= 64 and mean <= 210:
            return dict(z, kind="rows", lanes=16, grid=capped(cdiv(cdiv(nb, 4), ROW_WAVES), 32, n_cu), block=64 * ROW_WAVES, long_min=256)
    if mean <= 210:
        return dict(z, nch=4, grid=capped(cdiv(nb, 4), 128, n_cu), long_min=256)
    if mean <= 600:
        return dict(z, nch=10, grid=capped(cdiv(nb, 4), 96, n_cu), long_min=640)
    return dict(z, nch=21, grid=capped(cdiv(nb, 4), 64, n_cu), long_min=1344)


def plan(n, nb, f64=False, median=True, fused=False, min_stage=4096, n_cu=N_CU):
    return _ffi.ohlcv_plan(n, nb, amount_is_f64=f64, want_median=median, time_bar_fused=fused, n_cu=n_cu, pipe_min_stage=min_stage)


MEANS = (1, 32, 33, 44, 45, 56, 57, 63, 64, 65, 210, 211, 600, 601, 1200, 20000)
BARS = (1, 63, 64, 1000, 8 * 4095 + 7, 8 * 4096, 300000, 5000000)


@pytest.mark.parametrize("f64,median,fused", list(itertools.product((False, True), repeat=3)))
def test_every_boundary_against_the_table(f64, median, fused):
    for mean, nb in itertools.product(MEANS, BARS):
        for n in (mean * nb, mean * nb + nb - 1):            # both ends of the tick counts with this integer mean
            assert plan(n, nb, f64, median, fused) == expected(n, nb, f64, median, fused), (n, nb, f64, median, fused)


def test_float32_rules_by_hand():
    nb = 1000
    kinds = lambda mean, median: (lambda p: (p["kind"], p["tile"], p["lanes"], p["nch"], p["long_min"]))(plan(mean * nb, nb, median=median))
    # with the median: lanes to 32, eight lanes per bar 33 .. 63, sixteen from 64
    assert kinds(32, True) == ("lanes", 1024, 0, 0, 64)
    assert kinds(33, True) == ("rows", 0, 8, 0, 128)
    assert kinds(63, True) == ("rows", 0, 8, 0, 128)
    assert kinds(64, True) == ("rows", 0, 16, 0, 256)
    assert kinds(65, True) == ("rows", 0, 16, 0, 256)
    # without: lanes to 56 (the large tile from 45), sixteen lanes per bar from 57
    assert kinds(44, False) == ("lanes", 1024, 0, 0, 64)
    assert kinds(45, False) == ("lanes", 2048, 0, 0, 64)
    assert kinds(56, False) == ("lanes", 2048, 0, 0, 64)
    assert kinds(57, False) == ("rows", 0, 16, 0, 256)
    for median in (False, True):
        assert kinds(210, median) == ("rows", 0, 16, 0, 256)
        assert kinds(211, median) == ("small", 0, 0, 10, 640)
        assert kinds(600, median) == ("small", 0, 0, 10, 640)
        assert kinds(601, median) == ("small", 0, 0, 21, 1344)
    # fewer than 64 bars: the wave-per-bar kernels whatever the mean
    for median in (False, True):
        for mean in (1, 33, 45, 64, 210):
            p63, p64 = plan(mean * 63, 63, median=median), plan(mean * 64, 64, median=median)
            assert (p63["kind"], p63["nch"], p63["long_min"], p63["grid"], p63["block"]) == ("small", 4, 256, 16, 256)
            assert p64["kind"] in ("lanes", "rows")


def test_float64_takes_the_wave_per_bar_kernels_only():
    for median, fused, nb in itertools.product((False, True), (False, True), (63, 64, 1000, 8 * 4096, 5000000)):
        for mean, nch, long_min in ((1, 4, 256), (33, 4, 256), (64, 4, 256), (210, 4, 256), (211, 10, 640), (600, 10, 640),
                                    (601, 21, 1344), (1200, 21, 1344)):
            p = plan(mean * nb, nb, f64=True, median=median, fused=fused)
            assert (p["kind"], p["nch"], p["long_min"], p["first_stage"], p["block"]) == ("small", nch, long_min, 0, 256)


def test_pipelined_step():
    mean = 1200
    for median in (False, True):
        nb = 8 * 4096 - 1                                       # first stage of 4095 bars: below the default minimum
        assert plan(mean * nb, nb, median=median, fused=True)["kind"] == "small"
        nb = 8 * 4096
        p = plan(mean * nb, nb, median=median, fused=True)
        assert p == dict(kind="pipelined", tile=0, lanes=0, nch=21, grid=1024, block=256, long_min=1344, first_stage=4096)
        assert plan(mean * nb, nb, median=median, fused=False)["kind"] == "small"        # close indices given: nothing to pipeline
        assert plan(600 * nb + nb - 1, nb, median=median, fused=True)["kind"] == "small"   # mean 600: the <= 640-tick kernel
        assert plan(601 * nb, nb, median=median, fused=True)["kind"] == "pipelined"
        # the first stage is a multiple of 256 bars
        nb = 833333
        assert plan(mean * nb, nb, median=median, fused=True)["first_stage"] == 104166 & ~255 == 103936
        # the developer knob: stages below 256 bars are never pipelined
        nb = 8 * 300
        assert plan(mean * nb, nb, median=median, fused=True, min_stage=255)["kind"] == "small"
        p = plan(mean * nb, nb, median=median, fused=True, min_stage=256)
        assert (p["kind"], p["first_stage"], p["grid"]) == ("pipelined", 256, 64)
        assert plan(mean * nb, nb, median=median, fused=True, min_stage=301)["kind"] == "small"
        assert plan(mean * nb, nb, median=median, fused=True, min_stage=300)["kind"] == "pipelined"


def test_grid_caps():
    big = 50_000_000
    assert plan(20 * big, big)["grid"] == N_CU * 96             # lane per bar
    assert plan(40 * big, big)["grid"] == N_CU * 32             # eight lanes per bar
    assert plan(100 * big, big)["grid"] == N_CU * 32            # sixteen lanes per bar
    assert plan(100 * big, big, f64=True)["grid"] == N_CU * 128
    assert plan(300 * big, big)["grid"] == N_CU * 96
    assert plan(1200 * big, big)["grid"] == N_CU * 64
    assert plan(1200 * big, big, fused=True)["grid"] == N_CU * 64          # first stage of 6 250 000 bars
    # ... and just below / at / above the cap of the 1-minute kernel: min(ceil(nb / 4), n_cu * 64)
    for nb, grid in ((4 * N_CU * 64 - 4, N_CU * 64 - 1), (4 * N_CU * 64 - 3, N_CU * 64), (4 * N_CU * 64 + 1, N_CU * 64)):
        assert plan(1200 * nb, nb)["grid"] == grid
    # uncapped: one workgroup per 4 bars / 4 x 4 bars / 4 x 8 bars / 2 x 64 bars
    assert plan(1200 * 1001, 1001)["grid"] == 251
    assert plan(100 * 1001, 1001)["grid"] == 63
    assert plan(40 * 1001, 1001)["grid"] == 32
    assert plan(20 * 1001, 1001)["grid"] == 8
    assert plan(1200 * 1001, 1001, n_cu=2)["grid"] == 128


def test_bad_arguments():
    for n, nb, n_cu in ((0, 1, 256), (10, 0, 256), (10, 1, 0)):
        with pytest.raises(ValueError):
            _ffi.ohlcv_plan(n, nb, n_cu=n_cu)
