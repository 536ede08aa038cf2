"""The running-sum indicators on the MI355X (csrc/fmk_runsum.hip) on zero-volume bars among volumes that are not exactly summable,
where tests/test_gpu_runsum.py does not reach (its zero bars are all on integer volumes, whose sums are exact in any order), and
two loops of the kernels that no earlier test sends round a second time.

The reference differences sequential prefix sums, and adding 0.0 changes no bit of one: over zero-volume bars its recent and past
sums of comp_flow_acceleration and the three window sums of vpin are exactly 0.0, and its outputs there are
log(1e-12 / (past + 1e-12)), log((recent + 1e-12) / 1e-12) and NaN.  The scan adds the state that enters a thread's eight elements
in another order, so two of its prefix sums can differ in the last bits with nothing but zeros between them: the kernels decide
those windows by an exact count of non-zero terms, as long as the prefix sum is a number: behind a NaN volume every prefix sum of the
reference is NaN and so is every output, on windows of zero bars too (test_flow_behind_a_nan_on_zero_volume_bars).  Asked here: every NaN and infinity where the restatement has one and nowhere
else, and the deviations within the BOUND of tests/test_gpu_runsum.py, unchanged (zero_lot_volumes has a floor of 1.01, so a
window sum that is not zero is at least 1.01 against prefix noise of about 3e-11).

vwap_distance slides its sums, so on an all-zero window of such volumes the reference's own vsum is a residue of either sign: it
holds, computes or takes the log of a negative number by chance (tests/test_runsum_host.py).  Those outputs are left out (at most
1 % of a case, asserted); off them the NaN positions agree exactly and the values stay within BOUND["vwap"].

Every comparison goes through check() of tests/test_gpu_runsum.py; the largest deviation per function over this file's cases and
the outputs compared and left out are recorded (DESIGN.md 7f holds the figures).  Measured on the MI355X: flow 4.0e-11 (one zero
run at 255, [20, 1]), vwap 1.2e-12 (the runs of MANY, log mode), boll a scaled factor of 88.2 (526 345 elements), vpin no element
off as float32.  On the library without the counts both flow tests on zero bars, four of the six single runs, both vpin tests and
the two recorded flow cases failed: NaN for a number, a number for NaN, outputs off by 2.1 to 2.4."""
import numpy as np
import pytest

from tests import _counts
from tests import _runsum_ref as H
from tests.test_gpu_runsum import AGG_UNIT, BOUND, ITEMS, THREADS, TILE, _summable, check, dev_call
from tests.test_runsum_host import FLOW_ARGS, MANY, ZERO_SHARE, flow_windows_of_zero_bars, product

pytestmark = pytest.mark.gpu

N = 3 * TILE + 300
WORST = {}


def measured(fn, dev, what):
    """The largest deviation check() measured, per function, over the cases of this file."""
    if dev is not None and dev > WORST.get(fn, (-1.0, ""))[0]:
        WORST[fn] = (dev, what)
        _counts.record(f"runsum_zeros/max_deviation/{fn}", value=repr(dev), bound=repr(BOUND[fn]), case=what)


def both_ways(fn, ins, args, what, leave_out=None):
    """Through the `_dev` entry on a prefilled output and through the Python function."""
    for got, how in ((dev_call(fn, ins, args), "_dev"), (H.call(fn, ins, args, mod=product()), "python")):
        measured(fn, check(fn, got, ins, args, f"{what} ({how})", leave_out=leave_out), what)


# ---------------------------------------------------------------------------------------------- comp_flow_acceleration
@pytest.mark.parametrize("seed", (802, 818))
def test_flow_on_zero_volume_bars(seed):
    """30 % zero bars and the runs of MANY: hundreds of windows whose recent or past part is all zero at every phase of a thread's
    eight elements.  A sum there that is rounding noise instead of 0.0 shows as a NaN (the log of a negative number) or as an output
    that is off by far more than the bound."""
    v = H.zero_lot_volumes(N, seed, MANY)
    zero_recent = 0
    for w, r in FLOW_ARGS:
        want = H.comp_flow_acceleration(v, w, r)
        assert np.isfinite(want[w - 1:]).all()
        both_ways("flow", (v,), [w, r], f"flow zero bars seed={seed} [{w}, {r}]")
        zero_recent += int(H.zero_windows(v, r)[w - 1:].sum()) if r else 0
    assert zero_recent > 2000
    _counts.record(f"runsum_zeros/flow/seed{seed}", outputs_compared=2 * N * len(FLOW_ARGS), zero_recent_windows=2 * zero_recent)


@pytest.mark.parametrize("k", (1, 32, 255, 256, 257, 512))
def test_flow_with_one_zero_run_over_an_edge(k):
    """No zero bar but one run of recent_periods + 3 that begins at the last element of a thread: over a thread's edge (k = 1), a
    wave's (32: lane 32), the last thread of a tile and the first of the next (255, 256, 257) and the second tile edge (512).  The
    recent part lies on both sides of the edge and all of it behind it.  With [3, 1] the run of 4 lies behind the first output for
    k = 1 as well (with a window of 20 it lies in front of it), and two of its windows are zero bars in both parts: 0.0."""
    seen = 0
    for w, r in ((20, 1), (20, 5), (3, 1)):
        start = ITEMS * k - 1
        v = H.zero_lot_volumes(N, 802, [[start, r + 3]], share=0)
        assert (v == 0.0).sum() == r + 3 and start + r + 3 < N
        zero = H.zero_windows(v, r)
        assert zero.sum() == 4 and zero[start + r - 1] and zero[start + r + 2]
        zero &= np.arange(N) >= w - 1
        assert w != 3 or zero.sum() == 4
        both = flow_windows_of_zero_bars(v, w, r)
        assert both.sum() == (2 if w == 3 else 0) and not (both & ~zero).any()
        want = H.comp_flow_acceleration(v, w, r)
        assert np.isfinite(want[w - 1:]).all()
        assert (want[zero & ~both] < -25.0).all() and (want[both] == 0.0).all()       # log(1e-12 / past), log(1e-12 / 1e-12)
        both_ways("flow", (v,), [w, r], f"flow one zero run at {start} [{w}, {r}]")
        seen += int(zero.sum())
    _counts.record(f"runsum_zeros/flow_edge/k{k}", outputs_compared=6 * N, zero_recent_windows=2 * seen)


@pytest.mark.parametrize("at", (5, TILE - 1, TILE))
def test_flow_behind_a_nan_on_zero_volume_bars(at):
    """A NaN volume in a thread's sixth element, in the last element of a tile and in the first of the next, in front of the 30 %
    zero bars and the runs of MANY: every prefix sum behind it is NaN in the reference and so is every output, on windows whose
    bars are all zero as well (NaN - NaN), where the count of non-zero terms alone would say 0.0 and 0.0: log(1) = 0.0.  NaN
    positions are compared exactly; in front of the NaN the outputs are those of the clean series."""
    v = H.zero_lot_volumes(N, 802, MANY)
    v[at] = np.nan
    zero_windows = 0
    for w, r in ((1, 0), (20, 1), (20, 5)):
        want = H.comp_flow_acceleration(v, w, r)
        first = max(at, w - 1)
        assert np.isnan(want[first:]).all() and np.isfinite(want[w - 1:at]).all()
        zero = flow_windows_of_zero_bars(v, w, r)
        zero[:first] = False
        assert zero.sum() >= 10, (w, r, int(zero.sum()))
        both_ways("flow", (v,), [w, r], f"flow NaN at {at} in front of zero bars [{w}, {r}]")
        zero_windows += int(zero.sum())
    _counts.record(f"runsum_zeros/flow_nan/at{at}", outputs_compared=2 * 3 * N, zero_windows_behind_the_nan=2 * zero_windows)


# ---------------------------------------------------------------------------------------------- vpin
@pytest.mark.parametrize("share,windows", [(0, (1, 2, 20)), (0.3, (1,))], ids=("runs", "scattered"))
def test_vpin_on_zero_volume_bars_at_large_totals(share, windows):
    """Volumes x 1024: the totals reach 1.5e8, a unit in their last place is 3e-8 and above the reference's `tot > 1e-9`, so a
    window of zero bars whose total is noise gets a number where the reference has NaN.  The same runs in both series; with 30 %
    zeros in each, independently, every eleventh bar is zero in both (window 1)."""
    b, s = H.zero_lot_kilo(N, 802, MANY, share), H.zero_lot_kilo(N, 803, MANY, share)
    zero_windows = 0
    for w in windows:
        zero = H.zero_windows(b, w) & H.zero_windows(s, w)
        want = H.vpin(b, s, w)
        assert zero.sum() >= 50 and np.array_equal(np.isnan(want[w - 1:]), zero[w - 1:])
        both_ways("vpin", (b, s), [w], f"vpin zero bars x1024 share={share} [{w}]")
        zero_windows += int(zero.sum())
    _counts.record(f"runsum_zeros/vpin/share{share}", outputs_compared=2 * N * len(windows), zero_windows=2 * zero_windows)


# ---------------------------------------------------------------------------------------------- vwap_distance
VWAP_RUNS = {"ends_at_edge_1": [[TILE - 40, 40]], "straddles_edge_1": [[TILE - 30, 60]], "begins_at_edge_1": [[TILE, 40]],
             "straddles_edge_2": [[2 * TILE - 30, 60]], "many": MANY}


@pytest.mark.parametrize("name", sorted(VWAP_RUNS))
def test_vwap_on_volumes_that_are_not_summable_with_zero_bars(name):
    """Zero bars shorter than the window everywhere (30 %) and runs longer than it at the tile edges: off the all-zero windows
    vsum is at least 1.01, every output is a number within the bound and none is held; on them nothing is asked."""
    w = 20
    c, v = H.grid_walk(N, 801), H.zero_lot_volumes(N, 802, VWAP_RUNS[name])
    out = H.zero_windows(v, w)
    assert 0 < out.sum() <= ZERO_SHARE * (N - (w - 1)), (name, int(out.sum()))
    for lg in (False, True):
        want, held = H.vwap_distance(c, v, w, lg, sums=True)
        assert np.isfinite(want[w - 1:][~out[w - 1:]]).all() and not held[~out].any()
        both_ways("vwap", (c, v), [w, lg], f"vwap zero bars {name} log={lg}", leave_out=out)
    _counts.record(f"runsum_zeros/vwap/{name}", outputs_compared=4 * (N - int(out.sum())), left_out=4 * int(out.sum()),
                   left_out_share=repr(float(out.sum()) / (N - (w - 1))))


@pytest.mark.parametrize("name,runs,finite", [("a_value_from_tile_0", [[TILE - 25, 257 * TILE + 60]], 530_422),
                                              ("nan_from_element_0", [[0, 257 * TILE + 100]], 4005)])
def test_the_hold_looks_back_over_more_than_one_trip(name, runs, finite):
    """k_rs_hold walks the tile records 256 at a time.  259 tiles, 257 of them without a value, on exactly summable inputs (bit for
    bit): tiles 257 and 258 find the value of tile 0 in the loop's second pass, and with zeros from element 0 the loop runs out of
    records (NaN is carried)."""
    n, w = 259 * TILE + 9, 20
    assert 257 > THREADS
    c, v = H.grid64_walk(n, 804), H.int_volumes(n, 805, runs)
    assert _summable(c) and _summable(v)
    for lg in (False, True):
        want, held = H.vwap_distance(c, v, w, lg, sums=True)
        assert np.isfinite(want).sum() == finite and np.isnan(want).sum() == n - finite
        start, length = runs[0]
        assert held[max(start + w - 1, w - 1):start + length].all() and not held[start + length]
        if start:
            assert (want[start + w - 1:start + length] == want[start + w - 2]).all() and np.isfinite(want[start + w - 2])
        else:
            assert np.isnan(want[:length]).all()
        check("vwap", dev_call("vwap", (c, v), [w, lg]), (c, v), [w, lg], f"vwap hold {name} log={lg}")      # bit for bit
    _counts.record(f"runsum_zeros/hold/{name}", outputs_compared=2 * n, held=int(held.sum()))


# ---------------------------------------------------------------------------------------------- bollinger_percent_b
def test_bollinger_across_the_second_trip_of_the_aggregate_scan():
    """tests/test_gpu_runsum.py sends vwap_distance and vpin over more than 256 tiles; the sum of squares, which is the channel that
    cancels, had not been carried across trips."""
    n, args = AGG_UNIT * TILE + TILE + 9, [20, 2.0]
    assert n == 526_345
    c = H.grid_walk(n, 807, 5)
    assert c.min() > 10.0 and not H.flat_windows(c, args[0]).any()
    got = dev_call("boll", (c,), args)
    assert np.isnan(got[:19]).all() and np.isfinite(got[19:]).all()
    measured("boll", check("boll", got, (c,), args, f"boll {args} n={n} (second trip)"), f"boll {args} n={n} (second trip)")
    _counts.record("runsum_zeros/second_trip/boll", outputs_compared=n)
