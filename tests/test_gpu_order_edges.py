"""The windowed order statistics on the MI355X (csrc/fmk_order.hip) where tests/test_gpu_order.py does not reach: signed, zero,
subnormal and infinite values through every path (the recorded `signed.*`, `alt.*` and `hostile.*` cases), one planted element at
the slab and wave edges of a walk of three slabs, spans that are NaN altogether or up to one element or by half the sorted entries,
and the second trip of the grid-stride loops.  Every comparison is bit for bit; burst ratio, roc and pct_change also in the sign
of a zero (equal_bits)."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _order_ref as H
from tests.test_gpu_order import SLAB, SORT_WINDOW_MAX, SPAN_MAX, TILE, WALK_TILE, dev_call, equal, equal_bits
from tests.test_order_host import MANIFEST, VALUE_CLASS_CASES, case_input, expected, product

pytestmark = pytest.mark.gpu

LONG = 8500                          # a window of three slabs: 8499 + WALK_TILE = 8755 span elements


# ---------------------------------------------------------------------------------------------- value classes through every path
@pytest.mark.parametrize("name", VALUE_CLASS_CASES)
def test_value_classes_replay(name):
    c, ins = MANIFEST[name], case_input(name)
    eq = equal if c["fn"] == "stoch" else equal_bits             # %K: the sign of a zero is not the reference's to give
    want = expected(name)                                        # recorded, or the restatement whose hash is
    eq(H.call(c["fn"], ins, c["arg"], mod=product()), want, name + " (python)")
    eq(dev_call(c["fn"], ins, c["arg"]), want, name + " (_dev)")
    _counts.record(f"order/value_classes/{name}", outputs_compared=2 * c["n"], finite=c["finite"])


# ---------------------------------------------------------------------------------------------- one planted element
def _planted_positions(span):
    """Span positions of the first tile: the first and last lane of a wave group, both sides of each slab edge, the last element."""
    return (0, WALK_TILE - 1, WALK_TILE, SLAB - 1, SLAB, SLAB + WALK_TILE - 1, 2 * SLAB - 1, 2 * SLAB, span - 1)


@pytest.mark.parametrize("p", _planted_positions(LONG - 1 + WALK_TILE))
def test_stoch_k_sees_a_planted_low_in_exactly_its_windows(p):
    length, n = LONG, LONG - 1 + 2 * WALK_TILE
    close, low, high = np.full(n, 15.0), np.full(n, 10.0), np.full(n, 20.0)
    low[p] = 5.0
    t = np.arange(n)
    holds = (t >= p) & (t < p + length)
    closed = np.where(t < length - 1, np.nan, np.where(holds, (100.0 * (15.0 - 5.0)) / (20.0 - 5.0), (100.0 * (15.0 - 10.0)) / (20.0 - 10.0)))
    want = H.stoch_k(close, low, high, length)
    assert np.array_equal(want, closed, equal_nan=True) and 0 < holds[length - 1:].sum()
    equal(product().stoch_k(close, low, high, length), want, f"stoch, low planted at {p}")
    equal(product().stoch_k(close, -high, -low, length), H.stoch_k(close, -high, -low, length), f"stoch, high planted at {p}")
    _counts.record(f"order/planted/stoch_p{p}", outputs_compared=2 * n)


@pytest.mark.parametrize("p", _planted_positions(LONG + WALK_TILE))
def test_burst_ratio_bisection_sees_a_planted_median_in_exactly_its_windows(p):
    """Window 8501 over 1, 3, 1, 3, ... with one 2.0 put IN at p (the pattern goes on behind it): a window that holds it has 4250
    ones and 4250 threes around it and the median 2.0; any other has 4251 of what it starts with."""
    window, n = LONG + 1, LONG + 2 * WALK_TILE
    pattern = np.where(np.arange(n) % 2 == 0, 1.0, 3.0)
    x = np.concatenate([pattern[:p], [2.0], pattern[p:n - 1]])
    t = np.arange(n)
    holds = (t >= p) & (t < p + window)
    closed = np.where(t < window - 1, np.nan, np.where(holds, x / 2.0, 1.0))
    want = H.comp_burst_ratio(x, window)
    assert np.array_equal(want, closed, equal_nan=True) and 0 < holds[window - 1:].sum()
    equal_bits(product().comp_burst_ratio(x, window), want, f"burst, median planted at {p}")
    _counts.record(f"order/planted/burst_p{p}", outputs_compared=n)


# ---------------------------------------------------------------------------------------------- NaN-saturated spans, sorted path
def _saturated(window, how):
    """-> (x, tiles, m): a series of `tiles` full tiles of outputs and one of three.  Tile m's span [m * TILE, m * TILE + span) is
    made NaN as `how` says; m lies far enough behind tile 0 and before the last full tile that both are finite throughout (a
    window of 20 reaches back over one tile: m = 2 of 5; one of 3073 over three: m = 4 of 9).  how == "tail": the span of the
    partial tile is all NaN instead."""
    reach = -(-(window - 1) // TILE)                             # the tiles a window reaches back over
    span = window - 1 + TILE
    P = 1 << (span - 1).bit_length()                             # the entries sorted (BurstArgs.P)
    m = reach + 1
    tiles = reach + 1 if how == "tail" else m + reach + 2
    n = window - 1 + tiles * TILE + 3
    x = np.array(H.grid_walk(n, 720 + window))
    s0 = m * TILE
    if how == "all":
        x[s0:s0 + span] = np.nan
    elif how == "all_but_last":
        x[s0:s0 + span - 1] = np.nan
    elif how == "all_but_first":
        x[s0 + 1:s0 + span] = np.nan
    elif how == "tail":
        x[tiles * TILE:] = np.nan
    else:
        x[s0:s0 + P // 2 + int(how)] = np.nan                    # P/2 - 1, P/2, P/2 + 1 NaN entries
    return x, tiles, m


@pytest.mark.parametrize("how", ["all", "all_but_last", "all_but_first", "-1", "0", "1", "tail"])
@pytest.mark.parametrize("window", [20, SORT_WINDOW_MAX])
def test_burst_ratio_sorted_path_nan_saturated_span(window, how):
    x, tiles, m = _saturated(window, how)
    n = len(x)
    assert SPAN_MAX >= window - 1 + TILE
    want = H.comp_burst_ratio(x, window)
    first = want[window - 1:window - 1 + TILE]
    assert np.isfinite(first).all() and np.isnan(want[-3:]).all() == (how == "tail")
    if how != "tail":
        last = want[window - 1 + (tiles - 1) * TILE:window - 1 + tiles * TILE]
        middle = want[window - 1 + m * TILE:window - 1 + (m + 1) * TILE]
        assert np.isfinite(last).all() and np.isfinite(want[-3:]).all()
        assert np.isnan(middle).sum() >= (TILE if window > TILE or how.startswith("all") else TILE - 1)
    equal_bits(product().comp_burst_ratio(x, window), want, f"burst w={window}, span NaN: {how}")
    _counts.record(f"order/nan_saturated/w{window}_{how}", outputs_compared=n)


# ---------------------------------------------------------------------------------------------- a NaN at the ends of a long walk
# span positions of the first tile at window 8500 (slabs [0, 4096), [4096, 8192), [8192, 8755)): the last element of lane 100's
# window, which lies in its third slab; the first element of lane 100's window; the element that leaves with the first tile
NAN_AT = {"last_of_third_slab": 100 + LONG - 1, "first_of_first_slab": 100, "leaves_at_the_tile_edge": WALK_TILE - 1}


def _nan_outputs(n, window, p):
    t = np.arange(n)
    return (t < window - 1) | ((t >= p) & (t < p + window))


@pytest.mark.parametrize("where", sorted(NAN_AT))
def test_burst_ratio_bisection_one_nan_at_the_ends_of_three_slabs(where):
    window, n, p = LONG, LONG - 1 + 2 * WALK_TILE + 1, NAN_AT[where]
    x = np.array(H.signed_sizes(n, 730))
    x[p] = np.nan
    want = H.comp_burst_ratio(x, window)
    nan_by_window = _nan_outputs(n, window, p)
    assert np.isnan(want[nan_by_window]).all() and np.isfinite(want[~nan_by_window]).sum() > 50
    equal_bits(product().comp_burst_ratio(x, window), want, f"burst w={window}, NaN at {p}")
    _counts.record(f"order/nan_ends/burst_{where}", outputs_compared=n)


@pytest.mark.parametrize("column", ["low", "high"])
@pytest.mark.parametrize("where", sorted(NAN_AT))
def test_stoch_k_one_nan_at_the_ends_of_three_slabs(where, column):
    length, n, p = LONG, LONG - 1 + 2 * WALK_TILE + 1, NAN_AT[where]
    close, low, high = (np.array(a) for a in H.ohlc_walk(n, 731))
    (low if column == "low" else high)[p] = np.nan
    want = H.stoch_k(close, low, high, length)
    nan_by_window = _nan_outputs(n, length, p)
    assert np.isnan(want[nan_by_window]).all() and np.isfinite(want[~nan_by_window]).all() and (~nan_by_window).sum() > 50
    equal(product().stoch_k(close, low, high, length), want, f"stoch l={length}, NaN in {column} at {p}")
    _counts.record(f"order/nan_ends/stoch_{column}_{where}", outputs_compared=n)


# ---------------------------------------------------------------------------------------------- the second trip of the grid-stride loops
def _n_cu(ctx):
    from finmlkit_amd._ffi import c_i64
    v = c_i64()
    ctx.call("fmk_diag_n_cu", C.byref(v))
    return v.value


@pytest.fixture(scope="module")
def past_the_grid():
    """A series 257 elements longer than what the capped grid (n_cu * 16 blocks of 256) covers in one trip."""
    from finmlkit_amd import _ffi
    n_cu = _n_cu(_ffi.default_context())
    assert n_cu > 0
    one_trip = n_cu * 4096
    x = H.grid_walk(one_trip + 257, 740)
    x.setflags(write=False)
    return one_trip, x


def test_roc_and_pct_change_past_one_trip_of_the_grid(past_the_grid):
    one_trip, x = past_the_grid
    n = len(x)
    for lag in (1, one_trip + 1):
        for fn, ref in (("roc", H.roc), ("pct", H.pct_change)):
            want = ref(x, lag)
            assert np.isfinite(want[lag:]).all() and np.isnan(want[:lag]).all()
            equal_bits(dev_call(fn, x, lag, prefill=7.0), want, f"{fn} n={n} lag={lag}")
    _counts.record("order/second_trip/lagged", outputs_compared=4 * n)


def test_nan_head_past_one_trip_of_the_grid(past_the_grid):
    _, x = past_the_grid
    n = len(x)
    got = dev_call("burst", x, n + 1, prefill=7.0)
    assert got.shape == (n,) and np.isnan(got).all()
    got = dev_call("stoch", (x, x, x), n + 1, prefill=7.0)
    assert got.shape == (n,) and np.isnan(got).all()
    _counts.record("order/second_trip/nan_head", outputs_compared=2 * n)
