"""The recursive indicators on the MI355X where the state carried into a thread's eight elements is all there is: runs of bars without
a loss, a gain, a range or a term -- exact zeros, states that decay over whole tiles up to the step at which they leave the normal
range of float64 and beyond it -- inputs scaled by a power of two, and memories of several tiles (csrc/fmk_recur.hip on
csrc/fmk_recur_core.h).  tests/test_gpu_recur.py keeps away from all of these by construction.

Every call goes through the `_dev` entries with a prefilled output.  The expected values are the sequential restatement of
tests/_recur_ref.py, for the recorded cases runs.* after its hash has been found equal to the reference's (tests/golden/recur.json).
  a  exact zeros and NaN positions: no tolerance
  b  decaying runs inside the contract (0.9 x the horizon at the longest): every element compared
  c  runs of 1.3 x the steps to the smallest subnormal: compared over the record's `compare` ranges, counted and range-checked
     in between, where the reference stalls at the smallest subnormal and a composed a^len is 0.0
  d  inputs times 2^k: the same bits, times 2^k or unchanged
  e  windows of 3 to 10 tiles, spans up to 200 001
The tolerance of b, c and e is max(BOUND[fn], 16 x ref_dev): BOUND from tests/test_gpu_recur.py, ref_dev the restatement's own largest
deviation from the same recurrences in long double over the compared elements, recorded by tools/gen_recur_golden.py; x 16 because
which last bits differ moves with the data and the tile phase.  No figure here comes from a kernel's output.  The
largest deviation per function goes to the parity counts (recur_runs/max_deviation/*)."""
import numpy as np
import pytest

from tests import _counts
from tests import _recur_ref as H
from tests.test_gpu_recur import BOUND, RELATIVE, SENTINEL, close, dev_call, equal, seed_index
from tests.test_recur_host import MANIFEST, RUN_CASES, case_input, expected

pytestmark = pytest.mark.gpu

TILE = 2048                          # elements per workgroup of the scan's first and third launch (RC_TILE)
ITEMS = 8                            # consecutive elements per lane (RC_ITEMS)
AGG_UNIT = 256                       # tile aggregates per trip of the aggregate scan (RC_AGG_UNIT)
CEILING = {"ewma": 1e-9, "atr": 1e-9, "rsi": 1e-7, "adx": 1e-7}       # the contract's: relative / absolute on the 0-100 scale
WORST = {}


def tolerance(name):
    c = MANIFEST[name]
    tol = max(BOUND[c["fn"]], 16 * c["ref_dev"])
    assert tol * 10 <= CEILING[c["fn"]], (name, tol)
    return tol


def held(fn, got, want, mask, tol, what):
    """Over `mask`: NaN positions, exact zeros (of adx, and of ewma and atr, whose measure is relative) as the expected ones, every
    other element within tol in the measure of fn.  Nowhere a value the kernels did not write."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape == mask.shape, what
    assert not (got == SENTINEL).any(), (what, "unwritten", np.nonzero(got == SENTINEL)[0][:5])
    bad = np.nonzero(mask & (np.isnan(got) != np.isnan(want)))[0]
    assert len(bad) == 0, (what, "NaN positions", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    assert not np.isinf(got[mask]).any(), what
    if fn == "adx" or RELATIVE[fn]:
        bad = np.nonzero(mask & ((got == 0) != (want == 0)))[0]
        assert len(bad) == 0, (what, "zeros", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    ok = mask & ~np.isnan(want) & ((want != 0) if RELATIVE[fn] else True)
    if not ok.any():
        return
    dev = np.abs(got[ok] - want[ok])
    if RELATIVE[fn]:
        dev = dev / np.abs(want[ok])
    worst = float(dev.max())
    if worst > WORST.get(fn, (-1.0, ""))[0]:
        WORST[fn] = (worst, what)
        _counts.record(f"recur_runs/max_deviation/{fn}", value=repr(worst), relative=RELATIVE[fn], tolerance=repr(tol), case=what)
    print(f"deviation {fn} {what}: {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol, (what, worst, tol, int(np.nonzero(ok)[0][dev.argmax()]))


def first_series(make, ok, seed):
    """The first of the seeds seed, seed + 1, ... whose series has the property the test is about (a loss inside the first window,
    say); decided on the restatement before anything runs on the device."""
    for s in range(seed, seed + 40):
        ins = make(s)
        if ok(ins):
            return ins
    raise AssertionError("no series with the property")


# ---------------------------------------------------------------------------------------------- a. exact zeros, NaN positions
def change_points(seed):
    return (seed + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 7, 2 * TILE + 8)


@pytest.mark.parametrize("kind", ("rising", "falling"))
@pytest.mark.parametrize("w", (2, 14))
def test_rsi_without_a_loss_is_nan_and_without_a_gain_zero(w, kind):
    """No loss from bar 0 to p - 1 and the first one at p: NaN on [w, p), numbers from p.  No gain and the first at p: 0.0."""
    compared = 0
    for p in change_points(w):
        n = p + TILE + 9
        after = -7 if kind == "rising" else 7

        def ok(ins):
            want = H.rsi_wilder(ins[0], w)
            return (np.isnan(want[w:p]).all() if kind == "rising" else (want[w:p] == 0).all()) and np.isfinite(want[p:]).all()
        ins = first_series(lambda s: (H.run_series(kind, n, s, 0, p, after=after)[2],), ok, 1200 + p)
        want = H.rsi_wilder(ins[0], w)
        assert np.isnan(want[:w]).all() and want[p] > 0 and (kind == "falling" or want[p] < 100)
        got = dev_call("rsi", ins, [w], prefill=SENTINEL)
        equal(got[:p], want[:p], f"rsi w={w} {kind} to {p}: the head")
        close("rsi", got, want, f"rsi w={w} {kind} to {p}")
        compared += n
    _counts.record(f"recur_runs/exact/rsi_{kind}_w{w}", outputs_compared=compared)


@pytest.mark.parametrize("normalize", (False, True), ids=("plain", "normalize"))
@pytest.mark.parametrize("w", (3, 14))
def test_atr_ema_of_bars_without_a_range_is_zero(w, normalize):
    compared = 0
    for p in change_points(w - 1):
        n = p + TILE + 9
        ins = H.run_series("from_start", n, 1300 + p, 0, p, after=5)
        want = H.atr(*ins, w, True, normalize)
        assert np.isnan(want[:w - 1]).all() and (want[w - 1:p] == 0).all() and (want[p:] > 0).all() and np.isfinite(want[p:]).all()
        got = dev_call("atr", ins, [w, True, normalize], prefill=SENTINEL)
        equal(got[:p], want[:p], f"atr ema w={w} rangeless to {p}: the head")
        close("atr", got, want, f"atr ema w={w} norm={normalize} rangeless to {p}")
        compared += n
    _counts.record(f"recur_runs/exact/atr_w{w}_{int(normalize)}", outputs_compared=compared)


@pytest.mark.parametrize("span", (3, 27))
def test_ewma_of_zeros_is_zero(span):
    compared = 0
    for p in change_points(0):
        n = p + TILE + 9
        y = H.run_series("zeros", n, 1400 + p, 0, p)[2]
        want = H.ewma(y, span)
        assert (want[:p] == 0).all() and not np.signbit(want[:p]).any() and (want[p:] > 0).all()
        got = dev_call("ewma", (y,), [span], prefill=SENTINEL)
        equal(got[:p], want[:p], f"ewma span={span} zeros to {p}: the head")
        assert not np.signbit(got[:p]).any()
        close("ewma", got, want, f"ewma span={span} zeros to {p}")
        compared += n
    _counts.record(f"recur_runs/exact/ewma_s{span}", outputs_compared=compared)


@pytest.mark.parametrize("L", (3, 14))
def test_adx_of_bars_without_a_range(L):
    """Rangeless from bar 0 to p - 1, p inside the seed window of the sums, at its end, behind the seed of the last average and at a
    tile's edge: str_ > 0 and tot > 0 fail on exact zeros, not on NaN."""
    compared = 0
    for p in (L // 2 + 1, L + 1, 2 * L, TILE, TILE + 1):
        n = max(p, 2 * L - 1) + TILE + 9
        ins = H.run_series("from_start", n, 1500 + p, 0, p, after=5)
        want = H.adx_core(*ins, L)
        nz = np.nonzero(want)[0]
        assert len(nz) and nz[0] >= 2 * L - 1 and (p < 2 * L or nz[0] >= p) and np.isfinite(want).all()
        got = dev_call("adx", ins, [L], prefill=SENTINEL)
        assert np.array_equal(got == 0, want == 0), (L, p, np.nonzero((got == 0) != (want == 0))[0][:5])
        assert np.nonzero(got)[0][0] == nz[0]
        close("adx", got, want, f"adx L={L} rangeless to {p}")
        compared += n
    _counts.record(f"recur_runs/exact/adx_l{L}", outputs_compared=compared)


# ---------------------------------------------------------------------------------------------- b. decaying runs inside the contract
@pytest.mark.parametrize("name", [k for k in RUN_CASES if k.startswith("runs.b.")])
def test_decaying_run_inside_the_contract(name):
    c, ins = MANIFEST[name], case_input(name)
    assert c["left_out"] == 0 and c["compare"] == [[0, c["n"]]]
    got = dev_call(c["fn"], ins, c["args"], prefill=SENTINEL)
    held(c["fn"], got, expected(name), np.ones(c["n"], bool), tolerance(name), name)
    _counts.record(f"recur_runs/{name}", outputs_compared=c["n"])


@pytest.mark.parametrize("fn,args", [("rsi", [14]), ("atr", [14, True, False])], ids=("rsi", "atr_ema"))
def test_flat_run_across_the_trips_of_the_aggregate_scan(fn, args):
    """The run begins 50 bars in front of the last tile of the aggregate scan's first trip and ends in the second tile of the next: the
    decayed state crosses with the carried map.  Against the restatement within BOUND alone."""
    n = AGG_UNIT * TILE + 3 * TILE
    start, length = (AGG_UNIT - 1) * TILE - 50, 2 * TILE + 100
    assert start + length > (AGG_UNIT + 1) * TILE and length < 0.9 * H.horizon(13 / 14)
    h, lo, c = H.run_series("flat", n, 1600, start, length, step=5)          # (small moves: half a million bars stay off the floor)
    ins = (c,) if fn == "rsi" else (h, lo, c)
    want = H.call(fn, ins, args)
    assert np.isfinite(want[seed_index(fn, args):]).all()
    if fn == "rsi":
        assert len(set(want[start + 100:start + length])) < 40 and 0 < want[start + length - 1] < 100      # a plateau
    else:
        assert 0 < want[start + length - 1] < 1e-130
    close(fn, dev_call(fn, ins, args, prefill=SENTINEL), want, f"{fn} {args} n={n} (flat run across the trips)")
    _counts.record(f"recur_runs/trips/{fn}", outputs_compared=n)


# ---------------------------------------------------------------------------------------------- c. past the horizon
@pytest.mark.parametrize("name", [k for k in RUN_CASES if k.startswith("runs.c.")])
def test_run_past_the_horizon(name):
    c, ins = MANIFEST[name], case_input(name)
    fn, n = c["fn"], c["n"]
    mask = H.ranges_mask(c["compare"], n)
    assert int((~mask).sum()) == c["left_out"] and 0 < c["left_out"] < 0.35 * n and len(c["compare"]) == 2
    got = dev_call(fn, ins, c["args"], prefill=SENTINEL)
    held(fn, got, expected(name), mask, tolerance(name), name)
    between = got[~mask]
    if fn in ("rsi", "adx"):
        assert (np.isnan(between) | ((between >= 0) & (between <= 100))).all(), name
    else:
        last = got[c["compare"][0][1] - 1]                             # the last compared value in front of what is left out
        assert np.isfinite(between).all() and (between >= 0).all() and (between <= last).all() and last > 0, name
    _counts.record(f"recur_runs/{name}", outputs_compared=n - c["left_out"], left_out=c["left_out"])


# ---------------------------------------------------------------------------------------------- d. scaling by a power of two
@pytest.fixture(scope="module")
def unscaled():
    n = 2 * TILE + 9
    h, lo, c = H.hlc_walk(n, 1700)
    for a in (h, lo, c):
        a.setflags(write=False)
    return h, lo, c


SCALED = [("ewma", [w]) for w in (3, 14)] + [("atr", [w, True, False]) for w in (3, 14)] + [("atr", [w, False, False]) for w in (3, 14)] + \
    [("tr", [])]
UNCHANGED = [("rsi", [w]) for w in (3, 14)] + [("adx", [w]) for w in (3, 14)] + [("atr", [w, True, True]) for w in (3, 14)] + \
    [("atr", [w, False, True]) for w in (3, 14)]


@pytest.mark.parametrize("fn,args", SCALED + UNCHANGED, ids=lambda v: v if isinstance(v, str) else "-".join(str(a) for a in v))
def test_scaling_by_a_power_of_two(unscaled, fn, args):
    """No absolute constant, no underflow: every rounding commutes with 2^k, in the composed maps as in the steps."""
    ins = unscaled[2:] if fn in ("ewma", "rsi") else unscaled
    base = dev_call(fn, ins, args, prefill=SENTINEL)
    close(fn, base, H.call(fn, ins, args), f"{fn} {args} (unscaled)", fn == "tr" or (fn == "atr" and not args[1]))
    for k in (-40, 40):
        f = 2.0 ** k
        got = dev_call(fn, tuple(a * f for a in ins), args, prefill=SENTINEL)
        equal(got, base * f if (fn, args) in SCALED else base, f"{fn} {args} x 2^{k}")
    _counts.record(f"recur_runs/scaled/{fn}_{'_'.join(str(a) for a in args)}", outputs_compared=3 * len(base))


# ---------------------------------------------------------------------------------------------- e. long memories
@pytest.mark.parametrize("name", [k for k in RUN_CASES if k.startswith("runs.e.")])
def test_long_memory(name):
    """Seed sums over 3 to 10 tiles (many 256-element rounds of the seed loop), a within 1e-5 of 1."""
    c, ins = MANIFEST[name], case_input(name)
    fn, args, n = c["fn"], c["args"], c["n"]
    seed = seed_index(fn, args)
    assert c["left_out"] == 0 and n == (4 * TILE + 9 if fn == "ewma" else seed + TILE + 9)
    want = expected(name)
    assert np.isfinite(want[seed:]).all() and (want[seed:] > 0).all()
    got = dev_call(fn, ins, args, prefill=SENTINEL)
    equal(got[:seed], want[:seed], name + ": before the seed")
    held(fn, got, want, np.ones(n, bool), tolerance(name), name)
    _counts.record(f"recur_runs/{name}", outputs_compared=n)
