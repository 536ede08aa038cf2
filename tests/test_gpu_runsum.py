"""The running-sum indicators on the MI355X -- bollinger_percent_b, vwap_distance, comp_flow_acceleration, vpin, parkinson_range
(csrc/fmk_runsum.hip) -- against the reference's recorded outputs (tests/golden/runsum.npz) and the sequential restatement of
tests/_runsum_ref.py.

Bit for bit (np.array_equal, equal_nan=True): parkinson_range, every output before a seed index, every NaN position, which
vwap_distance outputs are held (a held output has the bits of the one before it), and every output on exactly summable inputs
(prices on a 1/64 grid, integer volumes below 64).  Otherwise within BOUND, because the sum that enters a thread's eight elements is
added in another order:
  vwap, flow  the absolute deviation;
  vpin        equal as float32, but for one float32 unit in the last place where the restatement's float64 quotient lies within
              BOUND["vpin"] (relative) of the boundary between the two float32 values; such elements are counted and reported;
  boll        |got - want| <= BOUND * 2^-52 * kappa * (1 + |want - 0.5|) per element with kappa = sumsq / ((window - 1) * var) from
              the restatement's own sums: the variance cancels.  A window whose elements are all equal has a true variance of zero,
              the reference's NaN-or-number there is rounding noise: such windows are left out (at most 2 % of a case, asserted),
              off them the NaN positions agree exactly.
vwap_distance on a window of all-zero volumes that are not exactly summable is the reference's own sliding-sum residue: a caller
that has such windows hands check() their mask (leave_out), and nothing is asked of them (tests/test_gpu_runsum_zeros.py).
BOUND is the largest figure measured on the MI355X over every case of this file x 16, rounded up to a power of ten (DESIGN.md 7f
holds the figures).  Every comparison goes through check(), which keeps the largest deviation per function and reports it with the
parity counts.  The inputs hold no infinities: they are outside the contract."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _runsum_ref as H
from tests.test_runsum_host import FLAT_SHARE, MANIFEST, OK_CASES, REFUSED, case_input, exactly_summable, expected, product, same_bits

pytestmark = pytest.mark.gpu

THREADS = 256                        # lanes per workgroup (csrc/fmk_recur_core.h: RC_THREADS)
ITEMS = 8                            # consecutive elements per lane (RC_ITEMS)
TILE = THREADS * ITEMS               # elements per workgroup of the scan's first and third launch (RC_TILE)
AGG_UNIT = 256                       # tile aggregates per trip of the aggregate scan (RC_AGG_UNIT)
ENTRY = {"boll": "fmk_bollinger_percent_b", "vwap": "fmk_vwap_distance", "flow": "fmk_flow_acceleration", "vpin": "fmk_vpin",
         "park": "fmk_parkinson_range"}
WINDOWS = (1, 2, 3, 20, 100)
# measured on the MI355X over all cases below, each x 16 and rounded up to a power of ten:
#   vwap 1.6e-12 absolute (vwap [1, True] n=2047; 1.2e-13 at n = 526 345), flow 5.5e-11 absolute (flow [2, 1] n=4098: one bar's
#   volume as the difference of two prefix sums of about 1e5), boll a scaled factor of 9.4 (boll [20, 2.0] n=4116), vpin 8.2e-12
#   relative distance of the float64 quotient from the float32 boundary (vpin [32] n=526345: 13 of 526 314 elements one float32
#   unit off; none in any other case)
BOUND = {"vwap": 1e-10, "flow": 1e-9, "boll": 1000.0, "vpin": 1e-9}
SENTINEL = 12345.678
WORST = {}
FLIPS = {"elements": 0, "compared": 0}


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert np.array_equal(got, want, equal_nan=True), (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def _measured(fn, worst, what, at):
    if worst > WORST.get(fn, (-1.0, ""))[0]:
        WORST[fn] = (worst, what)
        _counts.record(f"runsum/max_deviation/{fn}", value=repr(worst), bound=repr(BOUND[fn]), case=what)
    print(f"deviation {fn} {what}: {worst:.3e}")
    assert worst <= BOUND[fn], (what, worst, BOUND[fn], at)
    return worst


def check(fn, got, ins, args, what, want=None, leave_out=None):
    """`got` against the restatement on `ins` (and against `want`, a recorded output, which the restatement must equal): see the
    module's docstring.  Inputs that are exactly summable, and parkinson_range, are compared bit for bit.  leave_out: a mask of
    outputs that are the reference's own rounding noise (vwap_distance on all-zero windows of volumes that are not exactly
    summable): nothing is asked of them.  Returns the largest deviation where one is measured."""
    got = np.asarray(got)
    exact = fn == "park" or all(_summable(a) for a in ins)
    if fn == "boll":
        own, sq, var = H.bollinger_percent_b(*ins, *args, sums=True)
    elif fn == "vwap":
        own, held = H.vwap_distance(*ins, *args, sums=True)
    elif fn == "vpin":
        own, quot = H.vpin(*ins, *args, sums=True)
    else:
        own = H.call(fn, ins, args)
    if want is not None:
        assert same_bits(own, want), what
    if exact or (fn == "boll" and args[0] == 1):                    # (window 1: NaN everywhere)
        assert leave_out is None, (what, "every output is compared bit for bit: nothing can be left out")
        return equal(got, own, what)
    assert got.dtype == own.dtype and got.shape == own.shape, what
    keep = np.ones(len(own), bool) if leave_out is None else ~np.asarray(leave_out, bool)
    assert leave_out is None or fn == "vwap", what
    if fn == "boll":
        flat = H.flat_windows(ins[0], args[0])
        assert flat.sum() <= FLAT_SHARE * max(len(own) - (args[0] - 1), 1), (what, int(flat.sum()))
        keep = ~flat
    bad = np.nonzero((np.isnan(got) != np.isnan(own)) & keep)[0]
    assert len(bad) == 0, (what, "NaN positions", len(bad), bad[:5], got[bad[:3]], own[bad[:3]])
    bad = np.nonzero((np.isinf(got) | np.isinf(own)) & keep & (got != own))[0]
    assert len(bad) == 0, (what, "infinities", len(bad), bad[:5])
    ok = np.isfinite(own) & keep
    if fn == "vwap":
        at = np.nonzero(held & keep)[0]
        at = at[at > 0]
        assert same_bits(got[at], got[at - 1]), (what, "held outputs")
    if not ok.any():
        return
    idx = np.nonzero(ok)[0]
    if fn == "vpin":
        off = idx[got[idx] != own[idx]]
        FLIPS["compared"] += len(idx)
        if len(off) == 0:
            return
        g, o = got[off], own[off]
        assert ((np.nextafter(o, np.float32(np.inf)) == g) | (np.nextafter(o, np.float32(-np.inf)) == g)).all(), (what, off[:5], g[:3], o[:3])
        edge = (g.astype(np.float64) + o.astype(np.float64)) / 2.0          # the boundary between the two float32 values
        dist = np.abs(quot[off] - edge) / np.abs(edge)
        FLIPS["elements"] += len(off)
        _counts.record("runsum/vpin_one_unit_off", elements=FLIPS["elements"], compared=FLIPS["compared"])
        print(f"vpin {what}: {len(off)} of {len(idx)} one float32 unit off")
        return _measured(fn, float(dist.max()), what, int(off[dist.argmax()]))
    dev = np.abs(got[idx] - own[idx])
    if fn == "boll":
        with np.errstate(all="ignore"):
            kappa = sq[idx] / ((args[0] - 1) * var[idx])
        assert (kappa > 0).all() and np.isfinite(kappa).all(), what
        dev = dev / (2.0 ** -52 * kappa * (1.0 + np.abs(own[idx] - 0.5)))
    return _measured(fn, float(dev.max()), what, int(idx[dev.argmax()]))


def _summable(a):
    """On the 1/64 grid below 1024 (prices) or integers below 64 (volumes), NaN aside: every product and sum is exact."""
    a = np.asarray(a, np.float64)
    a = a[~np.isnan(a)]
    return bool(((a * 64 == np.round(a * 64)) & (np.abs(a) < 1024)).all())


def c_args(fn, args):
    if fn == "boll":
        return (C.c_int64(int(args[0])), C.c_double(float(args[1])))
    if fn == "vwap":
        return (C.c_int64(int(args[0])), C.c_int(bool(args[1])))
    return tuple(C.c_int64(int(a)) for a in args)


def dev_call(fn, inputs, args, ctx=None, prefill=SENTINEL, resident=None):
    """The `_dev` entry of `fn` on resident copies of the inputs -> host array.  prefill: what the output buffer holds before the
    call: an element the kernels do not write shows.  resident: DeviceArrays (or views) to use instead of uploading."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = ctx or _ffi.default_context()
    n = len(inputs[0]) if resident is None else resident[0].n
    dev = resident or [DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=np.float64)) for a in inputs]
    dtype = np.float32 if fn == "vpin" else np.float64
    out = DeviceArray.from_host(ctx, np.full(n, prefill, dtype))
    ctx.call(ENTRY[fn] + "_dev", *(d.p for d in dev), C.c_int64(n), *c_args(fn, args), out.p)
    got = out.to_host()
    assert not (got == dtype(prefill)).any(), (fn, args, n, "an element was left unwritten")
    return got


def first_output(fn, args):
    """The first index whose output carries a value."""
    return 0 if fn == "park" else max(args[0] - 1, 0)


@pytest.fixture(scope="module")
def series():
    """One 6444-element set of series, shared by the tests below (never written to), resident as well: a cent-grid walk, lot
    volumes (two of them), and the exactly summable pair: a 1/64-grid walk and integer volumes."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    n = 3 * TILE + 300
    made = {"cent": H.grid_walk(n, 801), "lot": H.lot_volumes(n, 802), "lot2": H.lot_volumes(n, 803), "g64": H.grid64_walk(n, 804),
            "int": H.int_volumes(n, 805), "int2": H.int_volumes(n, 806)}
    assert n == 6444 and all(np.isfinite(a).all() for a in made.values())
    assert _summable(made["g64"]) and _summable(made["int"]) and not _summable(made["cent"]) and not _summable(made["lot"])
    for a in made.values():
        a.setflags(write=False)
    ctx = _ffi.default_context()
    return made, {k: DeviceArray.from_host(ctx, a) for k, a in made.items()}


COLUMNS = {"boll": ("cent",), "vwap": ("cent", "lot"), "flow": ("lot",), "vpin": ("lot", "lot2"), "park": ("cent", "lot")}
EXACT_COLUMNS = {"boll": ("g64",), "vwap": ("g64", "int"), "flow": ("int",), "vpin": ("int", "int2")}


def inputs_of(fn, made, n, columns=COLUMNS):
    """The last n elements of the shared series: another phase of the series at every size."""
    return tuple(made[k][len(made[k]) - n:] for k in columns[fn])


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay(name):
    c, ins = MANIFEST[name], case_input(name)
    fn, args = c["fn"], c["args"]
    assert exactly_summable(name) <= all(_summable(a) for a in ins)
    # vwap_distance on all-zero windows of volumes that are not exactly summable: the reference's own residue, left out
    out = H.zero_windows(ins[1], args[0]) if fn == "vwap" and name.startswith("zerolot.") else None
    assert out is None or (0 < out.sum() == c["zero_windows"] and not _summable(ins[1]))
    check(fn, H.call(fn, ins, args, mod=product()), ins, args, name + " (python)", want=expected(name), leave_out=out)
    if c["n"]:
        check(fn, dev_call(fn, ins, args), ins, args, name + " (_dev)", want=expected(name), leave_out=out)
    left = 0 if out is None else 2 * int(out.sum())
    _counts.record(f"runsum/fixture/{name}", outputs_compared=2 * c["n"] - left, finite=c["finite"], left_out=left)


@pytest.mark.parametrize("name", [k for k in REFUSED if "unequal" not in k])
def test_refused_arguments_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    c, ins = MANIFEST[name], case_input(name)
    fn, args = c["fn"], c["args"]
    ctx, lib = _ffi.default_context(), _ffi.lib()
    with pytest.raises(ValueError) as e:
        dev_call(fn, ins, args)
    assert c["message"] in str(e.value)
    n = len(ins[0])
    out = np.zeros(n, np.float32 if fn == "vpin" else np.float64)
    rc = getattr(lib, ENTRY[fn])(ctx.handle, *(_ffi.ptr(a) for a in ins), C.c_int64(n), *c_args(fn, args), _ffi.ptr(out))
    assert rc == _ffi.E_ARG
    rc = getattr(lib, ENTRY[fn] + "_dev")(ctx.handle, *(None for _ in ins), C.c_int64(n), *c_args(fn, args), None)
    assert rc == _ffi.E_ARG                      # refused before any pointer is looked at


def test_a_series_of_two_to_the_31_is_refused():
    from finmlkit_amd import _ffi
    ctx, lib = _ffi.default_context(), _ffi.lib()
    for fn, args in (("boll", [5, 2.0]), ("vwap", [5, False]), ("flow", [5, 2]), ("vpin", [5]), ("park", [])):
        for entry in (ENTRY[fn] + "_dev", ENTRY[fn]):      # the host-pointer flavour too: nothing is uploaded first
            rc = getattr(lib, entry)(ctx.handle, *(None for _ in range(H.N_INPUTS[fn])), C.c_int64(1 << 31), *c_args(fn, args), None)
            assert rc == _ffi.E_ARG, entry


# ---------------------------------------------------------------------------------------------- geometry
GEOMETRY = [("boll", [w, 2.0]) for w in WINDOWS] + [("vwap", [w, lg]) for w in WINDOWS for lg in (False, True)] + \
    [("flow", [w, r]) for w, r in ((1, 0), (2, 1), (3, 0), (20, 5), (100, 99))] + [("vpin", [w]) for w in WINDOWS]


def ident(v):
    return v if isinstance(v, str) else "-".join(str(a) for a in v)


@pytest.mark.parametrize("fn,args", GEOMETRY, ids=ident)
def test_geometry(series, fn, args):
    """Lengths seed + m around the lane's eight elements and the tile, through the Python functions on the last n elements of one
    series (the lagged read crosses a tile edge from the second tile on); and lengths below the seed: all NaN."""
    made, _ = series
    seed = first_output(fn, args)
    lengths = sorted({seed + m for m in (0, 1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)} | {max(seed - 1, 1), max(seed // 2, 1)})
    compared = 0
    for n in lengths:
        for columns in (COLUMNS, EXACT_COLUMNS):
            ins = inputs_of(fn, made, n, columns)
            got = H.call(fn, ins, args, mod=product())
            if n <= seed:
                assert np.isnan(got).all()
            check(fn, got, ins, args, f"{fn} {args} n={n}")
            compared += n
    _counts.record(f"runsum/geometry/{fn}_{'_'.join(str(a) for a in args)}", outputs_compared=compared)


@pytest.mark.parametrize("fn,args", [("boll", [TILE, 2.0]), ("boll", [TILE + 1, 2.0]), ("vwap", [TILE, True]), ("vwap", [TILE + 1, True]),
                                     ("flow", [TILE, 5]), ("flow", [TILE + 1, TILE]), ("vpin", [TILE]), ("vpin", [TILE + 1])], ids=ident)
def test_seed_at_a_tile_edge(series, fn, args):
    """Windows 2048 and 2049: the first output is the last element of a tile and the first of the next; on resident views of the
    shared series."""
    made, resident = series
    seed = first_output(fn, args)
    n = seed + TILE + 9
    for columns in (COLUMNS, EXACT_COLUMNS):
        views = [resident[k].view(resident[k].n - n, n) for k in columns[fn]]
        ins = inputs_of(fn, made, n, columns)
        got = dev_call(fn, None, args, resident=views)
        assert np.isnan(got[:seed]).all() and np.isfinite(got[seed:]).all()
        check(fn, got, ins, args, f"{fn} {args} n={n} (seed edge)")
    _counts.record(f"runsum/seed_edge/{fn}_{args[0]}", outputs_compared=2 * n)


@pytest.mark.parametrize("fn,args", [("vwap", [20, True]), ("vpin", [32])], ids=ident)
def test_second_trip_of_the_aggregate_scan(fn, args):
    """One tile aggregate more than a trip of the aggregate scan takes, and a few elements: the carried sums cross trips."""
    n = AGG_UNIT * TILE + TILE + 9
    assert -(-n // TILE) == AGG_UNIT + 2 and n == 526_345
    # (moves of 5 cents at most: half a million larger ones reach the generators' floor of 1.00 and stay there)
    ins = (H.grid_walk(n, 807, 5), H.lot_volumes(n, 808)) if fn == "vwap" else (H.lot_volumes(n, 809), H.lot_volumes(n, 810))
    assert fn != "vwap" or ins[0].min() > 10.0
    got = dev_call(fn, ins, args)
    assert np.isfinite(got[first_output(fn, args):]).all()
    check(fn, got, ins, args, f"{fn} {args} n={n} (second trip)")
    _counts.record(f"runsum/second_trip/{fn}", outputs_compared=n)


# ---------------------------------------------------------------------------------------------- the hold of vwap_distance
HOLD_RUNS = {
    "ends_at_edge_1": [[TILE - 40, 40]], "straddles_edge_1": [[TILE - 30, 60]], "begins_at_edge_1": [[TILE, 40]],
    "ends_at_edge_2": [[2 * TILE - 40, 40]], "straddles_edge_2": [[2 * TILE - 30, 60]], "begins_at_edge_2": [[2 * TILE, 40]],
    "two_whole_tiles": [[TILE - 25, 2 * TILE + 60]], "first_window_into_tile_1": [[0, TILE + 100]],
    "many": [[3, 30], [TILE - 21, 21], [TILE + 500, 19], [2 * TILE - 1, 22], [3 * TILE - 10, 310]],
}


@pytest.mark.parametrize("name", sorted(HOLD_RUNS))
def test_hold_across_tiles(series, name):
    """Exactly summable inputs: a window of zero volumes has vsum == 0 exactly and holds the output before it.  Runs that end at,
    straddle and begin at the first and the second tile edge, one that leaves the second and the third tile without a value (the
    index carried into the third tile comes from two tiles back, into the fourth from three) and one from element 0 into the second
    tile (NaN is carried)."""
    made, _ = series
    n, w = len(made["g64"]), 20
    c, v = made["g64"], H.int_volumes(n, 805, HOLD_RUNS[name])
    for lg in (False, True):
        want, held = H.vwap_distance(c, v, w, lg, sums=True)
        expect = sum(max(length - (w - 1), 0) for _, length in HOLD_RUNS[name]) if name != "many" else None
        assert expect is None or held.sum() == min(expect, n - (w - 1)), (name, int(held.sum()))
        check("vwap", dev_call("vwap", (c, v), [w, lg]), (c, v), [w, lg], f"vwap hold {name} log={lg}")
    if name == "first_window_into_tile_1":
        assert np.isnan(want[:TILE + 100]).all() and np.isfinite(want[TILE + 100:]).all()
    if name == "two_whole_tiles":
        assert held[TILE - 6:3 * TILE + 35].all() and not held[TILE - 7] and not held[3 * TILE + 35]
        assert (want[TILE - 6:3 * TILE + 35] == want[TILE - 7]).all() and np.isfinite(want[TILE - 7])
    _counts.record(f"runsum/hold/{name}", outputs_compared=2 * n, held=int(held.sum()))


# ---------------------------------------------------------------------------------------------- NaN, positions compared exactly
@pytest.mark.parametrize("at", (TILE - 1, TILE))
def test_a_nan_at_a_tile_edge(series, at):
    """A NaN in the last element of a tile and in the first of the next, for each function and each of its inputs."""
    made, _ = series
    n = 2 * TILE + 100
    for fn, args in (("boll", [20, 2.0]), ("vwap", [20, False]), ("vwap", [20, True]), ("flow", [20, 5]), ("vpin", [20]), ("park", [])):
        for col in range(H.N_INPUTS[fn]):
            ins = [a.copy() for a in inputs_of(fn, made, n)]
            ins[col][at] = np.nan
            got = dev_call(fn, tuple(ins), args)
            if fn in ("boll", "flow") or (fn == "vwap" and col == 0):
                assert np.isfinite(got[19:at]).all() and np.isnan(got[at:]).all()       # NaN for good
            elif fn == "vwap":
                assert np.isfinite(got).sum() == n - 19 and (got[at:] == got[at - 1]).all()   # held for good
            elif fn == "vpin":
                assert np.isnan(got[at:at + 20]).all() and np.isfinite(got[at + 20:]).all() and np.isfinite(got[19:at]).all()
            else:
                assert np.isnan(got[at]) and np.isfinite(got).sum() == n - 1
            check(fn, got, tuple(ins), args, f"{fn} {args} NaN in input {col} at {at}")


# ---------------------------------------------------------------------------------------------- every element is written
@pytest.mark.parametrize("fn,args", [("boll", [300, 2.0]), ("boll", [1, 2.0]), ("vwap", [300, True]), ("flow", [300, 5]), ("flow", [5, 5]),
                                     ("flow", [0, 0]), ("vpin", [300]), ("vpin", [0]), ("park", [])], ids=ident)
def test_no_element_is_left_unwritten(series, fn, args):
    """A prefilled output buffer (dev_call asserts that no prefilled value is left): the NaN head and a series shorter than the
    window come from the kernels."""
    made, _ = series
    for n in (1, 7, 299, TILE - 1, TILE + 1, 2 * TILE + 3):
        ins = inputs_of(fn, made, n)
        check(fn, dev_call(fn, ins, args), ins, args, f"{fn} {args} n={n} (prefilled)")


# ---------------------------------------------------------------------------------------------- transforms, Compose, DeviceTrades
def test_transforms_on_a_small_frame():
    import pandas as pd

    from finmlkit_amd.feature.transforms import BollingerPercentB, FlowAcceleration, ParkinsonRange, VPIN, VWAPDistance
    n = 500
    h, lo, c = H.hlc_walk(n, 811)
    v, b, s = H.lot_volumes(n, 812), H.lot_volumes(n, 813), H.lot_volumes(n, 814)
    idx = pd.date_range("2024-01-01", periods=n, freq="min")
    frame = pd.DataFrame({"high": h, "low": lo, "close": c, "volume": v, "volume_buy": b, "volume_sell": s}, index=idx)
    for backend in ("nb", "pd"):
        for t, fn, args, ins in ((BollingerPercentB(20), "boll", [20, 2.0], (c,)), (BollingerPercentB(20, 1.5, "high"), "boll", [20, 1.5], (h,)),
                                 (VWAPDistance(20), "vwap", [20, False], (c, v)), (VWAPDistance(20, True), "vwap", [20, True], (c, v)),
                                 (ParkinsonRange(), "park", [], (h, lo)), (FlowAcceleration(20, 5), "flow", [20, 5], (v,)),
                                 (VPIN(), "vpin", [32], (b, s)), (VPIN(8, ["volume_sell", "volume"]), "vpin", [8], (s, v))):
            out = t(frame, backend=backend)
            assert out.name == t.output_name and out.index.equals(idx)
            assert out.dtype == (np.float32 if fn == "vpin" else np.float64)
            check(fn, out.values, ins, args, f"{type(t).__name__} {backend}")


def test_compose_chains_on_the_device():
    import pandas as pd

    from finmlkit_amd.feature.core.ma import ewma, sma
    from finmlkit_amd.feature.transforms import EWMA, SMA, BollingerPercentB, Compose, FlowAcceleration, SISOTransform
    n = 3000
    c, v = H.grid_walk(n, 815), H.lot_volumes(n, 816)
    idx = pd.date_range("2024-01-01", periods=n, freq="s")
    frame = pd.DataFrame({"close": c, "volume": v}, index=idx)
    P = product()
    # on the device path the chain is the two kernels on the same data: it equals the two functions called one after the other in
    # every bit, and the second step is held against the restatement on the first's output
    for chain, name, first, fn, args in (
            (Compose(EWMA(5, "close"), BollingerPercentB(20, 2.0, "ewma5")), "close_ewma5_bollb20", ewma(c, 5), "boll", [20, 2.0]),
            (Compose(EWMA(5, "volume"), FlowAcceleration(20, 5, "ewma5")), "volume_ewma5_flowacc_20_5", ewma(v, 5), "flow", [20, 5])):
        assert all(type(t)._dev is not SISOTransform._dev for t in chain.transforms)          # every step has a device form
        got = chain(frame)
        assert got.name == name
        want = H.call(fn, (first,), args, mod=P)
        assert np.isnan(want[:19]).all() and np.isfinite(want[19:]).all()
        equal(got.values, want, name)
        check(fn, want, (first,), args, name + ": the second step on the first's output")
    # SMA's NaN head lies in Bollinger's first window and poisons its sums for good, in the reference as well
    got = Compose(SMA(5, "close"), BollingerPercentB(20, 2.0, "sma5"))(frame)
    assert got.name == "close_sma5_bollb20" and np.isnan(got.values).all()
    equal(got.values, H.bollinger_percent_b(sma(c, 5), 20, 2.0), "Compose(SMA, BollingerPercentB)")


def test_device_trades_methods():
    from finmlkit_amd import _ffi, engine
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    n = TILE + 77
    h, lo, c = H.hlc_walk(n, 817)
    v, u = H.lot_volumes(n, 818), H.lot_volumes(n, 819)
    t = engine.DeviceTrades.synth(16, seed=1, ctx=ctx)
    dh, dl, dc, dv, du = (DeviceArray.from_host(ctx, a) for a in (h, lo, c, v, u))
    for got, fn, args, ins in ((t.bollinger_percent_b(dc, 20), "boll", [20, 2.0], (c,)), (t.bollinger_percent_b(dc, 20, 1.0), "boll", [20, 1.0], (c,)),
                               (t.vwap_distance(dc, dv, 20), "vwap", [20, False], (c, v)), (t.vwap_distance(dc, dv, 20, True), "vwap", [20, True], (c, v)),
                               (t.parkinson_range(dh, dl), "park", [], (h, lo)), (t.flow_acceleration(dv, 20, 5), "flow", [20, 5], (v,)),
                               (t.vpin(dv, du, 32), "vpin", [32], (v, u))):
        assert isinstance(got, DeviceArray) and got.n == n and got.dtype == (np.float32 if fn == "vpin" else np.float64)
        check(fn, got.to_host(), ins, args, f"DeviceTrades {fn} {args}")
    empty = DeviceArray(ctx, 0, np.float64)
    assert t.bollinger_percent_b(empty, 3).n == 0 and t.vpin(empty, empty, 3).n == 0 and t.vpin(empty, empty, 3).dtype == np.float32
