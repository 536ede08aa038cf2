"""The tick-level features on the MI355X -- comp_lagged_returns, ewmst, ewmst_mean0, ewms, realized_vol (csrc/fmk_ticklevel.hip) -- at
the kernels' own tile sizes and on irregular tapes, against the sequential restatement of tests/_ticklevel_ref.py, which
tests/test_ticklevel_host.py holds bit for bit against outputs recorded from the untouched reference.  Every call goes through the
`_dev` entry on resident arrays with the output buffer prefilled with a sentinel, so an element the kernels do not write shows; the
recorded cases also go through the Python functions.  No test reads the reference checkout.

Bit for bit: comp_lagged_returns, simple and log (np.array_equal, equal_nan=True; inf positions equal).
ewmst / ewmst_mean0: NaN and inf positions, out[0], every element where the restatement is sigma_floor or 0.0 exactly; elsewhere the
contract of DESIGN.md section 5 (1e-9 relative, or 1e-11 x the series' median absolute) and, on top of it, BOUND.
ewms: NaN positions exactly, the rest within BOUND.  realized_vol: NaN and inf positions exactly, the rest within BOUND of the
correctly rounded value.  BOUND[fn] is the largest relative deviation from the restatement measured on the MI355X over every case of
this file x 16, rounded up to a power of ten and never above the contract (realized_vol: the larger of that figure and the
interpreted reference's own deviation from the correctly rounded value, recorded in the fixture, and never above 1e-12); DESIGN.md
section 5 holds the measured figures.

Infinite y in ewmst is the one input on which a scan cannot follow the loop: across a tile whose decay product underflows to 0 the
composed state is 0 * inf = NaN where the loop keeps inf.  What must hold is tested: the outputs before the first infinite element
are unaffected, and from it on ewmst is sigma_floor (a NaN and an inf state both give that in the closing expression); ewmst_mean0
is compared from the infinite element on only on a tape whose decay product stays normal to the end.  No case with finite inputs
leaves out any element.

ewmst after a restart.  After a 3-day gap (alpha exactly 1: the state is one sample) followed by gaps of 0 and 1 ns, var_raw and
denom are both cancellation residues of 1e-10 x their operands and their quotient is a sigma of ordinary size, which a state
composed instead of stepped moves by 1e-16 / 1e-10: the recorded cases ewmst.length.n2047 (1.3e-5 relative before),
ewmst.half_life.600.0 (4.9e-7) and ewmst.half_life.0.05 (1.0e-7) hold such ticks.  The kernels step them (k_ew_restart_walk), and
test_ewmst_walk_after_a_restart places restarts by construction at every edge of that walk."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _ticklevel_ref as H
from tests._ticklevel_fixture import MANIFEST, NOTES, OK_CASES, REFUSED, RV_CASES, case_input, restated

pytestmark = pytest.mark.gpu

ENTRY = {"lr": "fmk_comp_lagged_returns_dev", "ewmst": "fmk_ewmst_dev", "ewmst0": "fmk_ewmst_dev", "ewms": "fmk_ewms_dev",
         "rv": "fmk_realized_vol_dev"}
CONTRACT = {"ewmst": 1e-9, "ewmst0": 1e-9, "ewms": 1e-9, "rv": 1e-12}
# measured on the MI355X over all cases below: ewmst 2.5e-10 (n = 526 345; x 16 is above the contract, so its bound is the contract), ewmst_mean0 3.6e-15, ewms 1.3e-14, realized_vol
# 4.6e-16 (the interpreted reference: 6.1e-16), each x 16, rounded up to a power of ten, never above the contract
BOUND = {"ewmst": 1e-9, "ewmst0": 1e-13, "ewms": 1e-12, "rv": 1e-14}
SENTINEL = 12345.678
WORST = {}


def product():
    from types import SimpleNamespace

    from finmlkit_amd.feature.core.utils import comp_lagged_returns
    from finmlkit_amd.feature.core.volatility import ewms, ewmst, ewmst_mean0, realized_vol
    return SimpleNamespace(comp_lagged_returns=comp_lagged_returns, ewmst=ewmst, ewmst_mean0=ewmst_mean0, ewms=ewms, realized_vol=realized_vol)


def c_args(fn, args):
    if fn == "lr":
        return (C.c_double(float(args[0])), C.c_int(bool(args[1])))
    if fn in ("ewmst", "ewmst0"):
        return (C.c_double(float(args[0])), C.c_double(float(args[1]) if len(args) > 1 else 1e-12), C.c_int(fn == "ewmst0"))
    if fn == "ewms":
        return (C.c_int64(int(args[0])),)
    return (C.c_int64(int(args[0])), C.c_int(bool(args[1])))


def dev_call(fn, inputs, args, resident=None, out=None):
    """The `_dev` entry of `fn` on resident copies of the inputs (or on `resident`: DeviceArrays or views of them) -> host array.
    The output buffer (or `out`, a view) holds SENTINEL before the call; no element may hold it afterwards."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    dev = resident or [DeviceArray.from_host(ctx, np.ascontiguousarray(a)) for a in inputs]
    n = dev[-1].n
    assert all(d.n == n for d in dev) and n > 0
    assert [d.dtype for d in dev] == ([np.int64, np.float64] if len(dev) == 2 else [np.float64])
    o = out if out is not None else DeviceArray.from_host(ctx, np.full(n, SENTINEL))
    assert o.n == n
    ctx.call(ENTRY[fn], *(d.p for d in dev), C.c_int64(n), *c_args(fn, args), o.p)
    got = o.to_host()
    assert not (got == SENTINEL).any(), (fn, args, n, "an element was left unwritten", np.flatnonzero(got == SENTINEL)[:5])
    return got


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert np.array_equal(got, want, equal_nan=True), (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def close(fn, got, want, what, floor=None):
    """comp_lagged_returns: every bit.  The others: NaN and inf positions exactly; ewmst / ewmst_mean0 also out[0], the elements where
    the restatement is `floor` or 0.0 exactly, and the contract; the rest within BOUND[fn] relative, the largest deviation kept."""
    got, want = np.asarray(got), np.asarray(want)
    if fn == "lr":
        return equal(got, want, what)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    for kind, g, w in (("NaN", np.isnan(got), np.isnan(want)), ("inf", np.isinf(got), np.isinf(want))):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, kind + " positions", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), (what, "sign of inf")
    ok = np.isfinite(want)
    if fn in ("ewmst", "ewmst0"):
        assert np.isnan(got[0]), what
        pinned = ok & ((want == 0.0) | (want == floor))
        bad = np.nonzero(pinned & (got != want))[0]
        assert len(bad) == 0, (what, "floor or zero", len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
        ok &= ~pinned
    else:
        zero = ok & (want == 0.0)
        assert (got[zero] == 0.0).all(), (what, "expected 0.0")
        ok &= ~zero
    if not ok.any():
        return
    err = np.abs(got[ok] - want[ok])
    dev = err / np.abs(want[ok])
    if fn in ("ewmst", "ewmst0"):                      # the contract, as test_ewmst_deviation_from_the_sequential_loop states it
        typical = float(np.median(np.abs(want[ok])))
        assert np.all((dev <= CONTRACT[fn]) | (err <= 1e-11 * typical)), (what, "contract", float(dev.max()), float(err.max()), typical)
    worst = float(dev.max())
    if worst > WORST.get(fn, (0.0, ""))[0]:
        WORST[fn] = (worst, what)
        _counts.record(f"ticklevel/max_deviation/{fn}", value=repr(worst), bound=repr(BOUND[fn]), case=what)
    print(f"deviation {fn} {what}: {worst:.3e}")
    assert worst <= BOUND[fn] <= CONTRACT[fn], (what, worst, BOUND[fn], int(np.nonzero(ok)[0][dev.argmax()]))


def tally(name, fn, compared, exact):
    _counts.record(f"ticklevel/{name}", fn=fn, outputs_compared=int(compared), exact_comparisons=int(exact))


def exact_count(fn, want, floor=None):
    """How many elements of a comparison with `want` are compared exactly."""
    if fn == "lr":
        return want.size
    pinned = ~np.isfinite(want) | (want == 0.0)
    if fn in ("ewmst", "ewmst0"):
        pinned |= want == floor
    return int(pinned.sum())


# ---------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay(name):
    c, ins, want = MANIFEST[name], case_input(name), restated(name)
    fn, args = c["fn"], c["args"]
    floor = args[1] if fn in ("ewmst", "ewmst0") else None
    close(fn, H.call(fn, ins, args, mod=product()), want, name + " (python)", floor)
    calls = 1
    if not (fn == "rv" and args[0] < 1):               # window 0: the Python function answers, the entry refuses (below)
        close(fn, dev_call(fn, ins, args), want, name + " (_dev)", floor)
        calls = 2
    tally(f"fixture/{name}", fn, calls * c["n"], calls * exact_count(fn, want, floor))


@pytest.mark.parametrize("name", REFUSED + ["rv.w0"])
def test_refused_arguments_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    c, ins = MANIFEST[name], case_input(name)
    fn, args = c["fn"], c["args"]
    ctx, lib = _ffi.default_context(), _ffi.lib()
    with pytest.raises(ValueError) as e:
        dev_call(fn, ins, args)
    assert c.get("message", H.RV_WINDOW_MESSAGE) in str(e.value)
    if name != "rv.w0":
        with pytest.raises(ValueError):
            H.call(fn, ins, args, mod=product())
    for entry in (ENTRY[fn], ENTRY[fn][:-4]):          # the host-pointer flavour too: refused before any pointer is looked at
        rc = getattr(lib, entry)(ctx.handle, *(None for _ in ins), C.c_int64(c["n"]), *c_args(fn, args), None)
        assert rc == _ffi.E_ARG, entry


# ---------------------------------------------------------------------------------------------- comp_lagged_returns
@pytest.mark.parametrize("kind,seed", [("burst", 961), ("small", 962)])
def test_lagged_returns_every_length_and_window(kind, seed):
    """The lengths around the tile of 1024 ticks x the windows below the float64 spacing, at it, inside the stage and longer than
    the tape, simple and log."""
    compared = 0
    for n in H.LR_LENGTHS:
        ts, px = H.lr_inputs(kind, n, seed, seed + 10)
        for w in H.LR_WINDOWS:
            lag = H.lag_index(ts, w)
            if w == 1e7 or (w == 1e-7 and kind == "burst"):
                assert (lag < 0).all()                 # longer than the tape; below the spacing of float64 at 1.7e18: ti <= target
            for lg in (False, True):
                want = H.comp_lagged_returns(ts, px, w, lg)
                assert np.array_equal(np.isnan(want), lag < 0)
                equal(dev_call("lr", (ts, px), [w, lg]), want, f"lr {kind} n={n} w={w} log={lg}")
                compared += n
    tally(f"lr_lengths/{kind}", "lr", compared, compared)


def stage_lengths(ts, w):
    """Per tile of k_lagged_returns the number of timestamps it needs staged: from the lag of its first tick (tick 0 when it has
    none) to its last tick."""
    tsf = np.asarray(ts, np.int64).astype(np.float64)
    out = []
    for first in range(0, len(tsf), H.LR_TILE):
        last = min(first + H.LR_TILE, len(tsf)) - 1
        lo = int(np.searchsorted(tsf[:first], tsf[first] - w * 1e9, side="right")) - 1
        out.append(last - max(lo, 0) + 1)
    return np.array(out)


@pytest.mark.parametrize("look", (2047, 2048, 2049))
def test_lagged_returns_at_the_capacity_of_the_stage(look):
    """1 ms spacing and a window of look - 0.5 ms: every tick from `look` on looks back exactly `look` ticks, so the fourth tile
    (the first whose first tick has a look-back that long) needs LR_CAP - 1, LR_CAP and LR_CAP + 1 timestamps: the last staged
    sizes and the first that falls back to the global search."""
    name = f"lr.stage.look{look}"
    ts, px = case_input(name)
    w = MANIFEST[name]["args"][0]
    lag = H.lag_index(ts, w)
    idx = np.arange(len(ts))
    assert (lag[look:] == idx[look:] - look).all() and (lag[:look] == -1).all()
    need = stage_lengths(ts, w)
    assert need[3] == H.LR_TILE + look == H.LR_CAP + (look - 2048) and (need[:3] <= H.LR_CAP).all()
    for lg in (False, True):
        equal(dev_call("lr", (ts, px), [w, lg]), H.comp_lagged_returns(ts, px, w, lg), f"{name} log={lg}")
    tally(f"lr_stage/{look}", "lr", 2 * len(ts), 2 * len(ts))


def test_lagged_returns_staged_and_unstaged_tiles_in_one_call():
    ts, px = case_input("lr.mixed.simple")
    need = stage_lengths(ts, 1.0)
    unstaged = np.flatnonzero(need > H.LR_CAP)
    assert len(unstaged) >= 1 and unstaged.min() >= 1 and unstaged.max() + 1 < len(need), need
    assert need[unstaged.min() - 1] <= H.LR_CAP and need[unstaged.max() + 1] <= H.LR_CAP, need      # staged neighbours on both sides
    assert H.equal_run_lengths(ts).max() >= H.LONG_RUN
    for lg in (False, True):
        want = restated("lr.mixed.log" if lg else "lr.mixed.simple")
        assert np.isfinite(want[unstaged[0] * H.LR_TILE:(unstaged[0] + 1) * H.LR_TILE]).any()
        equal(dev_call("lr", (ts, px), [1.0, lg]), want, f"lr mixed log={lg}")
    tally("lr_mixed", "lr", 2 * len(ts), 2 * len(ts))


def test_lagged_returns_target_on_a_run_of_equal_timestamps():
    """Exact timestamps 1 s apart with ticks 1020..1030 sharing one: the target of tick 1035 (15 s back) is that timestamp, and the
    lag is the last tick of the run, across the tile edge."""
    n = 1100
    ts = H.SMALL_BASE_NS + np.arange(n, dtype=np.int64) * 1_000_000_000
    ts[1020:1031] = ts[1020]
    px = H.prices(n, 963)
    lag = H.lag_index(ts, 15.0)
    assert ts[1035] - 15_000_000_000 == ts[1020] == ts[1030] < ts[1031]
    assert lag[1034] == 1019 and (lag[1035:1046] == 1030).all() and lag[1046] == 1031
    assert (lag[1020:1031] == 1005).all()              # the run's own ticks share one lag
    for lg in (False, True):
        want = H.comp_lagged_returns(ts, px, 15.0, lg)
        assert want[1035] == (H.host_log(px[1035] / px[1030]) if lg else px[1035] / px[1030] - 1.0)
        equal(dev_call("lr", (ts, px), [15.0, lg]), want, f"lr target on a run log={lg}")
    tally("lr_equal_run", "lr", 2 * n, 2 * n)


def test_lagged_returns_zero_and_nan_prices():
    """A zero price gives inf at the ticks that lag onto it (the reference's documented rule), a NaN price NaN at its own tick and
    at the ticks that lag onto it."""
    ts, px = case_input("lr.odd_prices.simple")
    lag = H.lag_index(ts, 1e-3)
    zeros, nans = np.flatnonzero(px == 0.0), np.flatnonzero(np.isnan(px))
    at = MANIFEST["lr.odd_prices.simple"]["source"]["kw"]
    assert list(zeros) == sorted(at["zero_at"]) and list(nans) == sorted(at["nan_at"]) and zeros[1] < H.LR_TILE <= nans[1]
    idx = np.arange(len(px))
    onto_zero = np.isin(lag, zeros)                    # (the zero divisor is looked at first: inf whatever the tick's own price)
    onto_nan = np.isin(lag, nans) | (np.isin(idx, nans) & (lag >= 0) & ~onto_zero)
    assert onto_zero.sum() >= 2 and onto_nan.sum() >= 3
    for lg in (False, True):
        got = dev_call("lr", (ts, px), [1e-3, lg])
        assert (got[onto_zero] == np.inf).all() and np.isnan(got[onto_nan]).all()
        own_zero = np.isin(idx, zeros) & (lag >= 0) & ~onto_zero & ~onto_nan       # a zero price over its lag: -1.0, or log(0) = -inf
        assert (got[own_zero] == (-np.inf if lg else -1.0)).all() and own_zero.any()
        equal(got, restated("lr.odd_prices.log" if lg else "lr.odd_prices.simple"), f"lr odd prices log={lg}")
    tally("lr_odd_prices", "lr", 2 * len(ts), 2 * len(ts))


@pytest.mark.parametrize("close_at,out_at", [(0, 0), (1, 0), (0, 1), (1, 1), (2, 2)])
def test_lagged_returns_on_views_of_every_alignment(close_at, out_at):
    """`close` and the output at an even and an odd element offset of their buffers: both the 16-byte and the scalar loads and
    stores of k_lagged_returns run; what lies around the output view stays as it was."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    n = 3 * 1024 + 5
    ts, px = H.lr_inputs("burst", n, 964, 965)
    d_ts = DeviceArray.from_host(ctx, np.concatenate((np.zeros(3, np.int64), ts)))
    d_px = DeviceArray.from_host(ctx, np.concatenate((np.full(close_at, np.nan), px)))
    for lg in (False, True):
        d_out = DeviceArray.from_host(ctx, np.full(n + 8, SENTINEL))
        got = dev_call("lr", None, [1e-3, lg], resident=[d_ts.view(3, n), d_px.view(close_at, n)], out=d_out.view(out_at, n))
        equal(got, H.comp_lagged_returns(ts, px, 1e-3, lg), f"lr views close+{close_at} out+{out_at} log={lg}")
        whole = d_out.to_host()
        assert (whole[:out_at] == SENTINEL).all() and (whole[out_at + n:] == SENTINEL).all()
    tally(f"lr_views/{close_at}_{out_at}", "lr", 2 * n, 2 * n)


# ---------------------------------------------------------------------------------------------- ewmst / ewmst_mean0 / ewms
@pytest.mark.parametrize("fn", ("ewmst", "ewmst0"))
def test_ewmst_second_level_of_the_scan(orc, fn):
    """257 tiles and 9 ticks: more tile maps than one group of the hierarchical scan holds, so the group maps are scanned too.  The
    one case whose expected values are the C oracle's, which tests/test_ticklevel_host.py holds bit for bit against the restatement
    on every recorded case."""
    n = (H.EW_GROUP + 1) * H.EW_TILE + 9
    assert -(-n // H.EW_TILE) == H.EW_GROUP + 2 > H.EW_GROUP
    ts, y = H.ew_inputs("burst", n, 966, 967, nan=[(0, 40), (300_000, 300_020)])
    assert np.isfinite(y[40:300_000]).all() and (np.diff(ts) == H.DAY3_NS).sum() == 2 and H.equal_run_lengths(ts).max() >= H.LONG_RUN
    want = H.call(fn, (ts, y), [600.0, 1e-12], mod=orc)
    assert np.isfinite(want[100:]).all()
    close(fn, dev_call(fn, (ts, y), [600.0, 1e-12]), want, f"{fn} n={n} (second level)", 1e-12)
    tally(f"ew_second_level/{fn}", fn, n, exact_count(fn, want, 1e-12))


@pytest.mark.parametrize("fn", ("ewmst", "ewmst0"))
def test_ewmst_on_views_at_an_odd_offset(fn):
    """The arrays one element behind a 16-byte boundary, as a shard's are: the 16-byte loads and stores of whole tiles on an 8-byte
    alignment."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    n = 3 * H.EW_TILE + 9
    ts, y = H.ew_inputs("burst", n, 968, 969, nan=[(0, 3)])
    want = H.call(fn, (ts, y), [5.0, 1e-12])
    d_ts = DeviceArray.from_host(ctx, np.concatenate((np.zeros(1, np.int64), ts)))
    d_y = DeviceArray.from_host(ctx, np.concatenate((np.zeros(1), y)))
    d_out = DeviceArray.from_host(ctx, np.full(n + 2, SENTINEL))
    got = dev_call(fn, None, [5.0, 1e-12], resident=[d_ts.view(1, n), d_y.view(1, n)], out=d_out.view(1, n))
    close(fn, got, want, f"{fn} views at +1", 1e-12)
    whole = d_out.to_host()
    assert whole[0] == SENTINEL and whole[-1] == SENTINEL
    tally(f"ew_views/{fn}", fn, n, exact_count(fn, want, 1e-12))


@pytest.mark.parametrize("at", (7, 2047, 2048, 2100))
def test_ewmst_with_an_infinite_element(at):
    """On the burst tape (3-day gaps: a decay product of exactly 0): the outputs before the infinite element are those of the series
    without it, and from it on ewmst is sigma_floor.  ewmst_mean0 is compared there on the recorded even tape only (fixture replay)."""
    n = H.N_EW
    ts, y = H.ew_inputs("burst", n, 970, 971, nan=[(0, 3)], inf_at=[at])
    _, plain = H.ew_inputs("burst", n, 970, 971, nan=[(0, 3)])
    assert np.isinf(y).sum() == 1 and (np.diff(ts) == H.DAY3_NS).any()
    for fn, floor in (("ewmst", 1e-12), ("ewmst", 1e-3), ("ewmst0", 1e-12)):
        want = H.call(fn, (ts, y), [5.0, floor])
        assert np.array_equal(want[:at], H.call(fn, (ts, plain), [5.0, floor])[:at], equal_nan=True)
        got = dev_call(fn, (ts, y), [5.0, floor])
        close(fn, got[:at], want[:at], f"{fn} before the inf at {at}", floor)
        if fn == "ewmst":                              # (NaN while no tick has had dt > 0 yet: the weights are still 0)
            assert ((want[at:] == floor) | np.isnan(want[at:])).all() and (want[at:] == floor).sum() > (n - at) // 2
            assert np.array_equal(got[at:], want[at:], equal_nan=True)
    tally(f"ew_inf/{at}", "ewmst", 3 * n, 2 * (n - at))


# ---------------------------------------------------------------------------------------------- ewmst: the walk after a restart
D3, S1, S55, S60 = H.DAY3_NS, 1_000_000_000, 55_000_000_000, 60_000_000_000      # with a half life of 5 s: 1 - alpha = 0, 0.82, 1.7e-5, 6.1e-6
RESTART_OM = 1e-5                    # csrc/fmk_ticklevel.hip: EW_RESTART_OM, a tick with 1 - alpha at most this is a restart
WALK_CAP = 1 << 16                   # EW_WALK_CAP: the ticks one walk steps
RESTART_RECORDS = 1 << 16            # EW_RESTART_RECORDS: a call with more restart records is not walked
# name -> (n, the placed gaps of H.gap_tape on a fill of 1 s, the ticks that are restarts)
WALKS = {
    "across_a_tile_edge": (4200, [(2040, 2040, D3), (2041, 2060, 0), (2061, 2061, 1), (2062, 2100, 0), (2101, 2110, 1)], [2040]),
    "ends_on_the_next_restart": (600, [(100, 100, D3), (101, 140, 1), (141, 141, D3), (142, 180, 1)], [100, 141]),
    "last_thread_of_a_tile": (2300, [(2047, 2047, D3), (2048, 2090, 1)], [2047]),
    "first_thread_of_a_tile": (2300, [(2048, 2048, D3), (2049, 2090, 1)], [2048]),
    "last_thread_of_the_series": (4101, [(4098, 4098, D3), (4099, 4100, 1)], [4098]),
    "walk_to_the_last_tick": (4104, [(4095, 4095, D3), (4096, 4103, 1)], [4095]),
    "alpha_just_below_one": (700, [(500, 500, S60), (501, 560, 1)], [500]),
    "alpha_just_above_the_threshold": (700, [(500, 500, S55), (501, 560, 1)], []),
    "start_of_the_series": (300, [(2, 60, 1), (61, 70, 0)], []),
    "start_after_equal_timestamps": (300, [(1, 12, 0), (14, 80, 1)], []),
    "two_restarts_in_one_thread": (300, [(96, 96, D3), (97, 98, 1), (99, 99, D3), (100, 150, 1)], [96, 99]),
    # the walk from tick 16 steps WALK_CAP ticks: the last is 15 + WALK_CAP, and the first tick behind it has an ordinary alpha ...
    "as_long_as_the_cap": (16 + WALK_CAP + 3000, [(10, 10, D3), (11, 30000, 0), (30001, 30001, 1), (30002, 15 + WALK_CAP, 0)], [10]),
    # ... or the equal timestamps go on behind it: the state is one sample, exact however it is carried
    "equal_timestamps_past_the_cap": (16 + WALK_CAP + 3000, [(10, 10, D3), (11, WALK_CAP + 600, 0)], [10]),
}


def walk_tape(name):
    n, placed, restarts = WALKS[name]
    ts = H.gap_tape(n, S1, placed)
    y = H.returns(n, 980)
    om = np.array([1.0 - H.alpha_of(int(d), 5.0) for d in np.diff(ts)])
    assert list(np.flatnonzero(om <= RESTART_OM) + 1) == restarts, name          # what the kernels take for a restart, from the tape alone
    return ts, y


@pytest.mark.parametrize("name", sorted(WALKS))
def test_ewmst_walk_after_a_restart(name):
    """A restart (or the first weighted tick) followed by gaps of 0 and 1 ns, placed by construction at the edges of the walk that steps
    those ticks (k_ew_restart_walk): where a record is written, where a walk starts, and each of the ways it ends."""
    ts, y = walk_tape(name)
    want = H.ewmst(ts, y, 5.0)
    assert np.isfinite(want[np.flatnonzero(np.diff(ts) > 0)[0] + 1:]).all()
    close("ewmst", dev_call("ewmst", (ts, y), [5.0, 1e-12]), want, f"ewmst walk {name}", 1e-12)
    close("ewmst0", dev_call("ewmst0", (ts, y), [5.0, 1e-12]), H.ewmst_mean0(ts, y, 5.0), f"ewmst0 walk {name}", 1e-12)
    tally(f"ew_walk/{name}", "ewmst", 2 * len(ts), exact_count("ewmst", want, 1e-12))


def test_ewmst_walk_in_a_shard_that_enters_with_a_state():
    """fmk_ewmst_shard_apply_dev: tick 0 of the arrays is the last tick of the shard before, the state in front of tick 1 is given.
    The shard's first thread enters with weights, so it is no start of a series; the restart five ticks in is walked."""
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray
    ctx = _ffi.default_context()
    ts, y = walk_tape("ends_on_the_next_restart")
    cut = 96
    state = []
    head = H.ewmst(ts[:cut], y[:cut], 5.0, final=state)
    want = H.ewmst(ts, y, 5.0)
    assert np.array_equal(head, want[:cut], equal_nan=True) and state[0] > 0.0
    assert np.array_equal(H.ewmst(ts[cut - 1:], y[cut - 1:], 5.0, state=tuple(state))[1:], want[cut:])
    n = len(ts) - (cut - 1)
    dev = [DeviceArray.from_host(ctx, np.ascontiguousarray(a[cut - 1:])) for a in (ts, y)]
    d_state, d_out = DeviceArray.from_host(ctx, np.array(state)), DeviceArray.from_host(ctx, np.full(n, SENTINEL))
    ctx.call("fmk_ewmst_shard_apply_dev", dev[0].p, dev[1].p, C.c_int64(n), C.c_double(5.0), C.c_double(1e-12), C.c_int(0), d_state.p, d_out.p)
    got = d_out.to_host()
    ctx.sync()
    assert np.isnan(got[0]) and not (got == SENTINEL).any()
    close("ewmst", np.concatenate(([np.nan], got[1:])), np.concatenate(([np.nan], want[cut:])), "ewmst shard with a restart", 1e-12)
    tally("ew_walk/shard", "ewmst", n, 0)


def test_ewmst_with_more_restarts_than_records():
    """A half life of 1e-301 s makes every tick with dt > 0 a restart: more records than a call keeps, so none is walked, and the
    composed outputs are the loop's all the same (alpha is exactly 1: every state is one sample, every sigma the floor)."""
    n = 8 * RESTART_RECORDS + 8 * 300 + 3
    ts, y = H.even_tape(n, 1_000_000), H.returns(n, 981)
    assert H.alpha_of(1_000_000, 1e-301) == 1.0 and n // 8 > RESTART_RECORDS
    head = H.ewmst(ts[:200], y[:200], 1e-301, 1e-3)
    assert np.isnan(head[0]) and (head[1:] == 1e-3).all()
    for _ in range(2):                                 # the same answer twice
        got = dev_call("ewmst", (ts, y), [1e-301, 1e-3])
        assert np.isnan(got[0]) and (got[1:] == 1e-3).all()
    tally("ew_walk/more_than_records", "ewmst", 2 * n, 2 * n)


# ---------------------------------------------------------------------------------------------- realized_vol
BEYOND = [(w, n) for w in H.RV_WINDOWS for n in H.rv_lengths(w) if not H.rv_recorded(w, n)] + [(2048, 3 * 4353 + 77)]


def test_realized_vol_cases_hold_what_they_should():
    """From the data alone, for every window but 1 (all NaN), in a recorded case or in one of BEYOND: the 25.0 outlier, one inf, a NaN
    run longer than the window across the edge between two workgroups (windows above RV_MAX_W: two segments), and windows with exactly
    0, 1 and 2 valid elements."""
    cases = [(MANIFEST[k]["args"][0], MANIFEST[k]["n"], MANIFEST[k]["source"]["kw"], k) for k in RV_CASES]
    cases += [(w, n, H.rv_plan(w, n), None) for w, n in BEYOND]
    seen = set()
    for w, n, kw, name in cases:
        if w < 2 or not kw.get("nan") or kw["nan"][0][1] - kw["nan"][0][0] <= w:
            continue
        (r,) = case_input(name) if name else H.rv_inputs(n, 972, **kw)
        lo, hi = kw["nan"][0]
        edge = H.rv_outputs_per_workgroup(w) if w <= H.RV_MAX_W else 2 * w
        assert np.isnan(r[lo:hi]).all() and hi - lo > w and lo < edge < hi and (r == 25.0).sum() == 1 and np.isinf(r).sum() == 1
        valid = np.convolve((~np.isnan(r)).astype(np.int64), np.ones(w, np.int64))[w - 1:n]
        assert (valid == 1).any() and (valid == 2).any() and (valid == 0).any()
        if name:
            want = restated(name)
            assert np.isnan(want[w - 1:][valid <= 1]).all() and not np.isnan(want[w - 1:][valid >= 2]).any()
        seen.add(w)
    assert seen == set(H.RV_WINDOWS) - {1}


@pytest.mark.parametrize("w,n", BEYOND)
def test_realized_vol_beyond_the_fixture(w, n):
    """The lengths of the table (H.rv_lengths) whose interpreted run is too long to record, and a third workgroup."""
    kw = H.rv_plan(w, n)
    (r,) = H.rv_inputs(n, 972, **kw)
    want = H.realized_vol(r, w, True)
    assert np.isinf(want).any() and np.isfinite(want).sum() > (n - w) // 4
    if n >= 3 * w + 20 or (w <= H.RV_MAX_W and n > 2 * H.rv_outputs_per_workgroup(w)):
        assert kw["nan"][0][1] - kw["nan"][0][0] > w and np.isnan(want[w - 1:]).any()
    close("rv", dev_call("rv", (r,), [w, True]), want, f"rv w={w} n={n}")
    tally(f"rv_beyond/{w}_{n}", "rv", n, int((~np.isfinite(want)).sum()))


def test_the_bounds_are_the_measured_ones():
    """BOUND is never above the contract, and realized_vol's is no tighter than the reference's own deviation from the correctly
    rounded value allows (x 16, as for a measured figure)."""
    for fn in BOUND:
        assert BOUND[fn] <= CONTRACT[fn]
    assert NOTES["reference_deviation_max"] * 16 <= BOUND["rv"] <= 1e-12
