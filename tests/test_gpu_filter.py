"""The symmetric CUSUM event filter on the MI355X: int64 indices, bit-equal to the reference's recorded outputs
(tests/golden/cusum_filter.npz) and to the plain-Python restatement of tests/_filter_ref.py.  Every case runs under both forced
schedules (FMK_CUSUM_FILTER_FORM) and under the library's own choice.  There is no tolerance: every output is an index."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import _counts
from tests import _filter_ref as H
from tests.test_filter_host import MANIFEST, OK_CASES, RAISING, case_inputs, expected

pytestmark = pytest.mark.gpu

L = 4096                            # ticks per chunk (csrc/fmk_cusum_onepass.h: CS1_L); tick i sits at chunk offset i - 1
BIG = 2 * 32 * L + L + 77           # two full workgroups of pass A plus a partial chunk
FORMS = ("onepass", "fixed", None)


class forced:
    """FMK_CUSUM_FILTER_FORM for the duration of a block (None: the library's own choice)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = os.environ.pop("FMK_CUSUM_FILTER_FORM", None)
        if self.form:
            os.environ["FMK_CUSUM_FILTER_FORM"] = self.form

    def __exit__(self, *a):
        os.environ.pop("FMK_CUSUM_FILTER_FORM", None)
        if self.old is not None:
            os.environ["FMK_CUSUM_FILTER_FORM"] = self.old


def diag_last():
    from finmlkit_amd import _ffi
    v = [C.c_int64() for _ in range(4)]
    _ffi.check(_ffi.lib().fmk_diag_cusum_filter_last(*[C.byref(x) for x in v]))
    return dict(zip(("form", "launches", "pending_first", "chunks"), (int(x.value) for x in v)))


def check(x, thr, name=None, want=None):
    """The filter under both forced forms and the default against `want` (default: the helper's indices) -> (want, default diag)."""
    from finmlkit_amd import sampling
    x, thr = np.asarray(x, np.float64), np.asarray(thr, np.float64)
    with np.errstate(all="ignore"):
        want = H.cusum_filter(x, thr) if want is None else want
    d = None
    for form in FORMS:
        with forced(form):
            got = sampling.cusum_filter(x, thr)
        d = diag_last()
        assert got.dtype == np.int64, (name, form)
        assert np.array_equal(got, want), (name, form, len(got), len(want))
        assert d["chunks"] == -(-(len(x) - 1) // L)
        if form:
            assert d["form"] == (form == "fixed"), (name, form, d)       # the forced form answered
    if name:
        _counts.record(f"cusum_filter/{name}", events_compared=len(want), forms=len(FORMS))
    return want, d


def walk(n, seed, sigma=1e-3):
    rng = np.random.default_rng(seed)
    return 100.0 * np.exp(np.cumsum(sigma * rng.standard_normal(n)))


@pytest.fixture(scope="module")
def big_walk():
    x = walk(BIG, 31)
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------- the reference's recorded outputs
@pytest.mark.parametrize("name", OK_CASES)
def test_fixture_replay(orc, name):
    x, thr = case_inputs(name, orc)
    check(x, thr, name="fixture/" + name, want=expected(name))


@pytest.mark.parametrize("name", RAISING)
def test_fixture_replay_raising(orc, name):
    from finmlkit_amd import _ffi, sampling
    x, thr = case_inputs(name, orc)
    with pytest.raises(ValueError) as e:
        sampling.cusum_filter(x, thr)
    assert str(e.value) == MANIFEST[name]["message"]
    # ... and the library itself says the same when it is handed the lengths
    ctx = _ffi.default_context()
    buf = np.zeros(4)
    m = C.c_int64()
    with pytest.raises(ValueError) as e:
        ctx.call("fmk_cusum_filter", _ffi.ptr(buf), C.c_int64(len(x)), _ffi.ptr(buf), C.c_int64(len(thr)), None, C.c_int64(0),
                 C.byref(m))
    assert str(e.value) == MANIFEST[name]["message"]


# ---------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("n", [2, 3, 64, 65, 66, 4096, 4097, 4098, 8193, 131_073, 131_074, BIG])
def test_geometry(big_walk, n):
    x = big_walk[BIG - n:]                          # the last n elements: a different phase of the walk at every size
    want, _ = check(x, [0.01], name=f"geometry/{n}/const")
    if n >= 4096:
        assert len(want) > n // 1000
    check(x, H.hashed_threshold(n, 0.006, True), name=f"geometry/{n}/per")


def test_events_on_both_sides_of_a_chunk_boundary():
    n = 3 * L + 5
    x = walk(n, 32)
    x[L:] *= 3.0                                    # tick 4096: the last of chunk 0
    x[L + 1:] *= 3.0                                # tick 4097: the first of chunk 1
    x[2 * L:] /= 3.0                                # ... and downwards at the next boundary
    x[2 * L + 1:] /= 3.0
    for thr in ([0.01], H.hashed_threshold(n, 0.006, True)):
        want, _ = check(x, thr, name=f"boundary/{len(thr)}")
        assert {L, L + 1, 2 * L, 2 * L + 1} <= set(want.tolist())


def test_constant_against_per_element(big_walk):
    n = 2 * L + 300
    x = big_walk[:n]
    for c in (0.01, 0.0, -1.0, math.inf):
        want, _ = check(x, [c], name=f"const_vs_per/{c}/const")
        check(x, np.full(n, c), name=f"const_vs_per/{c}/per", want=want)


# ---------------------------------------------------------------------------------------------- the decision rule
def test_strict_comparisons_powers_of_two():
    k = np.concatenate([np.arange(0, 1000), np.arange(1000, -1000, -1), np.arange(-1000, 1000), np.arange(1000, 0, -1)])
    x = 2.0 ** k                                    # returns of exactly +-log(2): the sum reaches the threshold without exceeding it
    thr = [np.log(2.0)]
    want, _ = check(x, thr, name="strict/powers_of_two")
    assert len(x) > L and want[0] == 2 and 1 not in want
    assert np.array_equal(want[:499], np.arange(2, 1000, 2))


def test_strict_comparisons_zero_threshold(orc):
    n = 5 * L + 17
    _, px, _, _ = orc.synth(61, 0, n)
    moves = np.flatnonzero(px[1:] != px[:-1]) + 1
    assert 0.3 * n < len(moves) < 0.7 * n           # runs of equal prices: a >= implementation fires inside them
    want, _ = check(px, [0.0], name="strict/zero")
    assert np.array_equal(want, moves)
    check(px, np.zeros(n), name="strict/zero_per", want=moves)


def test_negative_side_first():
    # the fixture's five-element case: both sides exceed at tick 2; the order of the resets shows at tick 4
    x = np.exp(np.cumsum([0.0, 5.0, -3.0, 0.0, -1.0]))
    thr = np.array([10.0, 10.0, 1.0, 10.0, 2.0])
    assert list(H.cusum_filter(x, thr)) == [2] and list(H.cusum_filter(x, thr, negative_first=False)) == [2, 4]
    check(x, thr, name="priority/five")
    # the same thing many times over, across chunks: thresholds that jump between ticks
    n = 3 * L + 11
    x = walk(n, 33, sigma=0.01)
    thr = np.where(H.hashed_threshold(n, 1.0, True) < 1.25, 0.002, 0.05)  # a tight threshold on one tick in four: it catches both sums
    neg, pos = H.cusum_filter(x, thr), H.cusum_filter(x, thr, negative_first=False)
    assert not np.array_equal(neg, pos) and len(set(pos.tolist()) ^ set(neg.tolist())) >= 10
    check(x, thr, name="priority/walk", want=neg)


def test_odd_values():
    nan, inf = math.nan, math.inf
    n = 3 * L + 100
    x = walk(n, 34)
    rng = np.random.default_rng(35)
    at = rng.choice(np.arange(1, n), 60, replace=False)
    x[at[:20]] = nan
    x[at[20:40]] = 0.0
    x[at[40:]] = -x[at[40:]]
    x[[L - 1, L, L + 1, 2 * L]] = [nan, 0.0, -1.0, nan]                 # ... and on the chunk boundary
    thr = np.full(n, 0.01)
    bt = rng.choice(np.arange(1, n), 90, replace=False)
    thr[bt[:30]] = nan
    thr[bt[30:60]] = -0.5
    thr[bt[60:]] = inf
    thr[[L, L + 1, 2 * L + 1]] = [-1.0, nan, -inf]
    want, _ = check(x, thr, name="odd/both")
    assert len(want) > 100
    check(x, [0.01], name="odd/x")
    check(walk(n, 36), thr, name="odd/thr")
    for c in (nan, inf, -inf):
        want, _ = check(x, [c], name=f"odd/const_{c}")
        assert len(want) == (n - 1 if c == -inf else 0)


def test_negative_constant_fires_on_every_tick():
    n = 2 * L + 50                                   # the densest staging row: 4096 closes in a chunk
    x = walk(n, 37)
    want, _ = check(x, [-0.01], name="odd/negative_const")
    assert np.array_equal(want, np.arange(1, n))
    check(x, np.full(n, -0.01), name="odd/negative_per", want=want)


# ---------------------------------------------------------------------------------------------- tapes that do not forget
def check_fallback(x, thr, name, min_events=0):
    want, d = check(x, thr, name=name)
    assert len(want) >= min_events
    assert d["form"] == 1 and d["pending_first"] > d["chunks"] // 4 + 1, d      # the default call went over to the re-walk
    return want, d


def test_no_forgetting_driftless_no_events():
    want, _ = check_fallback(walk(BIG, 1, sigma=1e-4), [math.inf], "no_forget/driftless_inf")
    assert len(want) == 0


def test_no_forgetting_increasing_prices():
    x = 100.0 * (1.0 + 1e-6) ** np.arange(BIG)       # s_pos never clamps: no chunk ever merges, one round per chunk
    assert np.all(np.diff(x) > 0)
    want, d = check_fallback(x, [math.inf], "no_forget/increasing")
    assert len(want) == 0 and d["launches"] >= d["chunks"] - 1


def test_no_forgetting_wide_threshold():
    # a threshold reached about once per 50 000 ticks; the seed was chosen on the CPU: 10 events under the helper
    want, _ = check_fallback(walk(BIG, 1, sigma=1e-4), [1e-4 * math.sqrt(50_000)], "no_forget/wide", min_events=3)
    assert len(want) == 10


# ---------------------------------------------------------------------------------------------- the C ABI's corners
def test_count_only_and_capacity(big_walk):
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray, c_i64
    ctx = _ffi.default_context()
    n = 2 * L + 300
    x = np.ascontiguousarray(big_walk[:n])
    want = H.cusum_filter(x, [0.01])
    d_x, d_thr = DeviceArray.from_host(ctx, x), DeviceArray.from_host(ctx, np.array([0.01]))
    m, rounds = c_i64(), c_i64()
    ctx.call("fmk_cusum_filter_dev", d_x.p, c_i64(n), d_thr.p, c_i64(1), None, c_i64(0), C.byref(m), C.byref(rounds))
    assert m.value == len(want) and rounds.value >= 1
    out = DeviceArray(ctx, len(want), np.int64)
    m = c_i64()
    rc = ctx.call("fmk_cusum_filter_dev", d_x.p, c_i64(n), d_thr.p, c_i64(1), out.p, c_i64(len(want) - 1), C.byref(m), None,
                  allow=(_ffi.E_CAPACITY,))
    assert rc == _ffi.E_CAPACITY and m.value == len(want)
    ctx.call("fmk_cusum_filter_dev", d_x.p, c_i64(n), d_thr.p, c_i64(1), out.p, c_i64(len(want)), C.byref(m), None)
    assert np.array_equal(out.to_host(), want)
    # the host flavour: count only, and a capacity one too small
    m = c_i64()
    thr = np.array([0.01])
    ctx.call("fmk_cusum_filter", _ffi.ptr(x), c_i64(n), _ffi.ptr(thr), c_i64(1), None, c_i64(0), C.byref(m))
    assert m.value == len(want)
    small = np.empty(len(want) - 1, np.int64)
    with pytest.raises(ValueError, match="capacity"):
        ctx.call("fmk_cusum_filter", _ffi.ptr(x), c_i64(n), _ffi.ptr(thr), c_i64(1), _ffi.ptr(small), c_i64(len(small)), C.byref(m))
    _counts.record("cusum_filter/count_only_capacity", events_compared=len(want))


# ---------------------------------------------------------------------------------------------- resident pipeline
def test_resident_flow(orc):
    """from_numpy -> ewmst sigma -> cusum_filter(10 sigma) -> triple_barrier: the events never leave the device on the way."""
    from finmlkit_amd import engine
    from finmlkit_amd._ffi import DeviceArray, c_i64
    from tests import _label_ref as LR
    n = 200_000
    ts, px, am, sd = orc.synth(71, 0, n)
    t = engine.DeviceTrades.from_numpy(ts, px, am, sd)
    ctx = t.ctx
    sigma = t.ewmst(t.lagged_returns(5.0, True), 60.0)
    thr = 10.0 * sigma.to_host()
    d_thr = DeviceArray.from_host(ctx, thr)
    for form in FORMS:
        with forced(form):
            d_ev = t.cusum_filter(d_thr)
        assert d_ev.dtype == np.int64
        d_tg = DeviceArray(ctx, d_ev.n, np.float64)
        ctx.call("fmk_gather_i64_dev", d_thr.p, c_i64(n), d_ev.p, c_i64(d_ev.n), d_tg.p)       # an 8-byte gather: the bits of 10 sigma
        lab, tch, ret, rat, skipped = t.triple_barrier(d_ev, d_tg, (1.0, 1.0), 60.0, 1.0)
        # ---- now download and compare
        with np.errstate(all="ignore"):
            ev = H.cusum_filter(px, thr)
        assert len(ev) >= 10 and np.array_equal(d_ev.to_host(), ev)
        tg = thr[ev]
        assert np.all(np.isfinite(tg)) and np.array_equal(d_tg.to_host(), tg)
        w = LR.triple_barrier(ts, px, ev, tg, (1.0, 1.0), 60.0, 1.0, None, 0.0)
        assert skipped.to_host()[0] == w[4].sum()
        for g, want in zip((lab, tch, ret, rat), w[:4]):
            assert np.array_equal(g.to_host(), want, equal_nan=want.dtype.kind == "f")
    # a float threshold on another series of the tape's length
    d_series = DeviceArray.from_host(ctx, px[::-1].copy())
    got = t.cusum_filter(2e-5, series=d_series).to_host()
    assert np.array_equal(got, H.cusum_filter(px[::-1], [2e-5])) and len(got) > 10
    _counts.record("cusum_filter/resident", events_compared=len(ev), labels_compared=len(ev))
