"""GPU tests of the price grid (csrc/fmk_common.h, fmk_price_grid_build_dev, the grid instantiations of k_bar_ohlcv_small).

A tape whose every price is reproduced bit for bit from an int32 k carries k as a fifth column; the 1-minute OHLCV kernel then reads
4 B per tick of it instead of the float64 price.  Three things are checked:
  certificate  form, scale and column against the host for tapes that must certify (k * 0.01: form A; np.round(x, d): form B) and
               tapes that must not (full mantissas, one off-grid tick, -0.0, NaN, inf, k beyond int32);
  parity       every output of time_bars_ohlcv and bar_ohlcv bitwise equal with the context's switch on and off, for both forms, on
               bar lengths that take every code path of the kernel's size classes -- and the last-call counter says that the grid
               kernel really ran (no case passes on the float64 path alone);
  carrier      which DeviceTrades carry a grid: from_numpy and synth do, a hand-built one and a with_halo view do not, place() keeps
               it at every position.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ["open", "high", "low", "close", "volume", "vwap", "trades", "median_trade_size"]
NONE, A, B = 0, 1, 2
T0 = 1_700_000_040_000_000_000            # a whole minute
MIN = 60_000_000_000


@pytest.fixture(scope="module")
def eng():
    from finmlkit_amd import engine
    return engine


@pytest.fixture(scope="module")
def ctx():
    from finmlkit_amd import _ffi
    return _ffi.default_context()


@pytest.fixture(autouse=True)
def _switch_back_on(ctx):
    yield
    ctx.set_price_grid(True)


def _tape(eng, px):
    px = np.asarray(px, np.float64)
    n = len(px)
    return eng.DeviceTrades.from_numpy(T0 + np.arange(n, dtype=np.int64) * 1_000_000, px, np.ones(n, np.float32))


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _grid_prices(form, n, seed, d=2):
    rng = np.random.default_rng(seed)
    if form == A:
        return (10_000 + np.cumsum(rng.integers(-3, 4, n))) * 0.01
    return np.round(rng.uniform(10.0, 1000.0, n), d)


# ---------------------------------------------------------------------------------------------------------------- certificate
N_CERT = 10_007             # odd; the sample reads every 78th tick and the last one, so index 5 is seen by the full pass alone


@pytest.mark.parametrize("case", ["k*0.01", "round2", "round5", "negative", "n=1"])
def test_certifies(eng, case):
    rng = np.random.default_rng(3)
    if case == "k*0.01":
        k = 10_000 + np.cumsum(rng.integers(-3, 4, N_CERT))
        px, form, d = k * 0.01, A, 2
    elif case == "round2":
        px, form, d = np.round(rng.uniform(10.0, 1000.0, N_CERT), 2), B, 2
    elif case == "round5":
        px, form, d = np.round(rng.uniform(10.0, 1000.0, N_CERT), 5), B, 5
    elif case == "negative":
        k = np.cumsum(rng.integers(-3, 4, N_CERT)) - 7          # both signs, zero among them
        px, form, d = k * 0.01, A, 2
        assert (k < 0).any() and (k > 0).any()
    else:
        px, d = np.array([101.27]), 2
        form = A if _bits(10127 * 0.01) == _bits(px[0]) else B
    t = _tape(eng, px)
    assert t.price_k is not None and t.price_grid is not None, case
    g = t.price_grid
    assert (g.form, g.d) == (form, d), (case, g.form, g.d)
    assert g.s == 10.0 ** d and g.r == float("1e-%d" % d)
    k_dev = t.price_k.to_host()
    assert k_dev.dtype == np.int32 and len(k_dev) == len(px)
    np.testing.assert_array_equal(k_dev, np.rint(px * 10.0 ** d).astype(np.int64), err_msg=case)
    # the host's own decode of the device's column gives the price's bits
    kd = k_dev.astype(np.float64)
    host = kd * g.r if form == A else kd / 10 ** d
    np.testing.assert_array_equal(_bits(host), _bits(px), err_msg=case)
    if form == B and len(px) > 1:
        assert (_bits(kd * g.r) != _bits(px)).any(), "the tape would have certified under form A"


@pytest.mark.parametrize("case", ["full mantissa", "off-grid first", "off-grid last", "off-grid unsampled", "-0.0", "nan", "inf",
                                  "beyond int32"])
def test_refuses(eng, case):
    rng = np.random.default_rng(4)
    px = (10_000 + np.cumsum(rng.integers(-3, 4, N_CERT))) * 0.01
    if case == "full mantissa":
        px = rng.uniform(10.0, 1000.0, N_CERT)
    elif case == "off-grid first":
        px[0] = np.nextafter(px[0], np.inf)
    elif case == "off-grid last":
        px[-1] = np.nextafter(px[-1], np.inf)
    elif case == "off-grid unsampled":
        px[5] = np.nextafter(px[5], -np.inf)
    elif case == "-0.0":
        px = (np.cumsum(rng.integers(-3, 4, N_CERT))) * 0.01
        px[5] = -0.0
    elif case == "nan":
        px[5] = np.nan
    elif case == "inf":
        px[5] = np.inf
    else:
        px = px + 30_000_000.0                                    # k = 3e9 at d = 2
        px[5] = 30_000_000.25
    t = _tape(eng, px)
    assert t.price_k is None and t.price_grid is None, case


# ---------------------------------------------------------------------------------------------------------------- parity
def _bar_lengths():
    """One round of bar lengths that takes every path of the 21-chunk kernel: the exact classes 11 .. 21, the generic classes of
    <= 1, <= 4, <= 10 and <= 16 chunks, each at a chunk edge - 1, + 0, + 1; the longest bar the kernel takes and the first it leaves to
    the long-bar kernels; empty bars."""
    ls = [1, 63, 64, 65, 0]
    for c in (2, 4, 10, 11, 17, 18, 19, 20, 21):
        ls += [64 * c - 1, 64 * c, 64 * c + 1]
    ls += [0, 0, 1344, 1345, 12 * 64 + 7, 16 * 64 - 5]
    return ls


ROUNDS = 64                               # ~2 400 bars, ~1.7e6 ticks: the first stage of the pipelined step gets 256 bars
_CACHE = {}


def _parity_tape(eng, form):
    """(ts, px, am, lengths): minute m of the tape holds lengths[m] ticks strictly inside it; the tape ends on a bar's last tick."""
    if form not in _CACHE:
        ls = np.array(_bar_lengths() * ROUNDS, np.int64)
        assert ls[-1] > 0
        n = int(ls.sum())
        ts = np.empty(n, np.int64)
        at = 0
        for m, L in enumerate(ls):
            if L:
                ts[at:at + L] = T0 + m * MIN + (np.arange(1, L + 1, dtype=np.int64) * (MIN // (L + 2)))
                at += L
        rng = np.random.default_rng(21 + form)
        px = _grid_prices(form, n, 5 + form)
        am = (rng.integers(1, 1 << 20, n) / 1024.0).astype(np.float32)
        _CACHE[form] = (ts, px, am, ls)
    return _CACHE[form]


def _same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if x.dtype.kind == "f":
            np.testing.assert_array_equal(x.view(np.uint64 if x.itemsize == 8 else np.uint32),
                                          y.view(np.uint64 if y.itemsize == 8 else np.uint32), err_msg=f"{what}: {k}")
        else:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {k}")


@pytest.mark.parametrize("form", [A, B])
def test_time_bars_parity(eng, ctx, orc, monkeypatch, form):
    monkeypatch.setenv("FMK_TB_PIPE_MIN_STAGE", "256")
    ts, px, am, ls = _parity_tape(eng, form)
    t = eng.DeviceTrades.from_numpy(ts, px, am)
    assert t.price_grid is not None and t.price_grid.form == form
    oclock, oci = orc._time_bar_indexer(ts, 60.0)
    got_ls = np.diff(oci)
    assert set(_bar_lengths()) <= set(got_ls.tolist()), "the tape does not hold the bar lengths it was built for"
    assert oci[-1] == len(ts) - 1 and got_ls[-1] > 0                  # the last bar ends on the tape's last tick
    assert (len(oci) - 1) // 8 >= 256 and len(ts) // (len(oci) - 1) > 600     # the pipelined step
    for want_median in (True, False):
        res = {}
        for on in (True, False):
            ctx.set_price_grid(on)
            clock, idx, o = t.time_bars_ohlcv(60.0, want_median)
            launches = ctx.ohlcv_grid_launches()
            assert launches == (2 if on else 0), (form, want_median, on, launches)
            res[on] = dict(eng.to_host(o), clock=clock.to_host(), close_idx=idx.to_host())
        _same(res[True], res[False], f"form {form}, median {want_median}")
        np.testing.assert_array_equal(res[True]["close_idx"], oci)
        np.testing.assert_array_equal(res[True]["clock"], oclock)


@pytest.mark.parametrize("form", [A, B])
def test_bar_ohlcv_parity(eng, ctx, orc, form):
    ts, px, am, ls = _parity_tape(eng, form)
    t = eng.DeviceTrades.from_numpy(ts, px, am)
    ci_h = np.concatenate([[-1], np.cumsum(ls) - 1]).astype(np.int64)          # hand-built: empty bars repeat an index
    assert ci_h[-1] == len(ts) - 1
    from finmlkit_amd._ffi import DeviceArray
    ci = DeviceArray.from_host(ctx, ci_h)
    for want_median in (True, False):
        res = {}
        for on in (True, False):
            ctx.set_price_grid(on)
            o = t.bar_ohlcv(ci, want_median)
            launches = ctx.ohlcv_grid_launches()
            assert launches == (1 if on else 0), (form, want_median, on, launches)
            res[on] = eng.to_host(o)
        _same(res[True], res[False], f"form {form}, median {want_median}")
    # a tape that does not certify never reads a grid, whatever the switch says
    px2 = px.copy()
    px2[len(px2) // 2] = np.nextafter(px2[len(px2) // 2], np.inf)
    t2 = eng.DeviceTrades.from_numpy(ts, px2, am)
    assert t2.price_k is None
    ctx.set_price_grid(True)
    t2.bar_ohlcv(ci)
    assert ctx.ohlcv_grid_launches() == 0


def test_small_case_against_oracle(eng, ctx, orc):
    ts, px, am, ls = _parity_tape(eng, A)
    n_bars = len(_bar_lengths())                                       # one round
    n = int(ls[:n_bars].sum())
    t = eng.DeviceTrades.from_numpy(ts[:n], px[:n], am[:n])
    ci_h = np.concatenate([[-1], np.cumsum(ls[:n_bars]) - 1]).astype(np.int64)
    from finmlkit_amd._ffi import DeviceArray
    got = eng.to_host(t.bar_ohlcv(DeviceArray.from_host(ctx, ci_h)))
    assert ctx.ohlcv_grid_launches() == 1
    want = orc.comp_bar_ohlcv(px[:n], am[:n], ci_h)
    for k, w in zip(FIELDS, want):
        if k == "vwap":
            np.testing.assert_allclose(got[k], w, rtol=1e-9, err_msg=k)      # a reassociated float64 sum (DESIGN: 1e-9 relative)
        else:
            np.testing.assert_array_equal(got[k], w, err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- carrier
def test_carriers(eng, ctx):
    n = 200_000
    t = eng.DeviceTrades.synth(n, seed=9)
    assert t.price_grid is not None and t.price_grid.form == A and t.price_grid.d == 2
    ref = eng.to_host(t.time_bars_ohlcv(60.0)[2])
    assert ctx.ohlcv_grid_launches() > 0
    # built by hand: the constructor cannot know that the price column is final
    hand = eng.DeviceTrades(ctx, t.ts, t.price, t.amount, t.side)
    assert hand.price_k is None and hand.price_grid is None
    _same(eng.to_host(hand.time_bars_ohlcv(60.0)[2]), ref, "hand-built")
    assert ctx.ohlcv_grid_launches() == 0
    assert t.without_grid().price_k is None and t.price_k is not None
    # a shard with head-room and its with_halo view: the halo elements are written later
    sh = eng.DeviceTrades.synth(n, seed=9, headroom=64)
    assert sh.price_k is None
    _same(eng.to_host(sh.time_bars_ohlcv(60.0)[2]), ref, "head-room")
    assert ctx.ohlcv_grid_launches() == 0
    halo = sh.with_halo(16)                                             # 16 more ticks in front; the bars start behind them
    assert halo.price_k is None and halo.n == n + 16
    _, ci = sh.time_bar_index(60.0)
    from finmlkit_amd._ffi import DeviceArray
    got = eng.to_host(halo.bar_ohlcv(DeviceArray.from_host(ctx, ci.to_host() + 16)))
    assert ctx.ohlcv_grid_launches() == 0
    _same(got, ref, "with_halo view")


def test_place_keeps_the_grid(eng, ctx):
    n = 200_000
    t = eng.DeviceTrades.synth(n, seed=9)
    ref = eng.to_host(t.time_bars_ohlcv(60.0)[2])
    seen = []

    def probe(p):
        got = eng.to_host(p.time_bars_ohlcv(60.0)[2])
        seen.append((id(p), p.price_k is not None and p.price_grid.form == A, ctx.ohlcv_grid_launches()))
        _same(got, ref, "a placed position")
        if p is not t:
            np.testing.assert_array_equal(p.price_k.to_host(), t.price_k.to_host())
            assert p.price_k.ptr != t.price_k.ptr

    chosen, info = t.place(probe, positions=2, reps=1, warm=0)
    assert len({s[0] for s in seen}) == 2, "place() probed position 0 only"
    assert all(s[1] and s[2] > 0 for s in seen), seen
    assert chosen.price_k is not None and chosen.price_grid.form == A
    _same(eng.to_host(chosen.time_bars_ohlcv(60.0)[2]), ref, "the chosen position")
    assert ctx.ohlcv_grid_launches() > 0
