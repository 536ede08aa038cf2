"""The encoded-series entropies on the MI355X (csrc/fmk_lz.hip) against tests/_lz_ref.py: the match lengths and the codes bit for
bit; the two estimators with their NaN positions exactly and their values within 1e-11 absolute.  That
bound is derived, not measured: at most 4096 terms, each below log2(1025) ~ 10 bits, summed in float64, lose less than
4096 * 2^-53 * 10 ~ 4.5e-12; 1e-11 leaves a factor of two for the device's log2.  Messages are 1100 codes long: more than four
256-position tiles of the match-length kernel, more than four 256-output runs of the plug-in kernel."""
import functools
import json
import math
import os

import numpy as np
import pandas as pd
import pytest

from tests import _lz_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1100
TILE = 256                           # positions per workgroup of the match lengths, outputs per wave of the plug-in (csrc/fmk_lz.hip)
LOOKBACKS = (1, 3, 63, 64, 65, 200)  # 63 / 64 / 65: where a wave's lag takes one mask word more
TOL = 1e-11
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "lz.json")))


@functools.lru_cache(maxsize=None)
def message(name, n_codes=N, stretch=None, invalid_at=None):
    """The seeded messages (tests/_lz_ref.py), shared by the tests here and in tests/test_gpu_lz_edges.py (never written to).
    At the defaults: 1100 codes, "spliced" with a constant stretch of 300 across the edge of tiles 0 and 1, "invalid" with three
    invalid codes, one at a tile's first element."""
    return R.message(name, n_codes, stretch, invalid_at)


MESSAGES = ("binary", "16-ary", "constant", "period 2", "period 65", "k mod 255", "spliced", "invalid")


@functools.lru_cache(maxsize=None)
def lam_ref(name, lookback):
    out = R.match_lengths(message(name), lookback)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def konto_ref(name, window, lookback):
    out = R.kontoyiannis_entropy(message(name), window, lookback)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def plugin_ref(name, window, word, alphabet):
    out = R.plugin_entropy(message(name), window, word, alphabet)
    out.setflags(write=False)
    return out


def lz():
    from finmlkit_amd.feature.core import lz as P
    return P


def ctx_():
    from finmlkit_amd import _ffi
    return _ffi.default_context()


def resident(function, host_array, *args):
    from finmlkit_amd._ffi import DeviceArray
    return lz().resident(ctx_(), function, DeviceArray.from_host(ctx_(), host_array), *args).to_host()


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def close(got, want, window, what):
    """NaN positions exactly, values within TOL; the reference is finite in at least half of the full windows"""
    full = want[window - 1:]
    assert np.isnan(want[:window - 1]).all() and 2 * int(np.isfinite(full).sum()) >= len(full) > 0, what
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = np.isfinite(want)
    err = float(np.abs(got[ok] - want[ok]).max())
    print(f"{what}: max |error| {err:.3e} over {int(ok.sum())} finite outputs")
    assert err <= TOL, (what, err)


# ---------------------------------------------------------------------------------------------- match lengths
@pytest.mark.parametrize("lookback", LOOKBACKS)
@pytest.mark.parametrize("name", MESSAGES)
def test_match_lengths_bit_for_bit(name, lookback):
    want = lam_ref(name, lookback)
    got = lz().match_lengths(message(name), lookback)
    assert got.dtype == np.uint16 and np.array_equal(got, want), (name, lookback, np.flatnonzero(got != want)[:8])


def test_the_match_length_cases_cover_what_they_are_for():
    for n in LOOKBACKS:
        assert (lam_ref("constant", n)[n:N - n + 1] == n + 1).all()                          # the cap n + 1 is reached
        assert (lam_ref("k mod 255", n)[n:N - n + 1] == 1).all()                             # and no match at all
        if n >= 2:
            assert (lam_ref("period 2", n)[n:N - n + 1] == n + 1).all()                      # lag 2 < the run: a match runs over p itself
        lam = lam_ref("binary", n)
        assert lam[N - n] > 0 and not lam[N - n + 1:].any() and not lam[:n].any() and lam[n] > 0     # the last and the first valid p
        bad = lam_ref("invalid", n)
        zero = np.zeros(N, bool)
        zero[:n], zero[N - n + 1:] = True, True
        for i in (3, 4 * TILE, N - 1):
            zero[max(0, i - n + 1):i + n + 1] = True
        assert np.array_equal(bad == 0, zero), n
    sp = lam_ref("spliced", 200)
    # (the stretch is codes[106 .. 406): from p = 200, the first valid one, to 206 it holds 200 matches at lag 1; then fewer and fewer)
    assert sp[200:TILE + 150 - 200 + 1].min() == 201 and 1 < sp[TILE + 149] < 201 and len(set(sp[TILE - 8:TILE + 8])) > 1
    sp = lam_ref("spliced", 64)
    assert (sp[TILE - 150 + 1:TILE + 150 - 64 + 1] == 65).all() and sp[TILE + 140:TILE + 150].max() < 65
    assert len(set(lam_ref("16-ary", 65)[65:N - 65])) >= 3 and len(set(lam_ref("binary", 200)[200:N - 200])) >= 5


@pytest.mark.parametrize("lookback", (1, 64, 200))
def test_a_message_shorter_than_two_lookbacks_has_no_match_length(lookback):
    for n_codes in (1, lookback, 2 * lookback - 1):
        got = lz().match_lengths(message("binary")[:n_codes], lookback)
        assert got.shape == (n_codes,) and not got.any()
    got = lz().match_lengths(message("binary")[:2 * lookback], lookback)                         # N == 2 n: one position
    assert np.array_equal(got, R.match_lengths(message("binary")[:2 * lookback], lookback)) and np.count_nonzero(got) == 1


# ---------------------------------------------------------------------------------------------- Kontoyiannis
def konto_windows(n):
    return sorted({2 * n, 2 * n + 1, 3 * n})


@pytest.mark.parametrize("lookback", LOOKBACKS)
@pytest.mark.parametrize("name", ("binary", "16-ary", "spliced", "invalid", "period 65"))
def test_kontoyiannis_against_the_reference(name, lookback):
    for window in konto_windows(lookback):
        got = lz().kontoyiannis_entropy(message(name), window, lookback)
        close(got, konto_ref(name, window, lookback), window, f"kontoyiannis {name} window {window} lookback {lookback}")


def test_kontoyiannis_nan_is_the_windows_that_read_an_invalid_code():
    for window, lookback in ((2, 1), (7, 3), (128, 64), (600, 200)):
        want = np.zeros(N, bool)
        want[:window - 1] = True
        for i in (3, 4 * TILE, N - 1):
            want[i:i + window] = True
        got = lz().kontoyiannis_entropy(message("invalid"), window, lookback)
        assert np.array_equal(np.isnan(got), want), (window, lookback)
    assert np.isnan(lz().kontoyiannis_entropy(message("binary")[:127], 128, 64)).all()           # no full window


@pytest.mark.parametrize("case", GOLDEN["kontoyiannis"], ids=lambda c: f"{c['message']}-{c['lookback']}-{c['window']}")
def test_kontoyiannis_closed_forms(case):
    n, w = case["lookback"], case["window"]
    codes = R.golden_message(case, N)
    assert (lz().match_lengths(codes, n)[n:N - n + 1] == case["match_length"]).all()
    got = lz().kontoyiannis_entropy(codes, w, n)
    assert np.isnan(got[:w - 1]).all() and float(np.abs(got[w - 1:] - case["value"]).max()) <= TOL
    assert len(set(bits(got[w - 1:]))) == 1                                                    # the same sum at every output


# ---------------------------------------------------------------------------------------------- plug-in
PLUGIN = [("binary", 2, ((1, 1), (2, 2), (12, 12), (64, 1), (64, 2), (129, 3), (600, 10), (TILE, 4), (TILE + 1, 4))),
          ("16-ary", 16, ((1, 1), (3, 3), (64, 1), (65, 2), (200, 3))),
          ("invalid", 3, ((1, 1), (7, 7), (64, 2), (129, 3), (400, 7))),
          ("over", 2, ((2, 2), (64, 2), (200, 5))),
          ("constant", 2, ((1, 1), (64, 2), (600, 12)))]


@pytest.mark.parametrize("name,alphabet,shapes", PLUGIN, ids=[p[0] for p in PLUGIN])
def test_plugin_entropy_against_the_reference(name, alphabet, shapes):
    for window, word in shapes:
        got = lz().plugin_entropy(message(name), window, word, alphabet)
        want = plugin_ref(name, window, word, alphabet)
        close(got, want, window, f"plug-in {name} window {window} word {word} alphabet {alphabet}")
        if window == word or name == "constant":
            assert (got[np.isfinite(got)] == 0.0).all()                                        # one word: exactly 0.0
    want = np.zeros(N, bool)
    want[:63] = True
    want[300:302 + 63] = True
    assert np.array_equal(np.isnan(lz().plugin_entropy(message("over"), 64, 2, 2)), want)      # 2 and 200 are invalid at alphabet 2
    want[300:302 + 63] = False
    assert np.array_equal(np.isnan(lz().plugin_entropy(message("over"), 64, 1, 201)), want)    # and codes at alphabet 201


@pytest.mark.parametrize("case", GOLDEN["plugin"], ids=lambda c: f"{c['message']}-{c['window']}-{c['word']}")
def test_plugin_closed_forms(case):
    w = case["window"]
    codes = R.golden_message(case, max(N, w + 70))
    got = lz().plugin_entropy(codes, w, case["word"], case["alphabet"])
    assert np.isnan(got[:w - 1]).all()
    if case["message"] == "constant":
        assert np.array_equal(bits(got[w - 1:]), bits(np.zeros(len(codes) - w + 1)))           # exactly +0.0
    else:
        assert float(np.abs(got[w - 1:] - case["value"]).max()) <= TOL


# ---------------------------------------------------------------------------------------------- encode
def test_encode_is_searchsorted_bit_for_bit():
    rng = np.random.default_rng(1899)
    for n_edges in (1, 2, 9, 254):
        edges = np.cumsum(rng.uniform(0.01, 1.0, n_edges)) - 0.4 * n_edges
        x = rng.normal(0.0, 0.3 * n_edges, N)
        x[:n_edges] = edges                                                                    # values equal to an edge
        x[n_edges:2 * n_edges] = np.nextafter(edges, -np.inf)                                  # and one ulp below
        x[[N - 1, N - 2, N - 3, N - 4, N - 5]] = [np.inf, -np.inf, np.nan, -0.0, 0.0]
        want = np.searchsorted(edges, x, side="right").astype(np.uint8)
        want[np.isnan(x)] = 255
        got = lz().encode(x, edges)
        assert got.dtype == np.uint8 and np.array_equal(got, want), n_edges
        assert got[N - 1] == n_edges and got[N - 2] == 0 and got[N - 3] == 255 and got[N - 4] == got[N - 5]
        assert np.array_equal(resident("encode", x, edges), want)
    assert np.array_equal(lz().encode([-1.0, -0.0, 0.0, 2.0, np.nan], lz().binary_edges()), [0, 1, 1, 1, 255])


# ---------------------------------------------------------------------------------------------- the routes
def test_every_route_gives_the_same_bits():
    from finmlkit_amd import engine
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.feature import transforms as T
    from finmlkit_amd.feature.core.utils import comp_lagged_returns
    P, ctx = lz(), ctx_()
    trades = engine.DeviceTrades.synth(N, seed=18, ctx=ctx)
    ts, price = trades.ts.to_host(), trades.price.to_host()
    ret = comp_lagged_returns(ts, price, 1e-6, False)
    edges = P.quantile_edges(ret, 4)
    codes = P.encode(ret, edges)
    assert np.array_equal(codes == 255, np.isnan(ret)) and len(set(codes) - {255}) >= 2
    d_codes = trades.encode(DeviceArray.from_host(ctx, ret), edges)
    assert d_codes.dtype == np.uint8 and np.array_equal(d_codes.to_host(), codes)
    frame = pd.DataFrame({"price": price}, index=pd.to_datetime(ts))
    step = T.ReturnT(pd.Timedelta(seconds=1e-6), input_col="price")
    flat = pd.DataFrame({"ret1": ret}, index=frame.index)
    for name, args, method, transform in (
            ("plugin_entropy", (64, 2, len(edges) + 1), trades.plugin_entropy, T.PluginEntropy(64, 2, edges=edges)),
            ("kontoyiannis_entropy", (64, 16), trades.kontoyiannis_entropy, T.KontoyiannisEntropy(64, 16, edges=edges))):
        host = getattr(P, name)(codes, *args)
        assert np.isnan(host[:63]).all() and 2 * int(np.isfinite(host).sum()) > N and len(set(host[np.isfinite(host)])) > 20
        routes = {"host again": getattr(P, name)(codes, *args), "_dev": resident(name, codes, *args),
                  "DeviceTrades": method(d_codes, *args).to_host(), "transform": transform(flat).values,
                  "Compose": T.Compose(step, transform)(frame).values}
        for route, got in routes.items():
            assert np.array_equal(bits(got), bits(host)), (name, route)
        q = type(transform)(64, args[1], edges=4)                                              # an int: quantile_edges(column, 4)
        assert np.array_equal(bits(q(flat).values), bits(host)) and q.output_name == transform.output_name
        with pytest.raises(ValueError) as e:
            T.Compose(step, q)(frame)
        assert "quantile_edges" in str(e.value)
    lam = P.match_lengths(codes, 16)
    assert np.array_equal(trades.match_lengths(d_codes, 16).to_host(), lam) and np.array_equal(resident("match_lengths", codes, 16), lam)
    assert np.array_equal(P.match_lengths(codes, 16), lam)
