"""The encoded-series entropies on the MI355X (csrc/fmk_lz.hip) at the limits of what their entries accept, where tests/test_gpu_lz.py
stops: lookbacks up to 1024 (17 mask words per wave, all 2304 staged codes), planted repeats that stop short of the cap at large lags,
Kontoyiannis windows up to 4096 over several tiles and both slabs of the window walk, plug-in windows up to 4096 with the largest
table and histogram, lengths that end on a tile's edge, and an encode of more elements than one sweep of its grid.  The references,
the comparisons and the bound are those of tests/test_gpu_lz.py: tests/_lz_ref.py, match lengths and codes bit for bit, the estimators
with their NaN positions exactly and their values within TOL = 1e-11, which was derived for 4096 terms -- the limit tested here.  What
the messages are for is asserted on the reference alone in tests/test_lz_host.py."""
import functools

import numpy as np
import pytest

from tests import _lz_ref as R
from tests.test_gpu_lz import bits, close, lz, message, resident

pytestmark = pytest.mark.gpu

TILE = R.TILE                        # positions per workgroup of the match lengths, outputs per wave of the plug-in
MEAN_TILE = 1024                     # outputs per workgroup of the Kontoyiannis mean
MAX_LOOKBACK = 1024


def frozen(a):
    a.setflags(write=False)
    return a


def same_lengths(codes, lookback, want, what):
    got = lz().match_lengths(codes, lookback)
    assert got.dtype == np.uint16 and got.shape == want.shape, what
    wrong = np.flatnonzero(got != want)
    print(f"{what}: {len(wrong)} of {len(want)} match lengths differ")
    assert not len(wrong), (what, wrong[:8], got[wrong[:8]], want[wrong[:8]])
    return got


# ---------------------------------------------------------------------------------------------- A. planted repeats
@functools.lru_cache(maxsize=None)
def planted(lookback):
    codes, plants = R.planted_message(lookback, R.plant_seed(lookback))
    return codes, plants, frozen(R.match_lengths(codes, lookback))


@pytest.mark.parametrize("lookback", (64, 129, 256, 1023, 1024))
def test_planted_repeats_bit_for_bit(lookback):
    codes, plants, want = planted(lookback)
    got = same_lengths(codes, lookback, want, f"planted lookback {lookback} ({len(plants)} plants, {len(codes)} codes)")
    for p, d, r in plants:                                             # (what the reference gives there: tests/test_lz_host.py)
        assert got[p] == 1 + min(r, lookback), (p, d, r)
    assert np.array_equal(resident("match_lengths", codes, lookback), want)


# ---------------------------------------------------------------------------------------------- B. large lookbacks
LARGE = (127, 128, 129, 255, 256, 257, 1023, 1024)
KINDS = ("binary", "16-ary", "constant", "period 65", "k mod 255", "spliced", "invalid")


edge_message = functools.lru_cache(maxsize=None)(R.edge_message)      # (name, lookback): tests/test_lz_host.py says what they hold


@pytest.mark.parametrize("lookback", LARGE)
@pytest.mark.parametrize("name", KINDS)
def test_match_lengths_at_large_lookbacks(name, lookback):
    codes = edge_message(name, lookback)
    same_lengths(codes, lookback, R.match_lengths(codes, lookback), f"{name} lookback {lookback}")


def test_a_message_of_invalid_codes_alone_has_no_match_length():
    """2400 staged 255s: the prefix count reaches 2304 at lookback 1024, and the 255s, which equal each other at every lag, must not
    show in the output"""
    codes = np.full(2400, 255, np.uint8)
    for lookback in (MAX_LOOKBACK, 1023, 64):
        got = lz().match_lengths(codes, lookback)
        assert got.dtype == np.uint16 and got.shape == (2400,) and not got.any(), lookback
    assert not resident("match_lengths", codes, MAX_LOOKBACK).any()


# ---------------------------------------------------------------------------------------------- C. lengths on a tile's edge
def edge_lengths(lookback):
    k = -(-(2 * lookback + 1) // TILE)                                 # the smallest k with 256 k - 1 >= 2 n
    assert TILE * k - 1 >= 2 * lookback > TILE * (k - 1) - 1
    return sorted({2 * lookback - 1, 2 * lookback, 2 * lookback + 1} | {TILE * j + e for j in (k, k + 1) for e in (-1, 0, 1)})


@pytest.mark.parametrize("lookback", (64, MAX_LOOKBACK))
@pytest.mark.parametrize("name", ("binary", "constant"))
def test_lengths_that_end_on_a_tile_edge(name, lookback):
    lengths = edge_lengths(lookback)
    assert len(lengths) == 9
    for n_codes in lengths:
        codes = message(name, n_codes)
        got = same_lengths(codes, lookback, R.match_lengths(codes, lookback), f"{name} lookback {lookback} length {n_codes}")
        assert np.count_nonzero(got) == max(0, n_codes - 2 * lookback + 1), n_codes


# ---------------------------------------------------------------------------------------------- D. Kontoyiannis
KONTO = ((3073, 1), (3074, 1), (3075, 1), (4096, 1),                  # counts 3072 .. 3074: either side of the slab split; 4095
         (2048, 1024), (2049, 1024), (4096, 1024), (4096, 64), (4095, 129))


@pytest.mark.parametrize("shape", KONTO, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("name", ("4-ary", "16-ary"))
def test_kontoyiannis_at_the_window_limit(name, shape):
    window, lookback = shape
    codes = message(name, window + 2 * MEAN_TILE + 300)                # three tiles of the mean, the last one partial
    got = lz().kontoyiannis_entropy(codes, window, lookback)
    close(got, R.kontoyiannis_entropy(codes, window, lookback), window, f"kontoyiannis {name} window {window} lookback {lookback}")
    assert np.array_equal(bits(resident("kontoyiannis_entropy", codes, window, lookback)), bits(got))


def test_kontoyiannis_output_counts_around_a_tile():
    window, lookback = 200, 64
    for outputs in (1, MEAN_TILE - 1, MEAN_TILE, MEAN_TILE + 1, 2 * MEAN_TILE + 1):
        codes = message("16-ary", window - 1 + outputs)
        got = lz().kontoyiannis_entropy(codes, window, lookback)
        close(got, R.kontoyiannis_entropy(codes, window, lookback), window, f"kontoyiannis window {window} lookback {lookback}, {outputs} outputs")


def test_kontoyiannis_nan_windows_at_the_window_limit():
    window, lookback, at = R.KONTO_NAN
    codes = message("invalid", 4 * window, None, at)
    want = np.zeros(len(codes), bool)
    want[:window - 1] = True
    for i in at:
        want[i:i + window] = True
    got = lz().kontoyiannis_entropy(codes, window, lookback)
    assert np.array_equal(np.isnan(got), want)
    close(got, R.kontoyiannis_entropy(codes, window, lookback), window, f"kontoyiannis invalid window {window} lookback {lookback}")


# ---------------------------------------------------------------------------------------------- E. plug-in
PLUGIN = ((4096, 1, 2), (4096, 12, 2), (4096, 1, 255), (4096, 2, 64), (4095, 3, 16), (4096, 4, 8))


@functools.lru_cache(maxsize=None)
def random_codes(alphabet, n_codes):
    m = np.random.default_rng(1900 + alphabet).integers(0, alphabet, n_codes).astype(np.uint8)
    m[n_codes // 2] = alphabet - 1                                     # the last code of the alphabet is there (254 of 255)
    return frozen(m)


@pytest.mark.parametrize("shape", PLUGIN, ids=lambda s: "-".join(map(str, s)))
def test_plugin_entropy_at_the_window_limit(shape):
    window, word, alphabet = shape
    codes = random_codes(alphabet, window + 2 * TILE + 77)             # two runs of 256 outputs and a partial one
    assert codes.max() == alphabet - 1 and len(set(codes)) == alphabet
    got = lz().plugin_entropy(codes, window, word, alphabet)
    close(got, R.plugin_entropy(codes, window, word, alphabet), window, f"plug-in window {window} word {word} alphabet {alphabet}")
    assert np.array_equal(bits(resident("plugin_entropy", codes, window, word, alphabet)), bits(got))


@pytest.mark.parametrize("word", (1, 12))
def test_plugin_entropy_of_a_constant_message_at_the_window_limit(word):
    codes = message("constant", 4096 + 2 * TILE + 77)
    got = lz().plugin_entropy(codes, 4096, word, 2)
    assert np.isnan(got[:4095]).all() and np.array_equal(bits(got[4095:]), bits(np.zeros(len(codes) - 4095)))     # exactly +0.0


def test_plugin_output_counts_around_a_wave_and_a_run():
    window, word, alphabet = 64, 2, 2
    for outputs in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        codes = message("binary", window - 1 + outputs)
        got = lz().plugin_entropy(codes, window, word, alphabet)
        close(got, R.plugin_entropy(codes, window, word, alphabet), window, f"plug-in window {window} word {word}, {outputs} outputs")


def test_plugin_invalid_code_at_a_run_boundary():
    """the last output of the first run (t = window - 1 + 255) and the first of the second: the word that enters there is invalid"""
    window, word, alphabet = 300, 3, 2
    for i, code in ((window - 1 + TILE - 1, 2), (window - 1 + TILE, 255)):
        codes = message("binary", window + 3 * TILE).copy()
        codes[i] = code
        want = np.zeros(len(codes), bool)
        want[:window - 1] = True
        want[i:i + window] = True
        got = lz().plugin_entropy(codes, window, word, alphabet)
        assert np.array_equal(np.isnan(got), want), i
        close(got, R.plugin_entropy(codes, window, word, alphabet), window, f"plug-in window {window} word {word}, code {code} at {i}")


# ---------------------------------------------------------------------------------------------- F. encode
ENCODE_N = 3 * 2 ** 20 + 777         # the grid is at most 16 blocks of 256 per compute unit: more than one sweep up to 768 of them


@functools.lru_cache(maxsize=None)
def encode_series():
    return frozen(np.random.default_rng(1898).normal(0.0, 1.0, ENCODE_N))


@pytest.mark.parametrize("n_edges", (9, 254))
def test_encode_beyond_one_sweep_of_the_grid(n_edges):
    rng = np.random.default_rng(1899 + n_edges)
    edges = np.cumsum(rng.uniform(0.01, 6.0 / n_edges, n_edges)) - 3.0
    x = encode_series().copy()
    kinds = [np.nan, np.inf, -np.inf, edges[n_edges // 2], np.nextafter(edges[n_edges // 2], -np.inf)]
    want_kinds = [255, n_edges, 0, n_edges // 2 + 1, n_edges // 2]
    anchors = (0, 2 ** 20 - 1, 2 ** 20, ENCODE_N - 1)
    for j, (anchor, first) in enumerate(zip(anchors, (0, 2 ** 20 - 5, 2 ** 20, ENCODE_N - 5))):
        order = np.roll(np.arange(5), anchor - first - j)             # the five kinds around the anchor, kind j on the anchor itself
        x[first:first + 5] = np.array(kinds)[order]
        assert order[anchor - first] == j
    want = np.searchsorted(edges, x, side="right").astype(np.uint8)
    want[np.isnan(x)] = 255
    for j, anchor in enumerate(anchors):
        assert want[anchor] == want_kinds[j]
    assert len(np.unique(want)) == n_edges + 2                               # every code and 255
    got = lz().encode(x, edges)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (n_edges, np.flatnonzero(got != want)[:8])
    assert np.array_equal(resident("encode", x, edges), want)
