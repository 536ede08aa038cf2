"""CPU-only: the encoded-series entropies (finmlkit_amd/feature/core/lz.py) without a device.  The book's
snippets 18.1, 18.3 and 18.4 restated on tuples against the per-lag NumPy form of tests/_lz_ref.py that the GPU tests compare with;
the edge helpers; what the functions refuse, in Python without the library and in both C flavours with a null context; the calls that
need no context; the exports and the transforms; the closed forms of tests/golden/lz.json; and the header of the rules on the host."""
import json
import math
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from finmlkit_amd import _ffi
from finmlkit_amd.feature import core
from finmlkit_amd.feature import transforms as T
from finmlkit_amd.feature.core import lz as P
from tests import _lz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = math.nan, math.inf
PAIRS = ((1, 2), (3, 6), (4, 11), (8, 16), (8, 40), (20, 41))        # (lookback, window)
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "lz.json")))


def messages(n=90):
    rng = np.random.default_rng(1801)
    return {"constant": np.full(n, 2, np.uint8), "period 3": (np.arange(n) % 3).astype(np.uint8),
            "random 2": rng.integers(0, 2, n).astype(np.uint8), "random 3": rng.integers(0, 3, n).astype(np.uint8),
            "random 16": rng.integers(0, 16, n).astype(np.uint8)}


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


# ---------------------------------------------------------------------------------------------- the two forms of the reference
@pytest.mark.parametrize("name", list(messages()))
def test_the_literal_and_the_per_lag_forms_agree(name):
    codes = messages()[name]
    for lookback, window in PAIRS:
        lam = R.match_lengths(codes, lookback)
        assert lam.dtype == np.uint16 and lam.max() <= lookback + 1
        for p in range(len(codes)):
            want = R.match_length(tuple(int(c) for c in codes), p, lookback) if lookback <= p <= len(codes) - lookback else 0
            assert lam[p] == want, (name, lookback, p)
        a, b = R.konto_literal(codes, window, lookback), R.kontoyiannis_entropy(codes, window, lookback)
        assert same_nan(a, b) and np.isnan(a[:window - 1]).all() and np.isfinite(a[window - 1:]).all()
        assert np.nanmax(np.abs(a - b)) < 1e-13, (name, lookback, window)
    alphabet = int(codes.max()) + 1 if name != "constant" else 3
    for window, word in ((1, 1), (2, 2), (11, 1), (11, 2), (40, 3), (41, 1)):
        a, b = R.plugin_literal(codes, window, word, alphabet), R.plugin_entropy(codes, window, word, alphabet)
        assert same_nan(a, b) and np.isfinite(a[window - 1:]).all()
        assert np.nanmax(np.abs(a - b)) < 1e-13, (name, window, word)


def test_an_invalid_code_takes_the_windows_that_read_it_in_both_forms():
    codes = messages()["random 3"].copy()
    codes[[0, 37, 38, 89]] = [255, 255, 7, 255]                      # 7: invalid for the plug-in at alphabet 3 alone
    for lookback, window in PAIRS:
        want = np.zeros(90, bool)
        want[:window - 1] = True
        for i in (0, 37, 89):
            want[i:i + window] = True
        a, b = R.konto_literal(codes, window, lookback), R.kontoyiannis_entropy(codes, window, lookback)
        assert np.array_equal(np.isnan(a), want) and np.array_equal(np.isnan(b), want), (lookback, window)
    want = np.zeros(90, bool)
    want[:10] = True
    for i in (0, 37, 38, 89):
        want[i:i + 11] = True
    a, b = R.plugin_literal(codes, 11, 2, 3), R.plugin_entropy(codes, 11, 2, 3)
    assert np.array_equal(np.isnan(a), want) and np.array_equal(np.isnan(b), want)
    assert np.nanmax(np.abs(a - b)) < 1e-13


def test_codes_of_two_digits_are_codes_not_strings():
    """(1, 0) and (10,) are one string to ''.join(map(str, ..)); on tuples they are two words"""
    assert R.pmf1((1, 0, 10, 1, 0), 1) == {(1,): 0.4, (0,): 0.4, (10,): 0.2}
    assert R.match_length((1, 0, 10, 1, 0, 10), 3, 3) == 4 and R.match_length((1, 0, 10, 10, 1, 0), 3, 3) == 2


# ---------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("case", GOLDEN["kontoyiannis"], ids=lambda c: f"{c['message']}-{c['lookback']}-{c['window']}")
def test_kontoyiannis_closed_forms_on_the_reference(case):
    n, w = case["lookback"], case["window"]
    codes = R.golden_message(case, w + 150)
    lam = R.match_lengths(codes, n)
    assert (lam[n:len(codes) - n + 1] == case["match_length"]).all() and not lam[:n].any() and not lam[len(codes) - n + 1:].any()
    want = math.log2(n + 1) / (n + 1) if case["message"] != "ramp" else math.log2(n + 1)
    assert case["value"] == want
    h = R.kontoyiannis_entropy(codes, w, n)
    assert np.isnan(h[:w - 1]).all() and np.abs(h[w - 1:] - want).max() < 1e-13


@pytest.mark.parametrize("case", GOLDEN["plugin"], ids=lambda c: f"{c['message']}-{c['window']}-{c['word']}")
def test_plugin_closed_forms_on_the_reference(case):
    w = case["window"]
    codes = R.golden_message(case, w + 70)
    h = R.plugin_entropy(codes, w, case["word"], case["alphabet"])
    assert np.isnan(h[:w - 1]).all()
    if case["message"] == "constant":
        assert case["value"] == 0.0 and (h[w - 1:] == 0.0).all()
    else:
        assert case["value"] == math.log2(case["modulus"]) and w % case["modulus"] == 0
        assert np.abs(h[w - 1:] - case["value"]).max() < 1e-13


# ---------------------------------------------------------------------------------------------- the edge helpers
def test_binary_and_quantile_edges():
    assert np.array_equal(P.binary_edges(), [0.0]) and P.binary_edges().dtype == np.float64
    x = np.random.default_rng(5).normal(size=1001)
    x[[3, 500]] = [NAN, INF]
    e = P.quantile_edges(x, 10)
    fin = x[np.isfinite(x)]
    assert e.shape == (9,) and (np.diff(e) > 0).all()
    assert np.array_equal(e, np.unique(np.quantile(fin, np.arange(1, 10) / 10)))
    counts = np.bincount(np.searchsorted(e, fin, side="right"), minlength=10)
    assert counts.min() >= 99 and counts.max() <= 101                         # codes of equal frequency
    assert np.array_equal(P.quantile_edges([1.0, 1.0, 1.0, 2.0], 4), [1.0, 1.25])      # made unique
    assert P.quantile_edges(x, 255).shape == (254,)
    for q in (1, 0, 256):
        with pytest.raises(ValueError) as err:
            P.quantile_edges(x, q)
        assert str(err.value) == P.QUANTILE_MESSAGE
    with pytest.raises(ValueError) as err:
        P.quantile_edges([NAN, INF], 4)
    assert str(err.value) == "quantile_edges: the series holds no finite value."


def test_sigma_edges():
    e = P.sigma_edges([0.0, NAN, 1.0, -INF, 0.35], 0.25)
    assert np.array_equal(e, [0.25, 0.5, 0.75])                               # min + k sigma below max: 1.0 itself is no edge
    assert np.array_equal(P.sigma_edges([2.0, 2.1], 0.5), [2.5])              # a series narrower than sigma: one edge above it
    assert P.sigma_edges([0.0, 254.5], 1.0).shape == (254,)
    for x, sigma in (([0.0, 255.5], 1.0), ([0.0, 1e9], 1e-3)):
        with pytest.raises(ValueError) as err:
            P.sigma_edges(x, sigma)
        assert str(err.value) == P.SIGMA_MAX_MESSAGE
    for sigma in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError) as err:
            P.sigma_edges([0.0, 1.0], sigma)
        assert str(err.value) == P.SIGMA_MESSAGE
    P.rule_edges(P.sigma_edges(np.random.default_rng(6).normal(size=500), 0.1))


# ---------------------------------------------------------------------------------------------- refusals
BIG = 1 << 31
REFUSED = [
    ("plugin_entropy", dict(window=64, word=1, alphabet=1), P.ALPHABET_MESSAGE),
    ("plugin_entropy", dict(window=64, word=1, alphabet=256), P.ALPHABET_MESSAGE),
    ("plugin_entropy", dict(window=64, word=0, alphabet=0), P.ALPHABET_MESSAGE),            # two checks fail: the earlier message
    ("plugin_entropy", dict(window=64, word=0, alphabet=2), P.WORD_MESSAGE),
    ("plugin_entropy", dict(window=0, word=-3, alphabet=2), P.WORD_MESSAGE),
    ("plugin_entropy", dict(window=64, word=13, alphabet=2), P.WORDS_MESSAGE),
    ("plugin_entropy", dict(window=64, word=2, alphabet=65), P.WORDS_MESSAGE),
    ("plugin_entropy", dict(window=64, word=4, alphabet=16), P.WORDS_MESSAGE),
    ("plugin_entropy", dict(window=5000, word=1000000, alphabet=2), P.WORDS_MESSAGE),
    ("plugin_entropy", dict(window=2, word=3, alphabet=2), P.PLUGIN_WINDOW_MESSAGE),
    ("plugin_entropy", dict(window=4097, word=1, alphabet=2), P.PLUGIN_MAX_WINDOW_MESSAGE),
    ("match_lengths", dict(lookback=0), P.MATCH_LOOKBACK_MESSAGE),
    ("match_lengths", dict(lookback=-1), P.MATCH_LOOKBACK_MESSAGE),
    ("match_lengths", dict(lookback=1025), P.MATCH_LOOKBACK_MESSAGE),
    ("kontoyiannis_entropy", dict(window=64, lookback=0), P.KONTO_LOOKBACK_MESSAGE),
    ("kontoyiannis_entropy", dict(window=64, lookback=1025), P.KONTO_LOOKBACK_MESSAGE),
    ("kontoyiannis_entropy", dict(window=5000, lookback=1025), P.KONTO_LOOKBACK_MESSAGE),
    ("kontoyiannis_entropy", dict(window=31, lookback=16), P.KONTO_WINDOW_MESSAGE),
    ("kontoyiannis_entropy", dict(window=1, lookback=1), P.KONTO_WINDOW_MESSAGE),
    ("kontoyiannis_entropy", dict(window=4097, lookback=16), P.KONTO_MAX_WINDOW_MESSAGE),
]
ACCEPTED = [("plugin_entropy", dict(window=4096, word=12, alphabet=2)), ("plugin_entropy", dict(window=1, word=1, alphabet=255)),
            ("plugin_entropy", dict(window=2, word=2, alphabet=64)), ("match_lengths", dict(lookback=1)),
            ("match_lengths", dict(lookback=1024)), ("kontoyiannis_entropy", dict(window=2, lookback=1)),
            ("kontoyiannis_entropy", dict(window=2048, lookback=1024)), ("kontoyiannis_entropy", dict(window=4096, lookback=1024))]
REFUSED_EDGES = [(np.empty(0), P.EDGES_EMPTY_MESSAGE), (np.arange(255.0), P.EDGES_MAX_MESSAGE),
                 (np.array([0.0, NAN]), P.EDGES_FINITE_MESSAGE), (np.array([-INF, 0.0]), P.EDGES_FINITE_MESSAGE),
                 (np.array([0.0, INF]), P.EDGES_FINITE_MESSAGE), (np.array([0.0, 0.0]), P.EDGES_ORDER_MESSAGE),
                 (np.array([0.0, 1.0, 0.5]), P.EDGES_ORDER_MESSAGE),
                 (np.full(255, NAN), P.EDGES_MAX_MESSAGE), (np.array([1.0, 0.0, NAN]), P.EDGES_FINITE_MESSAGE)]     # the earlier message
ABI_ORDER = {"plugin_entropy": ("window", "word", "alphabet"), "match_lengths": ("lookback",), "kontoyiannis_entropy": ("window", "lookback")}


def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library or a context was asked for")
    monkeypatch.setattr(_ffi, "lib", refuse)
    monkeypatch.setattr(_ffi, "default_context", refuse)


def test_the_messages_are_of_the_projects_form():
    texts = [getattr(P, k) for k in dir(P) if k.endswith("_MESSAGE")]
    assert len(texts) >= 18
    for text in texts:
        assert re.fullmatch(r"(\w+|\{\}): .+\.", text), text
    assert P.SERIES_MESSAGE.format("encode") == "encode: the series must hold fewer than 2^31 elements."
    assert (P.INVALID, P.MAX_EDGES, P.MAX_WORDS, P.MAX_WINDOW, P.MAX_LOOKBACK) == (255, 254, 4096, 4096, 1024)


@pytest.mark.parametrize("function,scalars,message", REFUSED)
def test_what_check_arguments_refuses_without_the_library(function, scalars, message, monkeypatch):
    no_library(monkeypatch)
    with pytest.raises(ValueError) as e:
        P.check_arguments(function, 10, **scalars)
    assert str(e.value) == message
    with pytest.raises(ValueError) as e:                              # the rule before the length, the dtype and the empty answer
        P.check_arguments(function, BIG, **scalars)
    assert str(e.value) == message
    args = [scalars[k] for k in ABI_ORDER[function]]
    f64 = SimpleNamespace(dtype=np.dtype(np.float64), n=10)
    for call in (lambda: getattr(P, function)(np.zeros(10, np.uint8), *args), lambda: getattr(P, function)(np.empty(0, np.uint8), *args),
                 lambda: P.resident(None, function, f64, *args)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message
    # the transforms refuse at construction; PluginEntropy's alphabet is its edges' count plus one, so it is never outside 2..255
    build = None
    if function == "kontoyiannis_entropy":
        build = lambda: T.KontoyiannisEntropy(scalars["window"], scalars["lookback"])          # noqa: E731
    elif function == "plugin_entropy" and 2 <= scalars["alphabet"] <= 255:
        build = lambda: T.PluginEntropy(scalars["window"], scalars["word"], edges=np.arange(1.0, scalars["alphabet"]))   # noqa: E731
    if build:
        with pytest.raises(ValueError) as e:
            build()
        assert str(e.value) == message


@pytest.mark.parametrize("function,scalars", ACCEPTED)
def test_what_check_arguments_accepts(function, scalars, monkeypatch):
    no_library(monkeypatch)
    assert P.check_arguments(function, BIG - 1, **scalars) == tuple(scalars[k] for k in ABI_ORDER[function])
    with pytest.raises(ValueError) as e:
        P.check_arguments(function, BIG, **scalars)
    assert str(e.value) == P.SERIES_MESSAGE.format(function)


@pytest.mark.parametrize("case", range(len(REFUSED_EDGES)))
def test_what_encode_refuses_without_the_library(case, monkeypatch):
    edges, message = REFUSED_EDGES[case]
    no_library(monkeypatch)
    f32 = SimpleNamespace(dtype=np.dtype(np.float32), n=10)
    for call in (lambda: P.rule_edges(edges), lambda: P.encode(np.zeros(10), edges), lambda: P.encode(np.empty(0), edges),
                 lambda: P.resident(None, "encode", f32, edges), lambda: T.PluginEntropy(edges=edges),
                 lambda: T.KontoyiannisEntropy(edges=edges)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message
    assert P.rule_edges([0.5]).dtype == np.float64 and P.rule_edges(np.arange(254)).shape == (254,)


def test_both_c_flavours_refuse_the_same_with_a_null_context():
    last = lambda: _ffi.lib().fmk_last_error(None).decode()          # noqa: E731
    for function, scalars, message in REFUSED:
        args = [scalars[k] for k in ABI_ORDER[function]]
        for fn in P.entries(function):
            assert fn(None, None, 10, *args, None) == _ffi.E_ARG, (fn.__name__, scalars)
            assert last() == message
            assert fn(None, None, 0, *args, None) == _ffi.E_ARG, "the rule before the empty answer"
    for function, scalars in ACCEPTED:
        args = [scalars[k] for k in ABI_ORDER[function]]
        for fn in P.entries(function):
            for n in (BIG, -1):
                assert fn(None, None, n, *args, None) == _ffi.E_ARG
                assert last() == P.SERIES_MESSAGE.format(function)
            assert fn(None, None, 0, *args, None) == _ffi.OK        # n == 0 touches nothing, not even the context
    for edges, message in REFUSED_EDGES:
        for fn in P.entries("encode"):
            assert fn(None, None, 10, _ffi.ptr(edges) if edges.size else None, edges.size, None) == _ffi.E_ARG
            assert last() == message
    one = np.array([0.0])
    for fn in P.entries("encode"):
        assert fn(None, None, 10, None, 3, None) == _ffi.E_ARG and last() == P.EDGES_EMPTY_MESSAGE
        assert fn(None, None, BIG, _ffi.ptr(one), 1, None) == _ffi.E_ARG and last() == P.SERIES_MESSAGE.format("encode")
        assert fn(None, None, 0, _ffi.ptr(one), 1, None) == _ffi.OK


def test_the_header_declares_the_entries_outside_the_series_sections():
    text = open(os.path.join(ROOT, "include", "fmk.h")).read()
    at = text.index("/* ---- entropy of an encoded series")
    assert at > text.index("int fmk_sadf(") > text.index("/* ---- labels and sample weights")
    for function in P.ENTRIES:
        for name in ("fmk_" + function, "fmk_" + function + "_dev"):
            assert text.index("int " + name + "(") > at and hasattr(_ffi.lib(), name), name
    assert "fmk_lz.hip" in open(os.path.join(ROOT, "finmlkit_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------------------------------------- no device needed
def test_an_empty_message_needs_no_context(monkeypatch):
    def no_context():
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_ffi, "default_context", no_context)
    empty = np.empty(0, np.uint8)
    for out, dtype in ((P.encode(np.empty(0), [0.0]), np.uint8), (P.encode([], P.binary_edges()), np.uint8),
                       (P.plugin_entropy(empty, 64, 2, 2), np.float64), (P.plugin_entropy([], 64), np.float64),
                       (P.match_lengths(empty, 16), np.uint16), (P.kontoyiannis_entropy(empty, 64, 16), np.float64)):
        assert out.shape == (0,) and out.dtype == dtype
    u8, f64 = SimpleNamespace(dtype=np.dtype(np.uint8), n=0), SimpleNamespace(dtype=np.dtype(np.float64), n=0)
    for function, y, args, dtype in (("encode", f64, ([0.0],), np.uint8), ("plugin_entropy", u8, (64, 2, 2), np.float64),
                                     ("match_lengths", u8, (16,), np.uint16), ("kontoyiannis_entropy", u8, (64, 16), np.float64)):
        out = P.resident(None, function, y, *args)
        assert out.n == 0 and out.dtype == dtype and out.ptr == 0
    with pytest.raises(TypeError) as e:
        P.resident(None, "encode", SimpleNamespace(dtype=np.dtype(np.float32), n=10), [0.0])
    assert str(e.value) == "fmk_encode_dev: the series must be float64, not float32"
    with pytest.raises(TypeError) as e:
        P.resident(None, "kontoyiannis_entropy", SimpleNamespace(dtype=np.dtype(np.float64), n=10), 64, 16)
    assert str(e.value) == "fmk_kontoyiannis_entropy_dev: the series must be uint8, not float64"
    for bad in (np.array([0.5, 1.0]), np.array([0, 256]), np.array([-1, 0])):
        with pytest.raises(ValueError):
            P.match_lengths(bad, 1)


def test_the_exports():
    for name in ("encode", "plugin_entropy", "match_lengths", "kontoyiannis_entropy", "binary_edges", "quantile_edges", "sigma_edges"):
        assert getattr(core, name) is getattr(P, name) and name in core.__all__, name
    assert callable(P.check_arguments) and callable(P.resident)
    from finmlkit_amd.engine import DeviceTrades
    for name in ("encode", "plugin_entropy", "match_lengths", "kontoyiannis_entropy"):
        assert callable(getattr(DeviceTrades, name)), name


def test_the_transforms_are_built_without_a_device(monkeypatch):
    no_library(monkeypatch)
    t = T.PluginEntropy()
    assert (t.requires, t.produces, t.output_name) == (["ret1"], ["plugin64_w2"], "ret1_plugin64_w2")
    assert (t.window, t.word, t.alphabet) == (64, 2, 2) and np.array_equal(t.edges, [0.0])
    t = T.PluginEntropy(128, 3, edges=(-1.0, 0.0, 1.0), input_col="x")
    assert (t.requires, t.produces, t.output_name) == (["x"], ["plugin128_w3"], "x_plugin128_w3") and t.alphabet == 4
    t = T.PluginEntropy(100, 1, edges=10)
    assert t.edges == 10 and t.alphabet == 10
    t = T.KontoyiannisEntropy()
    assert (t.requires, t.produces, t.output_name) == (["ret1"], ["konto64_16"], "ret1_konto64_16")
    assert (t.window, t.lookback) == (64, 16) and np.array_equal(t.edges, [0.0])
    t = T.KontoyiannisEntropy(200, 50, edges=8, input_col="r")
    assert (t.requires, t.produces, t.output_name, t.edges) == (["r"], ["konto200_50"], "r_konto200_50", 8)
    for cls in (T.PluginEntropy, T.KontoyiannisEntropy):
        assert issubclass(cls, T.SISOTransform) and cls._dev is not T.SISOTransform._dev            # Compose keeps it on the device
        for q in (1, 256):
            with pytest.raises(ValueError) as e:
                cls(edges=q)
            assert str(e.value) == P.QUANTILE_MESSAGE
        with pytest.raises(ValueError) as e:                         # the device form has no column to take quantiles of
            cls(edges=4)._dev(None, None)
        assert "quantile_edges" in str(e.value) and str(e.value).startswith(cls.__name__ + ": ")
    import pandas as pd
    c = T.Compose(T.ReturnT(pd.Timedelta(seconds=1e-6), input_col="price"), T.KontoyiannisEntropy(64, 16))
    assert c.output_name == "price_ret1_konto64_16"


# ---------------------------------------------------------------------------------------------- the messages of the edge tests
@pytest.mark.parametrize("lookback", (64, 129, 256, 1023, 1024))
def test_planted_repeats_have_their_closed_form_on_the_reference(lookback):
    """tests/test_gpu_lz_edges.py compares the kernel with R.match_lengths on these messages; here the reference itself against what
    was planted: a run of exactly r matches at lag d from p on gives 1 + min(r, n) at p, and at least 1 + min(r - i, n) i codes on."""
    n = lookback
    codes, plants = R.planted_message(n, R.plant_seed(n))
    assert codes.dtype == np.uint8 and codes.max() <= 250 and len(plants) == len({(d, r) for _, d, r in plants}) >= 45
    lam = R.match_lengths(codes, n)
    for p, d, r in plants:
        assert codes[p - 1] != codes[p - 1 - d] and codes[p + r] != codes[p + r - d] and (codes[p:p + r] == codes[p - d:p + r - d]).all()
        assert lam[p] == 1 + min(r, n), (p, d, r)
        assert (lam[p:p + r] >= 1 + np.minimum(r - np.arange(r), n)).all(), (p, d, r)
    starts = [p for p, _, _ in plants]
    assert {0, 1, 63} <= {p % 64 for p in starts} and {0, 1, 255} <= {p % 256 for p in starts}
    assert starts[0] > 2 * n + 256 and len(codes) == starts[-1] + plants[-1][2] + n + 300
    assert min(b - 1 - (a + r + 1) for (a, _, r), b in zip(plants, starts[1:])) >= 2 * n + 8     # background between two plants
    # what the random messages do not hold: a run of more than 64 that stops before the cap, at a lag beyond 65
    assert lookback < 129 or sum(1 for _, d, r in plants if d > 65 and 64 < r < n) >= 6
    if lookback == 64:
        msg = tuple(int(c) for c in codes)
        for p in starts:
            assert R.match_length(msg, p, n) == lam[p], p


@pytest.mark.parametrize("lookback", (127, 128, 129, 255, 256, 257, 1023, 1024))
def test_the_messages_at_large_lookbacks_cover_what_they_are_for(lookback):
    n, N = lookback, R.edge_length(lookback)
    first, end = R.edge_stretch(n)
    assert end - first == 2 * n + 300 and first // 256 != (end - 1) // 256 and end < N
    sp = R.match_lengths(R.edge_message("spliced", n), n)
    assert (sp[first + 1:end - n + 1] == n + 1).all()                                           # the cap, on a stretch
    assert len(set(sp[end - n:end + 64])) >= 64                                                  # and the tail behind it: every length
    at = R.edge_invalid_at(n)
    assert at[0] == 3 and at[1] % 256 == 0 and at[1] > 2 * n and at[2] % 256 == 255 and at[2] // 256 != at[1] // 256 and at[3] == N - 1
    codes = R.edge_message("invalid", n)
    assert np.array_equal(np.flatnonzero(codes == 255), at)
    zero = np.zeros(N, bool)
    zero[:n], zero[N - n + 1:] = True, True
    for i in at:
        zero[max(0, i - n + 1):i + n + 1] = True
    bad = R.match_lengths(codes, n)
    assert np.array_equal(bad == 0, zero) and np.count_nonzero(bad) >= 256
    assert (R.match_lengths(R.edge_message("constant", n), n)[n:N - n + 1] == n + 1).all()
    ramp = R.match_lengths(R.edge_message("k mod 255", n), n)[n:N - n + 1]                    # a period within the lookback: the cap
    assert (ramp == (n + 1 if n >= 255 else 1)).all()
    assert not R.match_lengths(np.full(2400, 255, np.uint8), 1024).any()


def test_the_kontoyiannis_nan_message_on_the_reference():
    window, lookback, at = R.KONTO_NAN
    codes = R.message("invalid", 4 * window, None, at)
    assert at[0] == 3 and at[-1] == len(codes) - 1 and window < at[1] < len(codes) - 2 * window
    want = R.kontoyiannis_entropy(codes, window, lookback)
    nan = np.zeros(len(codes), bool)
    nan[:window - 1] = True
    for i in at:
        nan[i:i + window] = True
    assert np.array_equal(np.isnan(want), nan)
    assert 2 * int(np.isfinite(want[window - 1:]).sum()) >= len(codes) - window + 1               # finite in half of the full windows


# ---------------------------------------------------------------------------------------------- the header on the host
def test_rule_header_on_the_host(tmp_path):
    """tools/lz_check.cpp, built from csrc/fmk_lz_rule.h with the host compiler alone (no HIP), in its quick form: the runs a wave
    reads from its mask words, the match lengths of whole messages, the word ids and the codes against the literal definitions.  (The
    full run under ASan / UBSan is a tool run, not part of the suite.)"""
    exe = str(tmp_path / "lz_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "lz_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "quick"], capture_output=True, text=True)
    assert r.returncode == 0 and "failed checks 0" in r.stdout, r.stdout
    assert all(int(x) > 1000 for x in re.search(r"runs (\d+) positions (\d+) words (\d+)", r.stdout).groups())
