"""Entropy of an encoded series (Lopez de Prado, Advances in Financial Machine Learning, ch. 18) on the MI355X (csrc/fmk_lz.hip): the
encoding of a float64 series into a message of uint8 codes, the rolling plug-in entropy of the message's words (snippet 18.1) and
Kontoyiannis' sliding-window Lempel-Ziv estimator (snippets 18.3 and 18.4).  The reference has none of them; the definitions are this
project's (include/fmk.h):

    code[i]  = np.searchsorted(edges, x[i], side="right"), 255 for a NaN; a code >= alphabet is invalid, 255 always
    plug-in  H[t] = (log2 M - (1/M) sum_c N_c log2 c) / word over the M = window - word + 1 words of codes[t-window+1 .. t]
    L[p]     = 1 + max over d = 1 .. n of min(n, matches codes[k] == codes[k-d] in a row from k = p on), 0 without a full valid span
    LZ       H[t] = log2(n + 1) / (window - 2n + 1) * sum of 1 / L[p], p = t-window+1+n .. t-n+1

in bits per symbol; NaN before the first full window and in every window that reads an invalid code.  The match length belongs to
the position and not to the window it is read through: one pass over the message, then a rolling mean.  The edge helpers are plain
NumPy on the host.  Left to the caller: the redundancy 1 - H / log2(window) and the expanding-window form of snippet 18.4."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
from numpy.typing import NDArray

from ... import _ffi
from ..._ffi import DeviceArray, c_i64, c_vp, ptr

INVALID = 255                        # csrc/fmk_lz_rule.h: FMK_LZ_INVALID
MAX_EDGES = 254
MAX_WORDS = 4096
MAX_WINDOW = 4096
MAX_LOOKBACK = 1024
EDGES_EMPTY_MESSAGE = "encode: at least one edge is needed."
EDGES_MAX_MESSAGE = "encode: at most 254 edges."
EDGES_FINITE_MESSAGE = "encode: the edges must be finite."
EDGES_ORDER_MESSAGE = "encode: the edges must be strictly increasing."
ALPHABET_MESSAGE = "plugin_entropy: alphabet must be between 2 and 255."
WORD_MESSAGE = "plugin_entropy: word must be at least 1."
WORDS_MESSAGE = "plugin_entropy: alphabet^word must be at most 4096."
PLUGIN_WINDOW_MESSAGE = "plugin_entropy: window must be at least word."
PLUGIN_MAX_WINDOW_MESSAGE = "plugin_entropy: window must be at most 4096."
MATCH_LOOKBACK_MESSAGE = "match_lengths: lookback must be between 1 and 1024."
KONTO_LOOKBACK_MESSAGE = "kontoyiannis_entropy: lookback must be between 1 and 1024."
KONTO_WINDOW_MESSAGE = "kontoyiannis_entropy: window must be at least 2 * lookback."
KONTO_MAX_WINDOW_MESSAGE = "kontoyiannis_entropy: window must be at most 4096."
SERIES_MESSAGE = "{}: the series must hold fewer than 2^31 elements."
SIGMA_MESSAGE = "sigma_edges: sigma must be finite and greater than 0."
SIGMA_MAX_MESSAGE = "sigma_edges: more than 254 edges; raise sigma."
QUANTILE_MESSAGE = "quantile_edges: q must be between 2 and 255."
NO_FINITE_MESSAGE = "{}: the series holds no finite value."
Q_DEV_MESSAGE = "{}: the device form takes explicit edges; compute them with quantile_edges on the host."


# ---------------------------------------------------------------------------------------------- edges (host, plain NumPy)
def binary_edges() -> NDArray[np.float64]:
    """[0.0]: code 0 below zero, code 1 at and above it."""
    return np.array([0.0])


def quantile_edges(x, q: int) -> NDArray[np.float64]:
    """The in-sample k / q quantiles of the finite values of `x`, k = 1 .. q - 1, made unique (AFML section 18.5.2): codes of about
    equal frequency.  Ties can leave fewer than q - 1 edges."""
    q = int(q)
    if not 2 <= q <= MAX_EDGES + 1:
        raise ValueError(QUANTILE_MESSAGE)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    x = x[np.isfinite(x)]
    if not x.size:
        raise ValueError(NO_FINITE_MESSAGE.format("quantile_edges"))
    return np.unique(np.quantile(x, np.arange(1, q) / q))


def sigma_edges(x, sigma: float) -> NDArray[np.float64]:
    """min + k * sigma, k = 1, 2, .. below max, over the finite values of `x` (AFML section 18.5.3): codes of equal width.  A series
    narrower than sigma gets the single edge min + sigma; more than 254 edges is a ValueError."""
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma > 0.0):
        raise ValueError(SIGMA_MESSAGE)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    x = x[np.isfinite(x)]
    if not x.size:
        raise ValueError(NO_FINITE_MESSAGE.format("sigma_edges"))
    lo, hi = float(x.min()), float(x.max())
    if (hi - lo) / sigma > MAX_EDGES + 1:
        raise ValueError(SIGMA_MAX_MESSAGE)
    edges = lo + sigma * np.arange(1, MAX_EDGES + 2)
    edges = edges[edges < hi]
    if edges.size > MAX_EDGES:
        raise ValueError(SIGMA_MAX_MESSAGE)
    return edges if edges.size else np.array([lo + sigma])


# ---------------------------------------------------------------------------------------------- rules (no library, no device)
def rule_edges(edges) -> NDArray[np.float64]:
    """What encode refuses about its edges, in the library's order (csrc/fmk_common.h: fmk_rule_encode) -> the edges as the library
    takes them."""
    e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if e.size < 1:
        raise ValueError(EDGES_EMPTY_MESSAGE)
    if e.size > MAX_EDGES:
        raise ValueError(EDGES_MAX_MESSAGE)
    if not np.isfinite(e).all():
        raise ValueError(EDGES_FINITE_MESSAGE)
    if not (e[:-1] < e[1:]).all():
        raise ValueError(EDGES_ORDER_MESSAGE)
    return e


def check_arguments(function: str, n: int = 0, *, window=None, word=None, alphabet=None, lookback=None):
    """What `function` ("plugin_entropy", "match_lengths", "kontoyiannis_entropy", "encode") refuses about its scalars and the
    length n of its series, in the library's order, with the library's messages -> the scalars as ints, in ABI order.  Needs no
    library."""
    if function == "plugin_entropy":
        window, word, alphabet = int(window), int(word), int(alphabet)
        if not 2 <= alphabet <= 255:
            raise ValueError(ALPHABET_MESSAGE)
        if word < 1:
            raise ValueError(WORD_MESSAGE)
        if word > 12 or alphabet ** word > MAX_WORDS:
            raise ValueError(WORDS_MESSAGE)
        if window < word:
            raise ValueError(PLUGIN_WINDOW_MESSAGE)
        if window > MAX_WINDOW:
            raise ValueError(PLUGIN_MAX_WINDOW_MESSAGE)
        out = (window, word, alphabet)
    elif function == "match_lengths":
        lookback = int(lookback)
        if not 1 <= lookback <= MAX_LOOKBACK:
            raise ValueError(MATCH_LOOKBACK_MESSAGE)
        out = (lookback,)
    elif function == "kontoyiannis_entropy":
        window, lookback = int(window), int(lookback)
        if not 1 <= lookback <= MAX_LOOKBACK:
            raise ValueError(KONTO_LOOKBACK_MESSAGE)
        if window < 2 * lookback:
            raise ValueError(KONTO_WINDOW_MESSAGE)
        if window > MAX_WINDOW:
            raise ValueError(KONTO_MAX_WINDOW_MESSAGE)
        out = (window, lookback)
    elif function == "encode":
        out = ()
    else:
        raise KeyError(function)
    if not 0 <= int(n) < 2 ** 31:
        raise ValueError(SERIES_MESSAGE.format(function))
    return out


# ---------------------------------------------------------------------------------------------- the library's entries
# per function: (the element types in and out, the prototype behind context, series, n)
_u8, _u16, _f64 = np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float64)
ENTRIES = {"encode": (_f64, _u8, [c_vp, c_i64]),                             # edges (host), n_edges
           "plugin_entropy": (_u8, _f64, [c_i64, c_i64, c_i64]),             # window, word, alphabet
           "match_lengths": (_u8, _u16, [c_i64]),                            # lookback
           "kontoyiannis_entropy": (_u8, _f64, [c_i64, c_i64])}              # window, lookback


@functools.lru_cache(maxsize=None)
def entries(function: str):
    """(fmk_<function>, fmk_<function>_dev) of the loaded library with restype and argtypes set."""
    fns = tuple(getattr(_ffi.lib(), name) for name in ("fmk_" + function, "fmk_" + function + "_dev"))
    for fn in fns:
        fn.restype, fn.argtypes = C.c_int, [c_vp, c_vp, c_i64] + ENTRIES[function][2] + [c_vp]
    return fns


def _host(function: str, series, scalars) -> np.ndarray:
    """The host-pointer driver: `series` is a contiguous array of the entry's input type, the rules are asked already.  An empty
    series is answered without a context."""
    out = np.empty(len(series), ENTRIES[function][1])
    if len(series):
        ctx = _ffi.default_context()
        _ffi.check(entries(function)[0](ctx.handle, ptr(series), len(series), *scalars, ptr(out)), ctx.handle)
    return out


def resident(ctx, function: str, y: DeviceArray, *args) -> DeviceArray:
    """fmk_<function>_dev on a DeviceArray -> DeviceArray.  args: the function's arguments behind the series, as the host function
    takes them (encode: the edges, which stay on the host).  Rules and dtype are checked, in this order, before `ctx` or a pointer is
    looked at; an empty series is answered by an empty array that owns no memory."""
    t_in, t_out, _ = ENTRIES[function]
    if function == "encode":
        e = rule_edges(args[0])
        check_arguments(function, y.n)
        scalars = (ptr(e), e.size)
    elif function == "plugin_entropy":
        scalars = check_arguments(function, y.n, window=args[0], word=args[1], alphabet=args[2])
    elif function == "match_lengths":
        scalars = check_arguments(function, y.n, lookback=args[0])
    else:
        scalars = check_arguments(function, y.n, window=args[0], lookback=args[1])
    if y.dtype != t_in:
        raise TypeError(f"fmk_{function}_dev: the series must be {t_in}, not {y.dtype}")
    if not y.n:
        return DeviceArray(ctx, 0, t_out, dptr=0)
    out = DeviceArray(ctx, y.n, t_out)
    _ffi.check(entries(function)[1](ctx.handle, y.p, y.n, *scalars, out.p), ctx.handle)
    return out


def _codes(codes) -> NDArray[np.uint8]:
    c = np.asarray(codes)
    if c.dtype != np.uint8:
        if c.size and (not np.issubdtype(c.dtype, np.integer) or c.min() < 0 or c.max() > 255):
            raise ValueError("a message is an array of codes 0 .. 255 (uint8).")
        c = c.astype(np.uint8)
    return np.ascontiguousarray(c).reshape(-1)


# ---------------------------------------------------------------------------------------------- the functions
def encode(x, edges) -> NDArray[np.uint8]:
    """The message of a float64 series: code[i] = np.searchsorted(edges, x[i], side="right") with +-inf included, 255 for a NaN.
    `edges`: 1 to 254 finite, strictly increasing values; the alphabet is len(edges) + 1."""
    e = rule_edges(edges)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    check_arguments("encode", len(x))
    return _host("encode", x, (ptr(e), e.size))


def plugin_entropy(codes, window: int, word: int = 1, alphabet: int = 2) -> NDArray[np.float64]:
    """The plug-in (maximum likelihood) entropy rate of codes[t-window+1 .. t] in bits per symbol: -sum p log2 p / word over the
    frequencies p of the window's window - word + 1 overlapping words.  NaN before t = window - 1 and where the window reads a code
    >= alphabet; exactly 0.0 where every word is the same."""
    scalars = check_arguments("plugin_entropy", len(codes), window=window, word=word, alphabet=alphabet)
    return _host("plugin_entropy", _codes(codes), scalars)


def match_lengths(codes, lookback: int) -> NDArray[np.uint16]:
    """L[p] = 1 + the longest match of codes[p ..] with a string that starts at most `lookback` positions earlier, capped at
    lookback (so L lies in 1 .. lookback + 1); a match may run over p itself.  0 for p < lookback, p > len - lookback and wherever
    codes[p-lookback .. p+lookback) holds the code 255."""
    scalars = check_arguments("match_lengths", len(codes), lookback=lookback)
    return _host("match_lengths", _codes(codes), scalars)


def kontoyiannis_entropy(codes, window: int, lookback: int) -> NDArray[np.float64]:
    """Kontoyiannis' sliding-window Lempel-Ziv estimate of the entropy rate of codes[t-window+1 .. t] in bits per symbol (the book's
    snippet 18.4 with a look-back of `lookback` codes): log2(lookback + 1) times the mean of 1 / L over the window's
    window - 2 lookback + 1 inner positions.  NaN before t = window - 1 and where the window reads the code 255."""
    scalars = check_arguments("kontoyiannis_entropy", len(codes), window=window, lookback=lookback)
    return _host("kontoyiannis_entropy", _codes(codes), scalars)
