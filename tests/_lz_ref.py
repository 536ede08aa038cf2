"""References of the encoded-series entropies (finmlkit_amd/feature/core/lz.py), no device and no library.

First the snippets 18.1, 18.3 and 18.4 of Advances in Financial Machine Learning restated literally on tuples of codes -- the book
joins the codes into a string with ''.join(map(str, msg)), which takes the codes 1, 0 and the code 10 for the same message -- and the
rolling estimators as the book would run them: the snippet on the tuple of every window.  Two departures, both this project's
definition: the plug-in counts all window - word + 1 words of a window (the loop of snippet 18.1 stops one word short), and a window
that holds an invalid code gives NaN.

Then the same values from NumPy, vectorised per lag, through the match length of a POSITION: 1 + the longest match of
codes[p ..] with a string that starts 1 .. n codes earlier, capped at n, does not depend on the window it is read through."""
import numpy as np

INVALID = 255


def golden_message(case, n):
    """the message of n codes that a case of tests/golden/lz.json names"""
    k = np.arange(n)
    if case["message"] == "constant":
        return np.full(n, case["code"], np.uint8)
    if case["message"] == "period":
        return (k % case["period"]).astype(np.uint8)
    assert case["message"] == "ramp"
    return (k % case["modulus"]).astype(np.uint8)


# ------------------------------------------------------------------------------------------ the book, on tuples
def pmf1(msg, w):
    """snippet 18.1: the frequencies of the words of w codes (every word of the message)"""
    lib = {}
    for i in range(w, len(msg) + 1):
        lib.setdefault(tuple(msg[i - w:i]), []).append(i - w)
    total = float(len(msg) - w + 1)
    return {word: len(at) / total for word, at in lib.items()}


def plug_in(msg, w):
    """snippet 18.1: the plug-in entropy rate"""
    pmf = pmf1(msg, w)
    return -sum(pmf[i] * np.log2(pmf[i]) for i in pmf) / w


def match_length(msg, i, n):
    """snippet 18.3: the matched length + 1, with overlap; i >= n and len(msg) >= i + n"""
    sub = ()
    for length in range(n):
        msg1 = tuple(msg[i:i + length + 1])
        for j in range(i - n, i):
            if msg1 == tuple(msg[j:j + length + 1]):
                sub = msg1
                break
    return len(sub) + 1


def konto(msg, window):
    """snippet 18.4 with a window: the mean of log2(window + 1) / match length over the points window .. len - window"""
    window = min(window, len(msg) // 2)
    total, num = 0.0, 0
    for i in range(window, len(msg) - window + 1):
        total += np.log2(window + 1) / match_length(msg, i, window)
        num += 1
    return total / num


def rolling_literal(codes, window, fn, alphabet=INVALID):
    """fn on the tuple of every full window; NaN before the first and where the window holds a code >= alphabet"""
    codes = [int(c) for c in codes]
    out = np.full(len(codes), np.nan)
    for t in range(window - 1, len(codes)):
        msg = tuple(codes[t - window + 1:t + 1])
        if max(msg) < alphabet:
            out[t] = fn(msg)
    return out


def plugin_literal(codes, window, word, alphabet):
    return rolling_literal(codes, window, lambda msg: plug_in(msg, word), alphabet)


def konto_literal(codes, window, lookback):
    return rolling_literal(codes, window, lambda msg: konto(msg, lookback))


# ------------------------------------------------------------------------------------------ NumPy, per lag
def match_lengths(codes, n):
    """uint16: 1 + max over d = 1 .. n of min(n, matches codes[k] == codes[k-d] in a row from p on) for n <= p <= N - n whose
    codes[p-n .. p+n) hold no 255; 0 elsewhere"""
    codes = np.asarray(codes, dtype=np.uint8)
    N = len(codes)
    out = np.zeros(N, np.uint16)
    if N < 2 * n:
        return out
    idx = np.arange(N + 1)
    best = np.zeros(N, np.int64)
    for d in range(1, n + 1):
        eq = np.zeros(N + 1, bool)                                   # eq[N] = False: every run ends
        eq[d:N] = codes[d:] == codes[:-d]
        stop = np.minimum.accumulate(np.where(eq, N, idx)[::-1])[::-1]      # the first k' >= k without a match
        np.maximum(best, np.minimum(stop[:N] - idx[:N], n), out=best)
    bad = np.concatenate(([0], np.cumsum(codes == INVALID)))
    p = np.arange(n, N - n + 1)
    ok = bad[p + n] == bad[p - n]
    out[p[ok]] = 1 + best[p[ok]]
    return out


def kontoyiannis_entropy(codes, window, lookback):
    """log2(n + 1) times the mean of 1 / L over p = t-window+1+n .. t-n+1; NaN before t = window - 1 and where one L is 0"""
    lam = match_lengths(codes, lookback).astype(np.float64)
    out = np.full(len(lam), np.nan)
    count = window - 2 * lookback + 1
    if len(lam) < window:
        return out
    with np.errstate(divide="ignore"):
        rcp = np.where(lam > 0, 1.0 / lam, np.nan)
    # output t reads rcp[t-window+1+n .. t-n+1]: the windows of `count` that start at n .. N - window + n
    sums = np.lib.stride_tricks.sliding_window_view(rcp[lookback:len(lam) - lookback + 1], count).sum(axis=1)
    out[window - 1:] = np.log2(lookback + 1) * sums / count
    return out


def plugin_entropy(codes, window, word=1, alphabet=2):
    """-sum p log2 p / word over the window - word + 1 words of every window; NaN where the window holds a code >= alphabet"""
    codes = np.asarray(codes, dtype=np.int64)
    N, M = len(codes), window - word + 1
    out = np.full(N, np.nan)
    if N < window:
        return out
    ids = np.zeros(N - word + 1, np.int64)
    for j in range(word):
        ids = ids * alphabet + codes[j:N - word + 1 + j]
    bad = np.concatenate(([0], np.cumsum(codes >= alphabet)))
    for t in range(window - 1, N):
        lo = t - window + 1
        if bad[t + 1] != bad[lo]:
            continue
        c = np.unique(ids[lo:lo + M], return_counts=True)[1]
        p = c / M
        out[t] = -(p * np.log2(p)).sum() / word + 0.0                # (+ 0.0: no -0.0 for a constant window)
    return out


# ------------------------------------------------------------------------------------------ the messages of the tests
TILE = 256                           # positions per workgroup of the match lengths (csrc/fmk_lz.hip)


def message(name, n_codes, stretch=None, invalid_at=None):
    """The seeded message `name` of n_codes codes (read-only).  `stretch` = (first, end) is the constant stretch of "spliced",
    `invalid_at` the positions of the 255s of "invalid"; the defaults are those of the 1100-code messages of tests/test_gpu_lz.py."""
    rng = np.random.default_rng(1800 + sum(map(ord, name)))
    k = np.arange(n_codes)
    if name == "binary":
        m = rng.integers(0, 2, n_codes)
    elif name == "4-ary":
        m = rng.integers(0, 4, n_codes)
    elif name == "16-ary":
        m = rng.integers(0, 16, n_codes)
    elif name == "constant":
        m = np.ones(n_codes)
    elif name == "period 2":
        m = k % 2
    elif name == "period 65":
        m = k % 65
    elif name == "k mod 255":
        m = k % 255
    elif name == "spliced":                                          # a constant stretch in a binary message
        first, end = stretch or (TILE - 150, TILE + 150)
        m = rng.integers(0, 2, n_codes)
        m[first:end] = 1
    elif name == "invalid":                                          # a few invalid codes in a 3-ary message
        m = rng.integers(0, 3, n_codes)
        m[list(invalid_at or (3, 4 * TILE, n_codes - 1))] = INVALID
    else:
        assert name == "over"                                        # codes beyond a binary alphabet that are not 255
        m = rng.integers(0, 2, n_codes)
        m[[300, 301]] = [2, 200]
    m = m.astype(np.uint8)
    m.setflags(write=False)
    return m


def edge_length(lookback):
    """the length of the messages at the large lookbacks: four lookbacks, three tiles and an odd rest"""
    return 4 * lookback + 3 * TILE + 77


def edge_stretch(lookback):
    """the constant stretch of the spliced message at a large lookback: 2 n + 300 codes (more than a tile: it crosses a tile's edge),
    from a little behind the first valid position"""
    return lookback + 50, 3 * lookback + 350


def edge_invalid_at(lookback):
    """the 255s of the invalid message at a large lookback: position 3, the first element of the first tile that starts beyond
    2 n, the last element of the tile after that one, and the last code"""
    tile = TILE * (2 * lookback // TILE + 1)
    return 3, tile, tile + 2 * TILE - 1, edge_length(lookback) - 1


def edge_message(name, lookback):
    return message(name, edge_length(lookback), edge_stretch(lookback), edge_invalid_at(lookback))


KONTO_NAN = (4096, 64, (3, 8000, 4 * 4096 - 1))       # (window, lookback, the 255s) of the 16384-code message of the NaN windows


PLANT_LAGS = (1, 2, 63, 64, 65)
PLANT_RUNS = (1, 2, 63, 64, 65, 127, 128, 129)


def planted_message(lookback, seed):
    """(codes, plants): random codes 0 .. 250 with one planted repeat per (lag d, run r), plants = [(p, d, r)].  A plant copies
    codes[i] = codes[i - d] for i = p .. p + r - 1, ascending (r > d: the match runs over p itself), and codes[p - 1] and codes[p + r]
    are made to differ from the codes d before them: the run at lag d starts at p and holds exactly r matches.  The starts cycle
    through the lanes 0, 1 and 63 of a wave; every fifth plant sits on the first, the second or the last element of a 256-position
    tile.  2 n + 8 background codes or more lie between two plants, the first starts beyond 2 n + 256, n + 300 codes follow the last."""
    n = lookback
    rng = np.random.default_rng(seed)
    lags = sorted({d for d in PLANT_LAGS + (n // 2, n - 1, n) if 1 <= d <= n})
    runs = sorted({r for r in PLANT_RUNS + (n - 1, n, n + 7) if r >= 1})
    plants, at = [], 2 * n + TILE + 1
    for k, (d, r) in enumerate((d, r) for d in lags for r in runs):
        if k % 5 == 4:
            p = at + (((0, 1, TILE - 1)[k // 5 % 3] - at) % TILE)
        else:
            p = at + (((0, 1, 63)[k % 3] - at) % 64)
        plants.append((p, d, r))
        at = p + r + 1 + 2 * n + 8 + 1                               # the stop code, the background, the code in front of the next plant
    codes = rng.integers(0, 251, plants[-1][0] + plants[-1][2] + n + 300)

    def differ(i, d):                                                # codes[i] != codes[i - d], whatever it was
        if codes[i] == codes[i - d]:
            codes[i] = (codes[i - d] + 1 + rng.integers(0, 250)) % 251

    for p, d, r in plants:
        differ(p - 1, d)
        for i in range(p, p + r):
            codes[i] = codes[i - d]
        differ(p + r, d)
    codes = codes.astype(np.uint8)
    codes.setflags(write=False)
    return codes, plants


def plant_seed(lookback):
    return 1900 + lookback
