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
