"""The sequential bootstrap of DESIGN.md §7n in Python integers and NumPy uint64, written from the definition alone (not from
csrc/fmk_seqboot_rule.h), in both forms: `brute` keeps one concurrency count per position of the axis, `compressed` one per
interval between span boundaries.  Every quantity is an integer below 2^63, so both are exact.  Also the plain bootstrap from the
same word generator and the book's mean average uniqueness of a sample, which the property test and bootstrap_uniqueness lean on."""
import numpy as np

ONE = 1 << 30
M64 = (1 << 64) - 1


def word(seed, index):
    """the random word of draw `index` = run * n_draws + draw"""
    z = (seed + (index + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def words_of(seed, n_runs, n_draws):
    return np.array([word(seed, i) for i in range(n_runs * n_draws)], np.uint64)


def _word(seed, words, index):
    return int(words[index]) if words is not None else word(seed, index)


def _pick(Q, w):
    """the smallest i with Q_0 + .. + Q_i > target for the word w; Q: a list of Python ints"""
    total = sum(Q)
    assert 0 < total < 1 << 62
    target = (w * total) >> 64
    acc = 0
    for i, q in enumerate(Q):
        acc += q
        if acc > target:
            return i
    raise AssertionError("target outside the total")


def brute(ev, tc, n, n_draws, n_runs=1, seed=0, words=None):
    """Per position: c[t] for every t of the axis -> (draws, Q) as int64 arrays of shape (n_runs, n_draws)."""
    ev, tc = [int(x) for x in ev], [int(x) for x in tc]
    assert all(0 <= e <= t < n for e, t in zip(ev, tc))
    draws, qs = np.zeros((n_runs, n_draws), np.int64), np.zeros((n_runs, n_draws), np.int64)
    for r in range(n_runs):
        c = [0] * n
        for k in range(n_draws):
            Q = [sum(ONE // (c[t] + 1) for t in range(e, t1 + 1)) // (t1 - e + 1) for e, t1 in zip(ev, tc)]
            i = _pick(Q, _word(seed, words, r * n_draws + k))
            draws[r, k], qs[r, k] = i, Q[i]
            for t in range(ev[i], tc[i] + 1):
                c[t] += 1
    return draws, qs


def compress(ev, tc):
    """-> (interval lengths, lo, hi): event i covers the intervals [lo_i, hi_i) between the sorted unique boundaries"""
    ev, tc = np.asarray(ev, np.int64), np.asarray(tc, np.int64)
    b = np.unique(np.concatenate([ev, tc + 1]))
    return np.diff(b).astype(np.uint64), np.searchsorted(b, ev), np.searchsorted(b, tc + 1)


def compressed(ev, tc, n, n_draws, n_runs=1, seed=0, words=None):
    """One count per interval; NumPy uint64 (every value stays below 2^63) -> (draws, Q) int64 of shape (n_runs, n_draws)."""
    ev, tc = np.asarray(ev, np.int64), np.asarray(tc, np.int64)
    assert len(ev) and np.all((0 <= ev) & (ev <= tc) & (tc < n)) and n <= 1 << 32
    lens, lo, hi = compress(ev, tc)
    L = (tc - ev + 1).astype(np.uint64)
    assert np.array_equal(np.concatenate([[0], np.cumsum(lens)])[hi] - np.concatenate([[0], np.cumsum(lens)])[lo], L)
    draws, qs = np.zeros((n_runs, n_draws), np.int64), np.zeros((n_runs, n_draws), np.int64)
    for r in range(n_runs):
        c = np.zeros(len(lens), np.uint64)
        for k in range(n_draws):
            P = np.concatenate([[np.uint64(0)], np.cumsum(lens * (np.uint64(ONE) // (c + np.uint64(1))), dtype=np.uint64)])
            Q = (P[hi] - P[lo]) // L
            cum = np.cumsum(Q, dtype=np.uint64)
            total = int(cum[-1])
            assert 0 < total <= len(ev) << 30 and int(Q.min()) > 0
            target = (_word(seed, words, r * n_draws + k) * total) >> 64
            i = int(np.searchsorted(cum, np.uint64(target), side="right"))
            draws[r, k], qs[r, k] = i, int(Q[i])
            c[lo[i]:hi[i]] += np.uint64(1)
    return draws, qs


def plain(m, n_draws, n_runs=1, seed=0):
    """The plain bootstrap from the same words: draw k of run r is the high 64 bits of word * m."""
    return np.array([[(word(seed, r * n_draws + k) * m) >> 64 for k in range(n_draws)] for r in range(n_runs)], np.int64)


def mean_uniqueness(ev, tc, n, sample):
    """The book's mean average uniqueness of a sample (event positions, with their multiplicities): the mean over the sample's
    members of the mean of 1 / concurrency over the member's span, the concurrency counted over the sample."""
    ev, tc = np.asarray(ev, np.int64)[np.asarray(sample)], np.asarray(tc, np.int64)[np.asarray(sample)]
    d = np.zeros(n + 1, np.int64)
    np.add.at(d, ev, 1)
    np.add.at(d, tc + 1, -1)
    inv = np.concatenate([[0.0], np.cumsum(1.0 / np.maximum(np.cumsum(d)[:n], 1), dtype=np.longdouble)])
    return float(np.mean((inv[tc + 1] - inv[ev]) / (tc - ev + 1)))


def uniqueness_given(ev, tc, n, drawn):
    """Q of every candidate after the events `drawn` (positions, in any order) have been drawn -> a list of Python ints"""
    c = [0] * n
    for i in drawn:
        for t in range(int(ev[i]), int(tc[i]) + 1):
            c[t] += 1
    return [sum(ONE // (c[t] + 1) for t in range(int(e), int(t1) + 1)) // (int(t1) - int(e) + 1) for e, t1 in zip(ev, tc)]
