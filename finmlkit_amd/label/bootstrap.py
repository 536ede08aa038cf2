"""The sequential bootstrap of Advances in Financial Machine Learning, section 4.5, on label spans: after every draw each event's
probability is proportional to its average uniqueness given the draws so far, so that a sample of overlapping labels holds less
redundancy than a plain bootstrap's.  The reference has no such function: the definition is this project's,
in integers, so that a run is a function of its events, its seed and nothing else.  The draws are made on the MI355X
(csrc/fmk_seqboot.hip), one workgroup per run: a bagging ensemble asks for one run per tree in one call."""
from __future__ import annotations

import ctypes as C
import operator
from typing import Optional

import numpy as np
from numpy.typing import NDArray

from .. import _ffi
from .._ffi import c_i64, ptr

MAX_EVENTS, MAX_DRAWS, MAX_WORDS, MAX_AXIS = (1 << 31) - 1, 1 << 24, 1 << 40, 1 << 32
UNIT = float(1 << 30)              # the library's uniqueness values count in units of 2^-30


def _spans(what, event_idxs, touch_idxs, n):
    ev, tc = np.asarray(event_idxs), np.asarray(touch_idxs)
    if ev.ndim != 1 or tc.ndim != 1 or (ev.size and ev.dtype.kind not in "iu") or (tc.size and tc.dtype.kind not in "iu"):
        raise ValueError(f"{what}: event_idxs and touch_idxs must be one-dimensional integer arrays.")
    if len(ev) != len(tc):
        raise ValueError(f"{what}: event_idxs and touch_idxs must have the same length.")
    if not 1 <= len(ev) <= MAX_EVENTS:
        raise ValueError(f"{what}: n_events must be between 1 and 2^31 - 1.")
    ev, tc = np.ascontiguousarray(ev, dtype=np.int64), np.ascontiguousarray(tc, dtype=np.int64)
    n = int(tc.max()) + 1 if n is None else operator.index(n)
    if not 0 <= n <= MAX_AXIS:
        raise ValueError(f"{what}: n must be between 0 and 2^32.")
    bad = int(np.count_nonzero((ev < 0) | (tc < ev) | (tc >= n)))
    if bad:
        raise ValueError(f"{what}: {bad} events outside 0 <= event_idx <= touch_idx < {n}")
    return ev, tc, n


def check_arguments(n_events, n_draws, n_runs, seed, draws_per_launch):
    """What the library refuses (FMK_E_ARG) of its scalar arguments, asked before anything reaches a device
    -> (n_draws, n_runs, seed mod 2^64, draws_per_launch) as ints."""
    try:
        n_draws = n_events if n_draws is None else operator.index(n_draws)
        n_runs, seed = operator.index(n_runs), operator.index(seed)
        draws_per_launch = 0 if draws_per_launch is None else operator.index(draws_per_launch)
    except TypeError:
        raise ValueError("sequential_bootstrap: n_draws, n_runs, seed and draws_per_launch must be integers.") from None
    if not 1 <= n_draws <= MAX_DRAWS:
        raise ValueError("sequential_bootstrap: n_draws must be between 1 and 2^24.")
    if n_runs < 1 or n_runs * n_draws > MAX_WORDS:
        raise ValueError("sequential_bootstrap: n_runs must be at least 1 and n_runs * n_draws at most 2^40.")
    if draws_per_launch < 0:
        raise ValueError("sequential_bootstrap: draws_per_launch must not be negative.")
    return n_draws, n_runs, seed & ((1 << 64) - 1), draws_per_launch


def geometry() -> dict:
    """The kernel's geometry (fmk_seqboot_geometry): needs no device."""
    out = (C.c_int64 * 3)()
    _ffi.check(_ffi.lib().fmk_seqboot_geometry(out))
    return dict(zip(("threads", "lds_intervals", "draws_per_launch"), (int(v) for v in out)))


def sequential_bootstrap(event_idxs: NDArray[np.int64], touch_idxs: NDArray[np.int64], n_draws: Optional[int] = None, n_runs: int = 1,
                         seed: int = 0, *, n: Optional[int] = None, words: Optional[NDArray[np.uint64]] = None,
                         return_uniqueness: bool = False, draws_per_launch: Optional[int] = None):
    """-> draws, int64 of shape (n_runs, n_draws): positions in event_idxs / touch_idxs (what `triple_barrier` and `trend_scanning`
    return), one sequential-bootstrap sample per row; with return_uniqueness also a float64 array of the same shape, the average
    uniqueness of each drawn event at the moment it was drawn, itself counted (a multiple of 2^-30: exact).  n_draws: the size of
    a sample (default: the number of events); n: the length of the axis the spans live on (default max(touch_idxs) + 1; it only
    bounds the events); seed: the runs of a call and the calls of different seeds are independent, equal seeds give equal samples;
    words: n_runs * n_draws uint64 random words that replace the generator's (tests steer a draw with them); draws_per_launch:
    how many draws one kernel launch makes (None: the library's choice), which changes nothing in the result.
    ValueError: no events, lengths that differ, an event outside 0 <= event_idx <= touch_idx < n, n_draws outside 1 .. 2^24,
    n_runs < 1 or n_runs * n_draws > 2^40, n > 2^32."""
    ev, tc, n = _spans("sequential_bootstrap", event_idxs, touch_idxs, n)
    n_draws, n_runs, seed, draws_per_launch = check_arguments(len(ev), n_draws, n_runs, seed, draws_per_launch)
    if words is not None:
        words = np.asarray(words)
        if words.dtype != np.uint64 or words.size != n_runs * n_draws:
            raise ValueError("sequential_bootstrap: words must be n_runs * n_draws uint64 values.")
        words = np.ascontiguousarray(words).reshape(-1)
    draws = np.empty((n_runs, n_draws), np.int64)
    q = np.empty((n_runs, n_draws), np.int64) if return_uniqueness else None
    _ffi.default_context().call("fmk_sequential_bootstrap", ptr(ev), ptr(tc), c_i64(len(ev)), c_i64(n), c_i64(n_draws), c_i64(n_runs),
                                C.c_uint64(seed), ptr(words), c_i64(draws_per_launch), ptr(draws), ptr(q))
    return (draws, q / UNIT) if return_uniqueness else draws


def bootstrap_uniqueness(event_idxs: NDArray[np.int64], touch_idxs: NDArray[np.int64], draws: NDArray[np.int64],
                         n: Optional[int] = None) -> float:
    """The mean average uniqueness of a sample (AFML section 4.5.4's comparison): `draws` are positions in the event arrays, with
    their multiplicities; the concurrency is counted over the sample alone, every member's average uniqueness is the mean of
    1 / concurrency over its span, and the result is their mean.  Runs on label_concurrency / label_weights (1e-9 relative).
    ValueError: an empty sample, a draw outside the events, a sample whose concurrency would pass int16 (32 767)."""
    ev, tc, n = _spans("bootstrap_uniqueness", event_idxs, touch_idxs, n)
    d = np.asarray(draws)
    if d.ndim != 1 or d.size == 0 or d.dtype.kind not in "iu":
        raise ValueError("bootstrap_uniqueness: draws must be a non-empty one-dimensional integer array (one sample).")
    if int(d.min()) < 0 or int(d.max()) >= len(ev):
        raise ValueError(f"bootstrap_uniqueness: a draw outside [0, {len(ev)})")
    sev, stc = np.ascontiguousarray(ev[d]), np.ascontiguousarray(tc[d])
    # the largest concurrency of the sample, from its sorted boundaries (an end before a start at the same position)
    at = np.concatenate([sev, stc + 1])
    step = np.concatenate([np.ones(len(sev), np.int64), -np.ones(len(sev), np.int64)])
    order = np.lexsort((step, at))
    if int(np.cumsum(step[order]).max()) > np.iinfo(np.int16).max:
        raise ValueError("bootstrap_uniqueness: the sample's concurrency passes int16 (32767).")
    ne = len(sev)
    concurrency, weights = np.zeros(n, np.int16), np.zeros(ne, np.float64)
    ctx = _ffi.default_context()
    ctx.call("fmk_label_concurrency", ptr(sev), ptr(stc), c_i64(ne), c_i64(n), ptr(concurrency))
    ctx.call("fmk_label_weights", None, ptr(concurrency), c_i64(n), ptr(sev), ptr(stc), c_i64(ne), ptr(weights), None)
    return float(np.mean(weights))
