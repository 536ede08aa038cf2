"""GPU: the sequential bootstrap against the definition in tests/_seqboot_ref.py.  The definition is in integers, so
"equal" is bit-equal everywhere: the draws and each drawn event's Q.  Event counts over the edges of the threads' runs, interval
counts around the LDS capacity (both flavours of the kernel), every split of the draws into launches, the degenerate shapes, the
64-bit products at n = 2^32, the resident form and the kit, and every refusal of the C layer."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest

from tests import _seqboot_ref as R
from tests.test_seqboot_host import BOOK, BOOK_Q_AFTER_1, BOOK_WORDS, ONE, property_spans, random_spans, spans_with_intervals

pytestmark = pytest.mark.gpu

M_EDGES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 5000)
U64_MAX = (1 << 64) - 1


def gpu(ev, tc, n, K=None, runs=1, seed=0, words=None, dpl=None):
    """-> (draws, Q as integers) of the host-pointer form, int64 of shape (runs, K)"""
    from finmlkit_amd.label import sequential_bootstrap
    draws, u = sequential_bootstrap(ev, tc, K, runs, seed, n=n, words=words, return_uniqueness=True, draws_per_launch=dpl)
    K = len(ev) if K is None else K
    assert draws.dtype == np.int64 and u.dtype == np.float64 and draws.shape == u.shape == (runs, K)
    q = u * float(ONE)
    assert np.array_equal(q, np.rint(q))
    only = sequential_bootstrap(ev, tc, K, runs, seed, n=n, words=words, draws_per_launch=dpl)
    assert isinstance(only, np.ndarray) and np.array_equal(only, draws)
    return draws, q.astype(np.int64)


def assert_equals_reference(ev, tc, n, K, runs=1, seed=0, words=None, dpl=None):
    got = gpu(ev, tc, n, K, runs, seed, words, dpl)
    ref = R.compressed(ev, tc, n, K, runs, seed, words)
    assert np.array_equal(got[0], ref[0]), "draws"
    assert np.array_equal(got[1], ref[1]), "Q"
    return got


@functools.lru_cache(maxsize=None)
def geometry():
    from finmlkit_amd.label import bootstrap
    return bootstrap.geometry()


# ---------------------------------------------------------------------------------------------- the definition's landmarks
def test_book_example():
    ev, tc, n = BOOK
    draws, q = assert_equals_reference(ev, tc, n, 2, words=BOOK_WORDS)
    assert draws.tolist() == [[1, 0]] and q.tolist() == [[ONE, BOOK_Q_AFTER_1[0]]]
    # each candidate's Q after event 1: a word that lands in the candidate's share draws it
    total = sum(BOOK_Q_AFTER_1)
    for i, want in enumerate(BOOK_Q_AFTER_1):
        below = sum(BOOK_Q_AFTER_1[:i])
        w = ((below << 64) + total - 1) // total                       # the smallest word whose target reaches `below`
        d, q = gpu(ev, tc, n, 2, words=np.array([1 << 63, w], np.uint64))
        assert d.tolist() == [[1, i]] and q[0, 1] == want
    assert_equals_reference(ev, tc, n, 6, runs=3, seed=11)


@pytest.mark.parametrize("m", [3, 1025, 5000])
def test_extreme_words(m):
    ev, tc, n = random_spans(m, m)
    K = 6
    d, _ = assert_equals_reference(ev, tc, n, K, words=np.zeros(K, np.uint64))
    assert np.all(d == 0)
    d, _ = assert_equals_reference(ev, tc, n, K, words=np.full(K, U64_MAX, np.uint64))
    assert np.all(d == m - 1)


@pytest.mark.parametrize("m", M_EDGES)
def test_event_counts_over_the_thread_run_edges(m):
    g = geometry()
    assert g["threads"] == 1024 and {g["threads"] - 1, g["threads"], g["threads"] + 1, 2 * g["threads"] - 1, 2 * g["threads"] + 1} <= set(M_EDGES)
    ev, tc, n = random_spans(m, m)
    assert m < 8 or (len(set(zip(ev.tolist(), tc.tolist()))) < m and np.any(np.diff(ev) < 0))      # duplicates, no order
    assert_equals_reference(ev, tc, n, min(m, 48), runs=3, seed=m)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_interval_counts_at_the_lds_capacity(delta):
    J = geometry()["lds_intervals"] + delta
    ev, tc, n = spans_with_intervals(J)
    assert len(R.compress(ev, tc)[0]) == J
    assert_equals_reference(ev, tc, n, 40, runs=2, seed=J)


@pytest.mark.parametrize("J", [1023, 1024, 1025, 2048, 8192])
def test_interval_counts_at_the_row_edges(J):
    """A thread's run of intervals grows by one at every multiple of the thread count; at a multiple the end of the last interval
    opens a row of its own."""
    assert geometry()["threads"] == 1024
    ev, tc, n = spans_with_intervals(J, extra=40)
    assert_equals_reference(ev, tc, n, 30, runs=2, seed=J)


@pytest.mark.parametrize("m", [90, 5000])
def test_draws_per_launch_changes_nothing(m):
    ev, tc, n = random_spans(m, m)
    assert (len(R.compress(ev, tc)[0]) > geometry()["lds_intervals"]) == (m == 5000)
    K = 23
    ref = R.compressed(ev, tc, n, K, 2, 77)
    for dpl in (1, 7, K, None):
        got = gpu(ev, tc, n, K, 2, 77, dpl=dpl)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), dpl


def test_default_draws_per_launch_is_crossed():
    K = 2 * geometry()["draws_per_launch"] + 5
    ev, tc, n = random_spans(17, 3)
    assert_equals_reference(ev, tc, n, K, seed=8)


# ---------------------------------------------------------------------------------------------- degenerate shapes
def test_one_event_drawn_3000_times():
    d, q = gpu(np.array([4]), np.array([9]), 12, 3000)
    assert np.all(d == 0)
    assert q[0].tolist() == [ONE // (k + 1) for k in range(3000)]


def test_all_events_the_same_span():
    m = 50
    ev, tc = np.full(m, 3, np.int64), np.full(m, 40, np.int64)
    _, q = assert_equals_reference(ev, tc, 64, 80, runs=2, seed=3)
    assert q[0].tolist() == [ONE // (k + 1) for k in range(80)]


def test_disjoint_events_keep_full_uniqueness_until_drawn():
    m = 300
    ev = np.arange(m, dtype=np.int64)[::-1] * 5
    tc = ev + np.arange(m) % 5
    d, q = assert_equals_reference(ev, tc, 5 * m, 200, seed=21)
    seen = {}
    for i, qi in zip(d[0].tolist(), q[0].tolist()):
        assert qi == ONE // (seen.get(i, 0) + 1)                         # an undrawn event still has Q = 2^30
        seen[i] = seen.get(i, 0) + 1


def test_nested_spans():
    m = 120
    ev = np.arange(m, dtype=np.int64)
    tc = 2 * m - ev
    assert_equals_reference(ev, tc, 2 * m + 1, 60, runs=2, seed=4)


def test_spans_of_length_one():
    rng = np.random.default_rng(12)
    ev = rng.integers(0, 700, 1500).astype(np.int64)                     # many events on the same position
    assert_equals_reference(ev, ev.copy(), 700, 48, runs=2, seed=6)


def test_a_span_over_an_axis_of_2_to_the_32():
    n = 1 << 32
    ev = np.array([5, 0, n - 1, 0, 1 << 31, n - 4096, 77], np.int64)
    tc = np.array([70000, n - 1, n - 1, 0, (1 << 31) + 1, n - 1, 77], np.int64)
    K = 40
    words = R.words_of(9, 1, K)
    words[::2] = np.uint64(U64_MAX // 7 + 12345)                        # lands in event 1's share: the whole axis, again and again
    d, q = assert_equals_reference(ev, tc, n, K, words=words)
    assert (d == 1).sum() >= K // 2 and q[0, 0] == ONE
    assert_equals_reference(ev, tc, n, 30, runs=2, seed=1)


# ---------------------------------------------------------------------------------------------- runs and prefixes
def test_first_draws_of_run_0_do_not_depend_on_the_number_of_draws():
    ev, tc, n = random_spans(1025, 1025)
    long_, short = gpu(ev, tc, n, 30, 2, 5), gpu(ev, tc, n, 12, 2, 5)
    assert np.array_equal(long_[0][0, :12], short[0][0]) and np.array_equal(long_[1][0, :12], short[1][0])


def test_five_runs_equal_five_reference_runs():
    ev, tc, n = random_spans(2049, 2049)
    K, seed = 20, 31
    got = assert_equals_reference(ev, tc, n, K, runs=5, seed=seed)
    words = R.words_of(seed, 5, K)
    for r in range(5):
        one = R.compressed(ev, tc, n, K, 1, 0, words[r * K:(r + 1) * K])
        assert np.array_equal(got[0][r], one[0][0]) and np.array_equal(got[1][r], one[1][0])
    assert len({tuple(row) for row in got[0].tolist()}) == 5


# ---------------------------------------------------------------------------------------------- the other forms
def test_resident_form_and_kit_equal_the_host_form():
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.engine import DeviceTrades
    from finmlkit_amd.label import SampleWeights
    ev, tc, n = random_spans(1500, 15)
    t = DeviceTrades.from_numpy(np.arange(n, dtype=np.int64), np.ones(n), np.ones(n, np.float32))
    d_ev, d_tc = DeviceArray.from_host(t.ctx, ev), DeviceArray.from_host(t.ctx, tc)
    want = gpu(ev, tc, n, 25, 3, 19)
    draws, q = t.sequential_bootstrap(d_ev, d_tc, 25, 3, 19, return_uniqueness=True)
    assert isinstance(draws, DeviceArray) and draws.n == q.n == 75 and draws.dtype == q.dtype == np.int64
    assert np.array_equal(draws.to_host().reshape(3, 25), want[0]) and np.array_equal(q.to_host().reshape(3, 25), want[1])
    assert np.array_equal(t.sequential_bootstrap(d_ev, d_tc, 25, 3, 19).to_host(), want[0].reshape(-1))
    # default number of draws: one per event
    full = t.sequential_bootstrap(d_ev, d_tc, seed=2)
    assert full.n == len(ev)
    with pytest.raises(ValueError, match="events outside 0 <= event_idx <= touch_idx < 100"):
        DeviceTrades.from_numpy(np.arange(100, dtype=np.int64), np.ones(100), np.ones(100, np.float32)).sequential_bootstrap(d_ev, d_tc)
    # the kit: row positions of a frame of labels; its axis ends at the last touch
    frame = pd.DataFrame({"event_idx": ev, "touch_idx": tc, "labels": 1})
    rows = SampleWeights.sequential_bootstrap(frame, 25, 3, 19)
    ref = R.compressed(ev, tc, int(tc.max()) + 1, 25, 3, 19)[0]
    assert rows.shape == (3, 25) and np.array_equal(rows, ref) and np.array_equal(rows, want[0])
    assert SampleWeights.sequential_bootstrap(frame, seed=2).shape == (1, len(ev))


def test_bootstrap_uniqueness():
    from finmlkit_amd.label import bootstrap_uniqueness, sequential_bootstrap
    ev, tc, n = property_spans()
    m = len(ev)
    seq = sequential_bootstrap(ev, tc, n_runs=2, seed=2024, n=n)
    assert np.array_equal(seq, R.compressed(ev, tc, n, m, 2, 2024)[0])
    for sample in (seq[0], seq[1], R.plain(m, m, 1, 2024)[0], np.array([7])):
        got, want = bootstrap_uniqueness(ev, tc, sample, n=n), R.mean_uniqueness(ev, tc, n, sample)
        assert abs(got - want) <= 1e-9 * want, (got, want)
    assert bootstrap_uniqueness(ev, tc, np.array([7, 7, 7, 7])) == 0.25
    assert bootstrap_uniqueness(ev, tc, seq[0], n=n) > bootstrap_uniqueness(ev, tc, R.plain(m, m, 1, 2024)[0], n=n)


# ---------------------------------------------------------------------------------------------- the C layer's refusals
def test_c_layer_refuses():
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray, c_i64, ptr
    ctx = _ffi.default_context()
    ev, tc = np.array([0, 2, 4], np.int64), np.array([2, 3, 5], np.int64)
    out, q = np.full(8, -7, np.int64), np.full(8, -7, np.int64)
    d_ev, d_tc, d_out = DeviceArray.from_host(ctx, ev), DeviceArray.from_host(ctx, tc), DeviceArray.from_host(ctx, out)

    def host(m=3, n=6, K=2, runs=1, dpl=0, e=ev, t=tc, o=out):
        ctx.call("fmk_sequential_bootstrap", ptr(e), ptr(t), c_i64(m), c_i64(n), c_i64(K), c_i64(runs), C.c_uint64(0), None, c_i64(dpl),
                 ptr(o), ptr(q))

    def dev(m=3, n=6, K=2, runs=1, dpl=0, e=d_ev, t=d_tc, o=d_out):
        ctx.call("fmk_sequential_bootstrap_dev", e.p, t.p, c_i64(m), c_i64(n), c_i64(K), c_i64(runs), C.c_uint64(0), None, c_i64(dpl),
                 None if o is None else o.p, None)

    for call in (host, dev):
        for kw, msg in ((dict(m=0), "n_events"), (dict(m=-1), "n_events"), (dict(m=1 << 31), "n_events"), (dict(K=0), "n_draws"),
                        (dict(K=(1 << 24) + 1), "n_draws"), (dict(runs=0), "n_runs"), (dict(K=1 << 20, runs=(1 << 20) + 1), "2\\^40"),
                        (dict(runs=(1 << 40) + 1, K=1), "2\\^40"), (dict(n=(1 << 32) + 1), "2\\^32"), (dict(n=-1), "2\\^32"),
                        (dict(dpl=-1), "draws_per_launch"), (dict(o=None), "null output"),
                        (dict(n=5), "sequential_bootstrap: 1 events outside 0 <= event_idx <= touch_idx < 5"),
                        (dict(n=0), "3 events outside")):
            with pytest.raises(ValueError, match=msg):
                call(**kw)
    for e, t, msg in ((np.array([-1, 2, 4], np.int64), tc, "1 events outside"), (tc, ev, "3 events outside"),
                      (ev, np.array([2, 3, 6], np.int64), "1 events outside 0 <= event_idx <= touch_idx < 6")):
        with pytest.raises(ValueError, match=msg):
            host(e=e, t=t)
        with pytest.raises(ValueError, match=msg):
            dev(e=DeviceArray.from_host(ctx, e), t=DeviceArray.from_host(ctx, t))
    assert np.all(out == -7) and np.all(d_out.to_host() == -7)          # a refused call writes nothing
    host()                                                              # and the largest legal axis bound is accepted as such
    host(n=1 << 32)
    dev()
    assert np.all(out[:2] >= 0) and np.all(d_out.to_host()[:2] >= 0) and np.all(d_out.to_host()[2:] == -7)
