"""GPU: the sequential bootstrap (csrc/fmk_seqboot.hip) where a thread's runs are longer than one batch of loads, against
tests/_seqboot_ref.py, bit-equal on the draws and on Q.  8, 9, 16 and 17 events per thread and 8, 16, 17 and more intervals per
thread: the batched loops of steps 1, 2 and 3 of sb_draws go round once without a remainder, twice without one and twice with one.
The inputs are tests/test_seqboot_host.py's, which asserts these counts from the geometry."""
import time

import numpy as np
import pytest

from tests import _seqboot_ref as R
from tests.test_gpu_seqboot import U64_MAX, assert_equals_reference, gpu
from tests.test_seqboot_host import BATCH_EXTRA, BATCH_J, BATCH_LAST_M, BATCH_M, random_spans, spans_with_intervals

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m", BATCH_M)
def test_event_runs_of_one_and_two_batches(m):
    ev, tc, n = random_spans(m, m)
    t0 = time.perf_counter()
    assert_equals_reference(ev, tc, n, 24, runs=2, seed=m)
    print(f"m = {m}: {time.perf_counter() - t0:.3f} s with the reference")


@pytest.mark.parametrize("J", BATCH_J)
def test_interval_runs_of_one_and_two_batches(J):
    ev, tc, n = spans_with_intervals(J, extra=BATCH_EXTRA)
    assert len(R.compress(ev, tc)[0]) == J
    assert_equals_reference(ev, tc, n, 24, runs=2, seed=J)


@pytest.mark.parametrize("m", (8193, 16385) + BATCH_LAST_M)
def test_extreme_words_in_the_later_batches(m):
    ev, tc, n = random_spans(m, m)
    K = 6
    t0 = time.perf_counter()
    d, _ = assert_equals_reference(ev, tc, n, K, words=np.zeros(K, np.uint64))
    assert np.all(d == 0)
    d, _ = assert_equals_reference(ev, tc, n, K, words=np.full(K, U64_MAX, np.uint64))
    assert np.all(d == m - 1)
    print(f"m = {m}: {time.perf_counter() - t0:.3f} s with the reference")


def test_draws_per_launch_changes_nothing_with_nine_events_per_thread():
    m = 8193
    ev, tc, n = random_spans(m, m)
    K = 23
    ref = R.compressed(ev, tc, n, K, 2, 77)
    for dpl in (1, 7, None):
        got = gpu(ev, tc, n, K, 2, 77, dpl=dpl)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), dpl
