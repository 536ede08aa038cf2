"""CPU-only checks of the sequential bootstrap: the definition in tests/_seqboot_ref.py in its two forms against
each other and on the book's example, the host program of csrc/fmk_seqboot_rule.h against it, the refusals of the Python layer, and
the property the feature exists for, on the reference alone.  The inputs are recorded here as functions; tests/test_gpu_seqboot.py
and tests/test_gpu_seqboot_edges.py import them."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _seqboot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 30

# AFML §4.5.3's example: three labels over six bars
BOOK = (np.array([0, 2, 4], np.int64), np.array([2, 3, 5], np.int64), 6)
BOOK_WORDS = np.array([1 << 63, 0], np.uint64)                # the middle of the total draws event 1, then 0 draws event 0
BOOK_Q_AFTER_1 = (894784853, 1 << 29, 1 << 30)                # 5/6, 1/2, 1 in units of 2^-30


def ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def random_spans(m, seed, max_len=40, dup_every=7):
    """m events in no order on an axis of 3 m + 50 positions, spans of 1 .. max_len positions, every dup_every-th one a copy of an
    earlier event -> (event_idx, touch_idx, n), read-only."""
    rng = np.random.default_rng(seed)
    n = 3 * m + 50
    ev = rng.integers(0, n, m)
    tc = np.minimum(ev + rng.integers(0, max_len, m), n - 1)
    for i in range(dup_every, m, dup_every):
        j = int(rng.integers(0, i))
        ev[i], tc[i] = ev[j], tc[j]
    return ro(ev.astype(np.int64), tc.astype(np.int64)) + (n,)


@functools.lru_cache(maxsize=None)
def spans_with_intervals(J, extra=150, seed=5):
    """Events whose boundaries cut the axis into exactly J intervals: J adjacent spans of 1 .. 4 positions, in no order, and `extra`
    longer events between boundaries that are there already -> (event_idx, touch_idx, n), read-only."""
    rng = np.random.default_rng(seed + J)
    b = np.concatenate([[0], np.cumsum(rng.integers(1, 5, J))])
    ev, tc = b[:-1].copy(), b[1:] - 1
    a = rng.integers(0, J, extra)
    z = np.minimum(a + rng.integers(1, 60, extra), J)
    ev, tc = np.concatenate([ev, b[a]]), np.concatenate([tc, b[z] - 1])
    order = rng.permutation(len(ev))
    ev, tc = ev[order].astype(np.int64), tc[order].astype(np.int64)
    assert len(R.compress(ev, tc)[0]) == J
    return ro(ev, tc) + (int(b[-1]),)


@functools.lru_cache(maxsize=None)
def property_spans():
    """The property test's inputs: 400 events with spans of 20 .. 300 positions on an axis of 20 000."""
    rng = np.random.default_rng(404)
    n, m = 20_000, 400
    L = rng.integers(20, 301, m)
    ev = rng.integers(0, n - L + 1)
    return ro(ev.astype(np.int64), (ev + L - 1).astype(np.int64)) + (n,)


def recorded_cases():
    """(event_idx, touch_idx, n, n_draws, n_runs, seed, words or None): what the host program is compared on"""
    out = [BOOK + (2, 1, 0, BOOK_WORDS), BOOK + (6, 3, 11, None)]
    for m, seed in ((1, 1), (2, 2), (17, 3), (90, 4)):
        out.append(random_spans(m, seed) + (min(m + 3, 25), 2, 100 + seed, None))
    ev, tc, n = random_spans(30, 9)
    out.append((ev, tc, n, 8, 2, 0, np.array([0, (1 << 64) - 1] * 8, np.uint64)))
    out.append((np.array([0, 7, (1 << 32) - 9], np.int64), np.array([(1 << 32) - 1, 7, (1 << 32) - 1], np.int64), 1 << 32, 12, 1, 5, None))
    return out


# ---------------------------------------------------------------------------------------------- the inputs of tests/test_gpu_seqboot_edges.py
SB_BATCH = 8                       # csrc/fmk_seqboot.hip SB_BATCH: the loads a thread keeps in flight; sb_draws walks its runs in such groups
BATCH_M = (8191, 8192, 8193, 16384, 16385)          # events: 8, 8, 9, 16, 17 per thread
BATCH_J = (7168, 8191, 16383, 16384)                # intervals: 8 per thread (with a spare row place, and to the last place), 16, 17
BATCH_LAST_M = (8199, 16388)                        # whole runs of 9 and 17 events: the last event closes the second and the third group
BATCH_EXTRA = 40


def runs_per_thread(ev, tc, threads):
    """-> (ept, ipt): the events and the intervals of a thread's run, as the library sizes them"""
    return -(-len(ev) // threads), len(R.compress(ev, tc)[0]) // threads + 1


def batch_passes(n):
    """-> (full groups of SB_BATCH, remainder) of a run of n elements"""
    return divmod(n, SB_BATCH)


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("seed", range(12))
def test_brute_force_equals_compressed_form(seed):
    rng = np.random.default_rng(seed)
    m = int(rng.integers(1, 15))
    ev, tc, n = random_spans(m, 50 + seed, max_len=int(rng.integers(1, 30)), dup_every=4)
    K, runs = int(rng.integers(1, 30)), int(rng.integers(1, 4))
    words = None if seed % 3 else R.words_of(seed, runs, K) | np.uint64(1 << 63)
    a, b = R.brute(ev, tc, n, K, runs, seed, words), R.compressed(ev, tc, n, K, runs, seed, words)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].min() >= 0 and a[0].max() < m and np.all(a[1][:, 0] == ONE)


def test_book_example_with_steering_words():
    ev, tc, n = BOOK
    for form in (R.brute, R.compressed):
        draws, q = form(ev, tc, n, 2, 1, 0, BOOK_WORDS)
        assert draws.tolist() == [[1, 0]] and q.tolist() == [[ONE, BOOK_Q_AFTER_1[0]]]
    assert tuple(R.uniqueness_given(ev, tc, n, [1])) == BOOK_Q_AFTER_1
    assert [round(x / ONE, 6) for x in BOOK_Q_AFTER_1] == [round(5 / 6, 6), 0.5, 1.0]


def test_extreme_words_draw_the_first_and_the_last_event():
    ev, tc, n = random_spans(17, 3)
    lo, hi = np.zeros(5, np.uint64), np.full(5, (1 << 64) - 1, np.uint64)
    assert R.compressed(ev, tc, n, 5, 1, 0, lo)[0].tolist() == [[0] * 5]
    assert R.compressed(ev, tc, n, 5, 1, 0, hi)[0].tolist() == [[16] * 5]


def test_word_generator_is_splitmix64():
    # splitmix64 seeded with 0: its first outputs (the generator's published test vector)
    assert [R.word(0, i) for i in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert R.word(5, 7) == R.word(5 + 0x9E3779B97F4A7C15, 6)


# ---------------------------------------------------------------------------------------------- the property
def test_sequential_samples_are_more_unique_than_plain_ones():
    ev, tc, n = property_spans()
    m, runs = len(ev), 16
    seq = R.compressed(ev, tc, n, m, runs, 2024)[0]
    pl = R.plain(m, m, runs, 2024)
    us = np.array([R.mean_uniqueness(ev, tc, n, s) for s in seq])
    up = np.array([R.mean_uniqueness(ev, tc, n, s) for s in pl])
    print(f"mean uniqueness over {runs} runs: sequential {us.mean():.4f}, plain {up.mean():.4f}; runs ahead {int((us > up).sum())}")
    assert us.mean() > up.mean()


# ---------------------------------------------------------------------------------------------- the host program
@functools.lru_cache(maxsize=None)
def check_program():
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(prefix="seqboot_check_"), "seqboot_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "seqboot_check.cpp"), "-o", exe])
    return exe


def case_text(ev, tc, n, K, runs, seed, words):
    nums = [len(ev), n, K, runs, seed, 0 if words is None else len(words)]
    nums += [int(x) for pair in zip(ev, tc) for x in pair] + ([] if words is None else [int(w) for w in words])
    return " ".join(str(x) for x in nums) + "\n"


def test_host_program_equals_the_reference_on_the_recorded_cases():
    cases = recorded_cases()
    r = subprocess.run([check_program()], input="".join(case_text(*c) for c in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2 * len(cases)
    for k, (ev, tc, n, K, runs, seed, words) in enumerate(cases):
        draws, q = R.compressed(ev, tc, n, K, runs, seed, words)
        d_line, q_line = lines[2 * k].split(), lines[2 * k + 1].split()
        assert d_line[0] == "draws" and q_line[0] == "q"
        assert [int(x) for x in d_line[1:]] == draws.reshape(-1).tolist(), k
        assert [int(x) for x in q_line[1:]] == q.reshape(-1).tolist(), k


def test_host_program_self_check():
    r = subprocess.run([check_program()], stdin=subprocess.DEVNULL, capture_output=True, text=True)
    assert r.returncode == 0 and "failed checks 0" in r.stdout, r.stdout
    assert int(re.search(r"cases (\d+)", r.stdout).group(1)) >= 400 and int(re.search(r"whole-axis draws (\d+)", r.stdout).group(1)) >= 200


# ---------------------------------------------------------------------------------------------- the Python layer's refusals
def test_python_layer_refuses_before_any_device_call():
    code = r"""
import numpy as np, pandas as pd, pytest
from finmlkit_amd import _ffi
from finmlkit_amd.label import sequential_bootstrap as f, bootstrap_uniqueness as u, SampleWeights
from finmlkit_amd.engine import DeviceTrades
ev, tc = np.array([0, 2, 4]), np.array([2, 3, 5])
for bad, msg in (((ev, tc[:2]), "same length"), ((ev[:0], tc[:0]), "n_events"), ((ev.astype(float), tc), "integer arrays"),
                 ((ev.reshape(3, 1), tc), "one-dimensional"), ((tc, ev), "3 events outside"), ((np.array([-1]), np.array([0])), "1 events outside")):
    with pytest.raises(ValueError, match=msg):
        f(*bad)
    with pytest.raises(ValueError, match=msg):
        u(*bad, np.array([0]))
for kw, msg in ((dict(n=5), "1 events outside 0 <= event_idx <= touch_idx < 5"), (dict(n=(1 << 32) + 1), "2\\^32"), (dict(n=-1), "2\\^32"),
                (dict(n_draws=0), "n_draws"), (dict(n_draws=(1 << 24) + 1), "n_draws"), (dict(n_runs=0), "n_runs"),
                (dict(n_draws=1 << 20, n_runs=(1 << 20) + 1), "2\\^40"), (dict(n_draws=1.5), "integers"), (dict(draws_per_launch=-1), "negative"),
                (dict(words=np.zeros(2, np.uint64)), "words"), (dict(words=np.zeros(3, np.int64)), "words")):
    with pytest.raises(ValueError, match=msg):
        f(ev, tc, **kw)
for d, msg in ((np.array([], np.int64), "non-empty"), (np.array([[0]]), "one-dimensional"), (np.array([3]), "outside"), (np.array([-1]), "outside"),
               (np.array([0.0]), "integer"), (np.zeros(32768, np.int64), "int16")):
    with pytest.raises(ValueError, match=msg):
        u(ev, tc, d)
with pytest.raises(ValueError, match="DataFrame"):
    SampleWeights.sequential_bootstrap(np.zeros(3))
with pytest.raises(ValueError, match="event_idx"):
    SampleWeights.sequential_bootstrap(pd.DataFrame({"event_idx": [1]}))
class Col:
    def __init__(self, n, dtype=np.int64): self.n, self.dtype, self.p = n, np.dtype(dtype), None
t = DeviceTrades(None, Col(9), Col(9, np.float64), Col(9, np.float32), None)
with pytest.raises(ValueError, match="same length"):
    t.sequential_bootstrap(Col(3), Col(2))
with pytest.raises(TypeError, match="int64"):
    t.sequential_bootstrap(Col(3), Col(3, np.int32))
with pytest.raises(ValueError, match="n_events"):
    t.sequential_bootstrap(Col(0), Col(0))
with pytest.raises(ValueError, match="n_draws"):
    t.sequential_bootstrap(Col(3), Col(3), n_draws=0)
assert _ffi._lib is None and _ffi._default_ctx is None
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_header_declares_and_library_exports_the_entry_points():
    from finmlkit_amd import _ffi
    from finmlkit_amd.label import bootstrap
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmk.h")).read(), flags=re.S)
    for s in ("fmk_sequential_bootstrap", "fmk_sequential_bootstrap_dev", "fmk_seqboot_geometry"):
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(_ffi.lib(), s), s
    assert "fmk_seqboot.hip" in open(os.path.join(ROOT, "finmlkit_amd", "csrc", "Makefile")).read()
    g = bootstrap.geometry()                                  # needs no device
    assert g["threads"] == 1024 and g["draws_per_launch"] >= 1
    assert 12 * g["lds_intervals"] + 8 <= 64 * 1024           # c (4 B) and P (8 B) per interval, one more P, in static LDS


# ---------------------------------------------------------------------------------------------- what the batched-loop cases hold
def test_batch_cases_go_round_the_batched_loops_twice_with_and_without_a_remainder():
    from finmlkit_amd.label import bootstrap
    g = bootstrap.geometry()
    T = g["threads"]
    by_m = {m: runs_per_thread(*random_spans(m, m)[:2], T) for m in BATCH_M + BATCH_LAST_M}
    by_j = {J: runs_per_thread(*spans_with_intervals(J, extra=BATCH_EXTRA)[:2], T) for J in BATCH_J}
    print("m -> (ept, ipt)", by_m, "J -> (ept, ipt)", by_j)
    ept = {v[0] for v in by_m.values()}
    ipt = {v[1] for v in list(by_m.values()) + list(by_j.values())}
    assert [by_m[m][0] for m in BATCH_M] == [8, 8, 9, 16, 17] and {8, 9, 16, 17} <= ept
    assert [by_j[J][1] for J in BATCH_J] == [8, 8, 16, 17] and 8 in ipt and max(ipt) >= 16
    assert all(ip > g["lds_intervals"] // T + 1 for _, ip in list(by_m.values()) + list(by_j.values()))       # all the scratch flavour
    for runs in (ept, ipt):                                              # steps 2 and 3 walk ept, step 1 walks ipt
        passes = {batch_passes(n) for n in runs}
        assert (1, 0) in passes                                          # one full group, an empty remainder
        assert any(full >= 2 and rest == 0 for full, rest in passes)     # twice round, an empty remainder
        assert any(full >= 2 and rest > 0 for full, rest in passes)      # twice round and a remainder
    # J = 7168 leaves whole threads without intervals and the end of the last interval a place in row 0; J = 8191 fills every place
    assert by_j[7168][1] * T - 7168 == T and by_j[8191][1] * T - 8191 == 1
    for m in BATCH_M + BATCH_LAST_M:
        assert len(set(zip(*[a.tolist() for a in random_spans(m, m)[:2]]))) < m        # duplicates among the events
    # the last event: which thread owns it, and in which group of its run it lies
    last = {m: divmod(m - 1, by_m[m][0]) for m in BATCH_M + BATCH_LAST_M}
    assert [last[m][1] // SB_BATCH for m in BATCH_LAST_M] == [1, 2] and all(last[m][1] == by_m[m][0] - 1 for m in BATCH_LAST_M)
    assert last[8193] == (910, 2) and last[16385] == (963, 13)           # a short last run, in the first and in the second group
