"""CPU-only checks of the imbalance / run bar indexers: the defining loops (tests/_flowbars_ref.py) on hand-written tapes whose closes
are written out, the identity the GPU tests lean on (a stretch of side-0 ticks changes no state), the host restatement of the
certificate, the C ABI's declarations and exports, and the argument errors that are raised before any device call."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _flowbars_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------- the loops, by hand
def test_an_exact_tie_closes():
    # theta: 1, 2, 3 (== thr: close), 1, 0, -1, -2, -3 (== -thr: close), 1
    assert R.imbalance([1, 1, 1, 1, -1, -1, -1, -1, 1], [1.0] * 9, 3.0) == [0, 2, 7]
    # up: 1, 2, 3 (close); then dn: 1, 2, 3 (close)
    assert R.run([1, 1, 1, -1, -1, -1, 1], [1.0] * 7, 3.0) == [0, 2, 5]
    assert R.imbalance([1, 1, 1], [1.0, 1.0, 0.999], 3.0) == [0]


def test_a_side_of_zero_contributes_nothing():
    assert R.imbalance([1, 0, 0, 1, 0, 1], [1.0, 50.0, 50.0, 1.0, 50.0, 1.0], 3.0) == [0, 5]
    assert R.run([1, 0, 0, 1, 0, 1], [1.0, 50.0, 50.0, 1.0, 50.0, 1.0], 3.0) == [0, 5]


def test_tick_zero_is_counted_but_cannot_close():
    # |x[0]| >= thr: no close at 0; tick 1 sees theta = 5 + 1 and closes
    assert R.imbalance([1, 1, 1, 1], [5.0, 1.0, 1.0, 1.0], 3.0) == [0, 1]
    assert R.imbalance([1, -1, 1, 1], [5.0, 1.0, 1.0, 1.0], 3.0) == [0, 1]        # theta = 4 at tick 1
    assert R.imbalance([1, -1, -1, -1], [3.0, 1.0, 1.0, 1.0], 3.0) == [0]         # 2, 1, 0: tick 0 was counted
    assert R.run([-1, 1, 1], [5.0, 1.0, 1.0], 3.0) == [0, 1]                      # dn = 5 from tick 0 closes at tick 1
    assert R.imbalance([1], [5.0], 3.0) == [0] and R.run([1], [5.0], 3.0) == [0]
    assert R.imbalance([], [], 3.0) == [0] and R.run([], [], 3.0) == [0]


def test_run_bars_close_on_the_sell_side_and_are_not_consecutive_runs():
    # buys and sells alternate: neither total is a "run" of consecutive ticks, the sell total reaches 3 first
    assert R.run([1, -1, -1, 1, -1, 1], [0.5, 1.0, 1.0, 0.5, 1.0, 0.5], 3.0) == [0, 4]
    # the imbalance of the same tape never gets there
    assert R.imbalance([1, -1, -1, 1, -1, 1], [0.5, 1.0, 1.0, 0.5, 1.0, 0.5], 3.0) == [0]


def test_nan_amount():
    b, q = [1, 1, 1, 1, -1, -1, -1, 1, 1, 1], [1.0, 1.0, 1.0, NAN, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    # imbalance: closes at 2, then theta is NaN for good
    assert R.imbalance(b, q, 3.0) == [0, 2]
    # run: up is NaN from tick 3 on and never closes; dn reaches 3 at tick 6 and the close clears both; then up: 1, 2, 3
    assert R.run(b, q, 3.0) == [0, 2, 6, 9]
    # a side of 0 with a NaN size: 0 * NaN is NaN for the imbalance sum, and nothing for the run totals
    assert R.imbalance([1, 0, 1, 1, 1], [1.0, NAN, 1.0, 1.0, 1.0], 3.0) == [0]
    assert R.run([1, 0, 1, 1, 1], [1.0, NAN, 1.0, 1.0, 1.0], 3.0) == [0, 3]


def test_thresholds_outside_the_tables_domain_do_what_the_comparisons_do():
    b, q = [1, -1, 1, 1], [1.0, 1.0, 1.0, 1.0]
    assert R.imbalance(b, q, 0.0) == [0, 1, 2, 3] and R.run(b, q, -1.0) == [0, 1, 2, 3]
    assert R.imbalance(b, q, NAN) == [0] and R.run(b, q, NAN) == [0] and R.imbalance(b, q, INF) == [0]
    assert R.imbalance([1, 1], [1.0, INF], INF) == [0, 1]


def test_closes_takes_numpy_columns_and_kinds():
    px = np.array([10.0, 10.0, 20.0, 20.0, 20.0])
    am = np.array([1.0, 1.0, 1.0, 1.0, 1.0], np.float32)
    sd = np.array([1, 1, 1, 1, 1], np.int8)
    assert R.closes("imbalance", "tick", px, am, sd, 2).tolist() == [0, 1, 3]
    assert R.closes("run", "dollar", px, am, sd, 40).tolist() == [0, 2, 4]
    assert R.closes("run", "volume", px, am, sd, 3).dtype == np.int64


# ---------------------------------------------------------------------------------------------- the identity behind the long-bar tests
@pytest.mark.parametrize("rule", ["imbalance", "run"])
@pytest.mark.parametrize("at", [1, 700, 4095])
def test_a_quiet_stretch_shifts_the_closes(rule, at):
    cols = R.recipe(4097)
    want = R.closes(rule, "volume", *cols, 8.0)
    assert len(want) > 3
    px, am, sd = R.with_quiet_stretch(cols, at, 300)
    assert len(sd) == 4397 and not sd[at:at + 300].any() and sd[at + 300] == cols[2][at]
    got = R.closes(rule, "volume", px, am, sd, 8.0)
    assert np.array_equal(got, R.shifted(want, at, 300))


# ---------------------------------------------------------------------------------------------- the certificate on the host
def test_low_bit_exp():
    assert R.low_bit_exp([1.0]) == 0 and R.low_bit_exp([0.0, 6.0]) == 1 and R.low_bit_exp([0.75, 8.0]) == -2
    assert R.low_bit_exp([0.0]) is None and R.low_bit_exp([5e-324]) == -1074 and R.low_bit_exp([2.0 ** -40, 2.0 ** 20]) == -40
    assert R.low_bit_exp([np.float32(0.001)]) >= -33


def test_certificate_predictions():
    px, am, sd = R.recipe(4097)
    assert R.certifies("imbalance", "volume", px, am, sd, 8.0) and R.certifies("run", "dollar", px, am, sd, 64.0)
    big = np.full(64, 2.0 ** 20, np.float32)
    big[5] = 2.0 ** -40
    assert not R.certifies("imbalance", "volume", np.ones(64), big, np.ones(64, np.int8), 8.0)       # 2^26 / 2^-40 > 2^53
    # milli-lots: the quantum is 2^-33 at the worst, 2^20 ticks sum to about 2^19: just inside
    px, am, sd = R.recipe((1 << 20) + 1, "milli")
    assert R.low_bit_exp(am.astype(np.float64)) >= -33 and R.certifies("imbalance", "volume", px, am, sd, 5.0)
    # prices with a full mantissa: the products do not share a usable quantum
    rng = np.random.default_rng(3)
    walk = 100.0 * np.exp(np.cumsum(1e-4 * rng.standard_normal(4097)))
    assert not R.certifies("imbalance", "dollar", walk, R.recipe(4097)[1], R.recipe(4097)[2], 1000.0)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_library_exports_the_entry_points():
    from finmlkit_amd import _ffi
    for header, names in (("fmk.h", ("fmk_flow_bar_indexer_dev",)), ("fmk_diag.h", ("fmk_diag_flowbars_last",))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for s in names:
            assert re.search(r"\b%s\s*\(" % s, txt), s
            assert hasattr(_ffi.lib(), s), s
    assert "fmk_flowbars.hip" in open(os.path.join(ROOT, "finmlkit_amd", "csrc", "Makefile")).read()
    from finmlkit_amd import bar
    from finmlkit_amd.bar import kit
    assert bar.ImbalanceBarKit is kit.ImbalanceBarKit and bar.RunBarKit is kit.RunBarKit
    assert issubclass(kit.ImbalanceBarKit, kit._ThresholdKit) and issubclass(kit.RunBarKit, kit._ThresholdKit)


def test_search_and_certificate_on_the_host(tmp_path):
    """tools/flowbars_check.cpp, built from the header with the host compiler alone (no HIP), in its quick form: every link of random
    tapes against the loop, the certificate's edges, the quantum of random doubles.  (The full run under ASan / UBSan is a tool run,
    not part of the suite.)"""
    exe = str(tmp_path / "flowbars_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "flowbars_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "quick"], capture_output=True, text=True)
    assert r.returncode == 0 and "failed checks 0" in r.stdout, r.stdout
    assert int(re.search(r"links compared (\d+)", r.stdout).group(1)) > 100_000


# ---------------------------------------------------------------------------------------------- argument errors, no device
def test_argument_errors_come_before_any_device_call():
    code = r"""
import numpy as np, pytest
from finmlkit_amd import _ffi
from finmlkit_amd.bar import logic as L
from finmlkit_amd.engine import DeviceTrades
ts, px, am, sd = np.arange(5), np.ones(5), np.ones(5, np.float32), np.ones(5, np.int8)
for f in (L._imbalance_bar_indexer, L._run_bar_indexer):
    with pytest.raises(ValueError, match="kind must be one of"):
        f(ts, px, am, 3.0, kind="lots", sides=sd)
    with pytest.raises(ValueError, match="same length"):
        f(ts[:4], px, am, 3.0, sides=sd)
    with pytest.raises(ValueError, match="same length"):
        f(ts, px, am[:3], 3.0, sides=sd)
    with pytest.raises(ValueError, match="same length"):
        f(ts, px, am, 3.0, kind="tick", sides=sd[:2])
    out = f(ts[:0], px[:0], am[:0], 3.0)
    assert out.dtype == np.int64 and out.tolist() == [0]
class Cols:
    n = 5
t = DeviceTrades(None, Cols, Cols, np.ones(5, np.float32), None)
for f in (t.imbalance_bar_index, t.run_bar_index):
    with pytest.raises(ValueError, match="side column"):
        f(3.0)
    with pytest.raises(ValueError, match="kind must be one of"):
        f(3.0, kind="lots")
assert _ffi._lib is None and _ffi._default_ctx is None
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

