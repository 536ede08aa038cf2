"""CPU-only checks of the imbalance / run bar indexers: the defining loops (tests/_flowbars_ref.py) on hand-written tapes whose closes
are written out, the identity the GPU tests lean on (a stretch of side-0 ticks changes no state), the host restatement of the
certificate, the tapes and closed forms that tests/test_gpu_flowbars_edges.py leans on, the C ABI's declarations and exports, and the
argument errors that are raised before any device call."""
import math
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
def hand_check(group):
    """Every tape of R.HAND_TAPES[group] gives, under the loops, the closes that are written beside it."""
    for sides, sizes, thr, want in R.HAND_TAPES[group]:
        assert want
        for rule, idx in want.items():
            assert R.RULES[rule](sides, sizes, thr) == idx, (group, rule, sides, sizes)
    return len(R.HAND_TAPES[group])


def test_an_exact_tie_closes():
    assert hand_check("tie") == 3


def test_a_side_of_zero_contributes_nothing():
    assert hand_check("side_zero") == 1


def test_tick_zero_is_counted_but_cannot_close():
    assert hand_check("tick_zero") == 6


def test_run_bars_close_on_the_sell_side_and_are_not_consecutive_runs():
    assert hand_check("sell_side") == 1


def test_nan_amount():
    assert hand_check("nan_amount") == 2


def test_hand_tapes_as_columns():
    """What the GPU tests run: float32 amounts keep the written closes, 600 ticks of side 0 behind the tape add no close (but
    for the one-tick tape, whose tick 0 could not close), and the tapes without a NaN certify (the tables must answer them)."""
    for group, tapes in R.HAND_TAPES.items():
        for sides, sizes, thr, want in tapes:
            for pad in (0, 600):
                cols = R.hand_tape_columns(sides, sizes, pad)
                assert len(cols[0]) == len(sides) + pad and cols[1].dtype == np.float32 and cols[2].dtype == np.int8
                for rule in R.RULES:
                    got = R.closes(rule, "volume", *cols, thr).tolist()
                    loop = R.RULES[rule](sides, sizes, thr)
                    assert loop == want.get(rule, loop)
                    if len(sides) == 1 and pad:
                        assert got == [0, 1], (group, rule)         # tick 0 alone reached thr: the first tick behind it closes
                    else:
                        assert got == loop, (group, rule, pad)
                    if group != "nan_amount":
                        assert R.certifies(rule, "volume", *cols, thr), (group, rule, pad)


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


# ---------------------------------------------------------------------------------------------- the tapes of the edge tests
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("K", [1, 2, 7, 8, 9, 513])
def test_one_sided_closed_form(K, sign):
    for n in (3 * K + 5, 3 * K, 3 * K - 1):                        # an open last bar, a close on the last tick, one tick fewer
        px, am, sd = R.one_sided(n, sign)
        assert len(px) == n and am.dtype == np.float32 and sd.dtype == np.int8 and (sd == sign).all() and (am == 1.0).all()
        want = R.closes_one_sided(n, K)
        assert want.dtype == np.int64 and (want[-1] == n - 1) == (n == 3 * K or K == 1)
        for rule in R.RULES:
            for kind in ("tick", "volume"):
                assert np.array_equal(R.closes(rule, kind, px, am, sd, float(K)), want), (rule, kind, K, n)
    px, am, sd = R.one_sided(3 * K + 5, sign, lot=0.25)
    for rule in R.RULES:
        assert np.array_equal(R.closes(rule, "volume", px, am, sd, K * 0.25), R.closes_one_sided(3 * K + 5, K))


def test_biased_tapes():
    n = 16 * 4096 + 1
    for p_up in (0.5, 0.7, 1.0):
        px, am, sd = R.biased(n, 1, p_up, 0.1, 0.05)
        assert len(px) == n and am.dtype == np.float32 and sd.dtype == np.int8
        assert 0.08 < (sd == 0).mean() < 0.12 and 0.03 < (am == 0).mean() < 0.07
        up = (sd == 1).sum() / (sd != 0).sum()
        assert abs(up - p_up) < 0.01 and ((sd == -1).sum() == 0) == (p_up == 1.0)
        assert (am * 64 == np.round(am * 64)).all() and (px * 4 == np.round(px * 4)).all() and (px > 0).all()
        for rule in R.RULES:
            for kind, thr in (("volume", 8.0), ("tick", 16.0), ("dollar", 800.0)):
                assert R.certifies(rule, kind, px, am, sd, thr)
                assert len(R.closes(rule, kind, px, am, sd, thr)) > 100
    assert not np.array_equal(R.biased(n, 1, 0.7, 0.1, 0.05)[2], R.biased(n, 2, 0.7, 0.1, 0.05)[2])


@pytest.mark.parametrize("rule", ["imbalance", "run"])
def test_certificate_edge_tapes(rule):
    inside, outside = (R.certificate_edge(X) for X in R.CERT_EDGE_X)
    for px, am, sd in (inside, outside):
        assert len(px) == 1500 and am.dtype == np.float64 and np.flatnonzero(sd).tolist() == list(R.CERT_EDGE_AT)
        assert R.low_bit_exp(am) == -30
        assert R.closes(rule, "volume", px, am, sd, R.CERT_EDGE_THR).tolist() == list(R.CERT_EDGE_CLOSES)
    assert math.fsum(inside[1].tolist()) + R.CERT_EDGE_THR == 2.0 ** 23 - 2.0 ** -30
    assert math.fsum(outside[1].tolist()) + R.CERT_EDGE_THR == 2.0 ** 23
    assert R.certifies(rule, "volume", *inside, R.CERT_EDGE_THR) and not R.certifies(rule, "volume", *outside, R.CERT_EDGE_THR)


@pytest.mark.parametrize("rule", ["imbalance", "run"])
def test_a_threshold_between_two_quanta_rounds_up(rule):
    """Lots of k / 64: a sum reaches thr exactly when it reaches the next multiple of 1 / 64 (what fb_certificate's ceil relies on)."""
    n = 65537
    cols = R.recipe(n)
    at = {thr: R.closes(rule, "volume", *cols, thr) for thr in R.ROUNDING_THR}
    lo, eight, hi, above, lot, sub = (at[thr] for thr in R.ROUNDING_THR)
    assert np.array_equal(lo, eight) and np.array_equal(hi, above) and not np.array_equal(hi, eight)
    assert np.array_equal(lot, np.arange(n)) and np.array_equal(sub, np.arange(n))


def test_long_bars_with_live_flow():
    n = (1 << 20) + 1
    for i, (rule, thr, longest) in enumerate(R.LONG_BARS):
        w = R.closes(rule, "volume", *R.recipe(n), thr)
        assert np.diff(w).max() == longest
        if i == 0:
            assert longest > 65 * 512                               # more than one round of 64 block summaries


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

