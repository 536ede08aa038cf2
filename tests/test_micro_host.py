"""CPU-only checks of the per-bar microstructure features: the definition (tests/_micro_ref.py) on hand-built bars
with known answers, the conditions on the reference alone that the GPU comparison leans on, the t-value tolerance measured from the
float64 restatement, the refusals of the Python layer and the host check program of csrc/fmk_micro_rule.h.  The inputs are recorded
here as functions; tests/test_gpu_micro.py imports them."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _micro_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("f32", "f64")
N_TICKS = 180_000

# tolerance(name): 4 x the largest relative error of a finite nonzero t-value of the float64 left-to-right restatement against the
# longdouble reference on tape(name) with closes(name) -- the margin of tests/test_gpu_trend.py, for the same reason: the kernel adds
# the same float64 terms in another order.  test_t_tolerance_is_four_times_the_measured_error keeps the constants honest.
T_TOL = {"f32": 7.6e-13, "f64": 1.4e-13}       # measured: 1.894e-13 and 3.474e-14


# ---------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def tape(name, n=N_TICKS):
    """A walk on a 0.01 price grid whose steps lean with the signed size (trades move the price), lognormal sizes (float32 or
    float64), sides +-1 with a few 0 -> (price f64, amount, side i8), read-only."""
    rng = np.random.default_rng({"f32": 1905, "f64": 1906}[name])
    sd = rng.choice(np.array([-1, 1], np.int8), n)
    sd[rng.random(n) < 0.04] = 0
    v = np.exp(0.9 * rng.standard_normal(n) - 0.5)
    step = np.rint(0.8 * sd * np.minimum(v, 3.0) + 2.5 * rng.standard_normal(n))
    p = np.round((20_000 + np.cumsum(step)) * 0.01, 2)
    assert p.min() > 50.0
    v = v.astype(np.float32) if name == "f32" else v
    for a in (p, v, sd):
        a.setflags(write=False)
    return p, v, sd


def lengths_to_closes(lengths, first=-1):
    return np.concatenate([[first], first + np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def closes(name, n=N_TICKS):
    """Close indices over tape(name): mostly bars of 3 .. 40 ticks, some of 33 .. 400, a few of 400 .. 3 000, now and then an
    empty, a one-tick or a two-tick bar; the first bar opens at tick 0."""
    rng = np.random.default_rng({"f32": 77, "f64": 78}[name])
    out, used = [], 0
    while True:
        c = rng.random()
        L = int(rng.integers(0, 3) if c < 0.03 else rng.integers(3, 41) if c < 0.75 else rng.integers(33, 401) if c < 0.97
                else rng.integers(400, 3001))
        if used + L > n:
            break
        out.append(L)
        used += L
    ci = lengths_to_closes(out)
    ci.setflags(write=False)
    return ci


@functools.lru_cache(maxsize=None)
def reference(name):
    return R.reference(*tape(name), closes(name))


def hand_bars(L):
    """Bars of L ticks with known answers -> [(label, price, amount f64, side i8, check(row))]; row: {column: float}.  Every value is
    dyadic where exactness is claimed."""
    k = np.arange(L)
    sd_mix = np.where(k % 5 == 0, -1, 1).astype(np.int8)
    v_mix = 1.0 + (k % 3)
    out = []
    for c in (0.25, -0.5):
        v = np.array([1.0, 2.0, 0.5, 4.0, 1.5, 3.0, 2.5, 0.75])[k % 8]
        sd = np.where((k * 7 // 3) % 2 == 0, 1, -1).astype(np.int8)
        p = 1024.0 + np.concatenate([[0.0], np.cumsum(c * sd[1:] * v[1:])])

        def chk(row, c=c):
            assert row["kyle_lambda"] == c and row["kyle_t"] == math_copysign_inf(c), row
        out.append((f"kyle c={c}", p, v, sd, chk))

    def chk_alt(row):
        assert row["serial_cov"] == -1.0 and row["roll_spread"] == 2.0, row
    out.append(("alternating", 100.0 + (k & 1), v_mix, sd_mix, chk_alt))

    def chk_ramp(row):
        assert row["serial_cov"] > 0 and row["roll_spread"] == 0.0 and not np.signbit(row["roll_spread"]), row
    out.append(("ramp", 100.0 + 0.5 * k, v_mix, sd_mix, chk_ramp))

    def chk_flat(row):
        for c in R.COLS:
            assert row[c] == 0.0 and not np.signbit(row[c]), (c, row)
    out.append(("flat", np.full(L, 250.0), v_mix, np.where(k & 1, 1, -1).astype(np.int8), chk_flat))

    def chk_side0(row):
        assert all(np.isnan(row[c]) for c in ("kyle_lambda", "kyle_t", "hasbrouck_lambda", "hasbrouck_t")), row
        assert np.isfinite(row["amihud_lambda"]) and np.isfinite(row["amihud_t"]) and np.isfinite(row["serial_cov"]), row
    p0 = tape("f64")[0][1000:1000 + L]
    out.append(("side 0", p0, tape("f64")[1][1000:1000 + L], np.zeros(L, np.int8), chk_side0))
    return out


def math_copysign_inf(c):
    return float("inf") if c > 0 else float("-inf")


def rows(res, nb=None):
    """{column: array} or the 8-tuple -> one {column: float} per bar"""
    if not isinstance(res, dict):
        res = dict(zip(R.COLS, res))
    nb = len(res[R.COLS[0]]) if nb is None else nb
    return [{c: float(res[c][b]) for c in R.COLS} for b in range(nb)]


HAND_LENGTHS = (12, 40, 200)


# ---------------------------------------------------------------------------------------------- the definition on hand-built bars
@pytest.mark.parametrize("L", HAND_LENGTHS)
def test_hand_built_bars_have_their_known_answers(L):
    for label, p, v, sd, chk in hand_bars(L):
        ci = np.array([-1, L - 1])
        for ev in (R.reference, R.restatement):
            res = ev(p, v, sd, ci)
            chk(rows(res, 1)[0])
        ref = R.reference(p, v, sd, ci)
        if label.startswith("kyle"):
            assert ref["aux"]["kyle"]["rule"][0] == 3 and ref["aux"]["kyle"]["u"][0] == 0
        if label == "flat":
            assert all(ref["aux"][g]["rule"][0] == 2 for g in R.REGS)
        if label == "side 0":
            assert ref["aux"]["kyle"]["rule"][0] == 1 and ref["aux"]["hasbrouck"]["rule"][0] == 1 and ref["aux"]["amihud"]["rule"][0] == 4


def test_short_bars_are_nan_rows_and_a_bar_reads_nothing_outside_itself():
    p, v, sd = tape("f64")
    ci = np.array([9, 9, 10, 12, 15, 40])                     # 0, 1, 2, 3, 25 ticks
    res = R.reference(p, v, sd, ci)
    for b in range(3):
        assert all(np.isnan(res[c][b]) for c in R.COLS)
    assert not np.isnan(res["serial_cov"][3]) and res["aux"]["m"].tolist() == [-1, 0, 1, 2, 24]
    # the tick in front of a bar is not part of it
    p2 = p.copy()
    p2[15] = np.nan
    res2 = R.reference(p2, v, sd, ci)
    assert all(R.same_bits(res2[c][4:].astype(np.float64), res[c][4:].astype(np.float64)) for c in R.COLS)
    assert np.isnan(res2["kyle_lambda"][3])


# ---------------------------------------------------------------------------------------------- conditions on the reference alone
@pytest.mark.parametrize("name", FAMILIES)
def test_reference_conditions(name):
    ref = reference(name)
    nb = len(ref["aux"]["m"])
    assert nb > 1000 and ref["aux"]["m"].max() > 2000 and (ref["aux"]["m"] < 2).sum() > 10
    for g in R.REGS:
        u = ref["aux"][g]["u"]
        assert not np.any((u > 0) & (u < 2.0 ** -20)), (g, "a bar inside the band around the exact-fit switch")
        assert (ref["aux"][g]["rule"] == 4).sum() > 0.9 * nb
    gam, bound = ref["serial_cov"], R.gamma_bound(ref)
    f = ~np.isnan(gam)
    share = float(np.mean(np.abs(gam[f]) < bound[f]))
    print(f"{name}: bars {nb}, share of |serial_cov| below its tolerance {share:.4f}")
    assert share < 0.02


# ---------------------------------------------------------------------------------------------- the tolerance and the bounds
@pytest.mark.parametrize("name", FAMILIES)
def test_t_tolerance_is_four_times_the_measured_error(name):
    err = float(R.t_errors(R.restatement(*tape(name), closes(name)), reference(name)).max())
    print(f"{name}: largest relative t-value error of the float64 restatement {err:.3e}, tolerance {T_TOL[name]:.3e}")
    assert 4 * err <= T_TOL[name] <= 8 * err


@pytest.mark.parametrize("name", FAMILIES)
def test_restatement_stays_inside_every_bound(name):
    R.assert_equal(R.restatement(*tape(name), closes(name)), reference(name), T_TOL[name], name)


# ---------------------------------------------------------------------------------------------- the Python layer's refusals
def test_python_layer_refuses_before_any_device_call():
    code = r"""
import numpy as np, pytest
from finmlkit_amd import _ffi
from finmlkit_amd.bar.base import comp_bar_microstructure_features as f
from finmlkit_amd.engine import DeviceTrades
p, v, sd = np.ones(6), np.ones(6, np.float32), np.ones(6, np.int8)
with pytest.raises(IndexError, match="out of bounds"):
    f(p, v, np.array([-1, 3, 6]), sd)
with pytest.raises(IndexError, match="out of bounds"):
    f(p, v, np.array([-2, 3, 5]), sd)
with pytest.raises(ValueError, match="same length"):
    f(p, v[:5], np.array([-1, 3, 5]), sd)
with pytest.raises(ValueError, match="same length"):
    f(p, v, np.array([-1, 3, 5]), sd[:2])
with pytest.raises(ValueError, match="negative dimensions"):
    f(p, v, np.array([], np.int64), sd)
class Cols:
    n = 6
    p = None
with pytest.raises(ValueError, match="side column"):
    DeviceTrades(None, Cols, Cols, v, None).bar_microstructure(Cols)
assert _ffi._lib is None and _ffi._default_ctx is None
assert [k for k, _ in _ffi.MICROSTRUCTURE_FIELDS] == ["kyle_lambda", "kyle_t", "amihud_lambda", "amihud_t", "hasbrouck_lambda",
                                                      "hasbrouck_t", "serial_cov", "roll_spread"]
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_kits_refuse_without_a_side_column():
    import pandas as pd
    from finmlkit_amd.bar.base import BarBuilderBase

    class Kit(BarBuilderBase):
        def __init__(self, df):
            self.trades_df, self._close_ts, self._close_indices = df, np.array([0, 1]), np.array([-1, 1])
            self._d_close_idx = object()

        def _comp_bar_close(self):
            raise AssertionError

    with pytest.raises(KeyError, match="side"):
        Kit(pd.DataFrame({"timestamp": [0, 1], "price": [1.0, 2.0], "amount": [1.0, 1.0]})).build_microstructure_features()


def test_header_declares_and_library_exports_the_entry_points():
    from finmlkit_amd import _ffi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmk.h")).read(), flags=re.S)
    for s in ("fmk_comp_bar_microstructure", "fmk_comp_bar_microstructure_dev"):
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(_ffi.lib(), s), s
    assert "fmk_micro.hip" in open(os.path.join(ROOT, "finmlkit_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------------------------------------- the header on the host
def test_rule_header_on_the_host(tmp_path):
    """tools/micro_check.cpp, built from csrc/fmk_micro_rule.h with the host compiler alone (no HIP), in its quick form: the terms,
    every branch of the rules and random bars against a long double evaluation.  (The full run under ASan / UBSan is a tool run, not
    part of the suite.)"""
    exe = str(tmp_path / "micro_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tools", "micro_check.cpp"),
                           "-o", exe])
    r = subprocess.run([exe, "quick"], capture_output=True, text=True)
    assert r.returncode == 0 and "failed checks 0" in r.stdout, r.stdout
    assert int(re.search(r"bars (\d+)", r.stdout).group(1)) > 4000
    assert all(int(x) > 0 for x in re.search(r"branches (\d+) (\d+) (\d+) (\d+) (\d+)", r.stdout).groups())
