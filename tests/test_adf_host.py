"""CPU-only checks of the ADF / SADF statistic: the longdouble restatement (tests/_adf_ref.py) against a plain least-squares ADF on
uncentred regressors, every argument rule on the host with no library loaded, the bookkeeping of min_ffd_d with a stubbed ADF, and
the tolerance the GPU tests use, measured here.  Also the home of the inputs tests/test_gpu_adf.py runs."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _adf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = tuple((lags, trend) for lags in range(5) for trend in ("c", "ct"))           # k = 2 .. 7, each reached both ways
FAMILIES = ("logwalk", "bubble", "level1e5")
MAX_LENS = (12, 63, 64, 65, 128, 129, 200)            # min_len itself, one step of the 64-row walk, its seams, carried sums


# ---------------------------------------------------------------------------------------------- the inputs of the GPU tests
@functools.lru_cache(maxsize=None)
def walk(family, n=400):
    rng = np.random.default_rng({"logwalk": 21, "bubble": 22, "level1e5": 23}[family] * 100003 + n)
    if family == "logwalk":                           # the logarithm of a price near 100 that moves by about 1 % a row
        y = np.log(100.0) + np.cumsum(0.01 * rng.standard_normal(n))
    elif family == "bubble":                          # the same with a drift that grows exponentially: explosive at the end
        y = np.log(100.0) + np.cumsum(0.01 * rng.standard_normal(n) + 2e-4 * np.exp(np.arange(n) * (4.0 / n)))
    else:                                             # a price level near 10^5 taken as given, steps of about 25
        y = 1e5 + np.cumsum(25.0 * rng.standard_normal(n))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def odd_tape():
    """A log walk (the seed is one at which no window enters the threshold bands) whose steps are zero over a stretch longer than
    max_len = 64 and over a shorter one, with an exactly geometric stretch (dy_i = 0.03 y_{i-1}: an exact fit for lags = 0,
    collinear columns with lags) after which the walk goes on from where the stretch ends, then NaN at the start, in the middle and
    at the end, +inf and -inf."""
    steps = 0.01 * np.random.default_rng(34).standard_normal(1500)
    steps[400:480] = 0.0
    steps[1100:1120] = 0.0
    y = np.log(100.0) + np.cumsum(steps)
    y[1350:1450] = y[1349] * 1.03 ** np.arange(1, 101)
    y[1450:] = y[1449] + np.cumsum(steps[1450:])
    y[0] = np.nan
    y[700] = np.nan
    y[1499] = np.nan
    y[300] = np.inf
    y[1000] = -np.inf
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def ramp_tape():
    """The log walk after an exact ramp longer than max_len = 64: its level is a multiple of the trend and its differences are
    constant, so a window inside it is degenerate under "ct" and with lags.  (A window whose targets are all equal while a regressor
    is not -- a ramp with lags = 0 and "c", or rows whose lagged differences reach back before a ramp -- is an exact fit whose level
    coefficient is zero up to rounding: the sign of that infinity is rounding's.  So the ramp opens the tape, and lags = 0 with "c"
    is not asked of it.)"""
    y = walk("logwalk", 400).copy()
    y[:100] = 4.5 + 0.0078125 * np.arange(100)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def end_points(count, n=3001):
    """`count` end points with duplicates, in no order; the last element and element 0 among them when there is room."""
    ev = np.random.default_rng(count).integers(0, n, count).astype(np.int64)
    if count >= 3:
        ev[0], ev[1], ev[2] = n - 1, 0, n - 1
    ev.setflags(write=False)
    return ev


END_COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 500)         # the batch of 8, the 64 lanes, and more than one claim


def all_inputs():
    """(name, y, end_idxs or None, min_len, max_len, step, lags, trend) of every call the GPU tests compare with the reference."""
    for c, (lags, trend) in enumerate(CONFIGS):       # every k over both trends at min_len = k + 1: one degree of freedom
        k = R.regressors(lags, trend)                 # (150 or 151 elements: the first length at which no window enters a band)
        n = 151 if (lags, trend) in ((1, "c"), (4, "c")) else 150
        yield f"k/{lags}{trend}", walk(FAMILIES[c % 3], n), None, k + 1, 65, 1, lags, trend
    for fam in FAMILIES:
        for ml in MAX_LENS:
            yield f"len/{fam}/{ml}", walk(fam), None, 12, ml, 1, 1, "c"
    for ml in (64, 65, 129):
        yield f"len/ct/{ml}", walk("bubble"), None, 12, ml, 1, 4, "ct"
    for step in (3, 64):
        yield f"step/{step}/1c", walk("logwalk"), None, 12, 200, step, 1, "c"
        yield f"step/{step}/2ct", walk("level1e5"), None, 12, 200, step, 2, "ct"
    yield "all_history", walk("bubble"), None, 12, 400, 1, 1, "c"
    for n in (1, 4, 5, 12 + 1, 12 + 1 + 1):           # n = 1, n = k + 1, n = min_len + L (one row short) and the first that fits
        yield f"tiny/{n}", walk("logwalk")[:n], None, 4 if n < 6 else 12, 12, 1, 1, "c"
    for lags, trend in ((0, "c"), (1, "c"), (0, "ct"), (4, "ct")):
        yield f"odd/{lags}{trend}", odd_tape(), None, 12, 64, 1, lags, trend
    for lags, trend in ((1, "c"), (0, "ct"), (4, "ct")):
        yield f"ramp/{lags}{trend}", ramp_tape(), None, 12, 64, 1, lags, trend
    for count in END_COUNTS:
        yield f"ends/{count}", walk("logwalk", 3001), end_points(count), 12, 65, 1, 1, "c"
    yield "long", walk("logwalk", 3001), None, 12, 129, 1, 1, "c"


@functools.lru_cache(maxsize=None)
def input_of(name):
    for item in all_inputs():
        if item[0] == name:
            return item[1:]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The longdouble reference of one input, computed once and shared."""
    return R.sadf(*input_of(name))


# The tolerance of a finite statistic on the GPU, relative to max(1, |stat|).  E is the largest error of the float64 restatement (the
# same recurrence with left-to-right sums) against the longdouble reference over EVERY window of every input of all_inputs(),
# measured on the CPU by test_recorded_tolerance_is_the_measured_one, which fails when a constant no longer covers its measurement:
#   E_WALK  the three walks in every shape, the tiny series, the end-point lists and the long walk: 2.2e-12 over 1.1 million finite
#           statistics;
#   E_DOF1  every k at min_len = k + 1: 2.9e-8 over 68 000.  With one degree of freedom SSR / sum dy^2 comes as close to the
#           exact-fit band as 1.4e-6, and the cancellation in SSR multiplies the rounding of the moments by its reciprocal;
#   E_ODD   the tapes with NaN, infinities, constant and geometric stretches and the ramp: 1.9e-9 over 300 000.  A window that is
#           constant or geometric but for a few rows is ill-conditioned (relative pivots down to 1.3e-6, still 1.4 times above the
#           band that no input may enter), which multiplies the rounding of its moments.
# The two ill-conditioned groups keep constants of their own so that they do not widen the bound of every other input.
# The GPU is allowed FACTOR * E: it sums 64-row blocks plus a carry where the restatement sums left to right, and 4 covers another
# association of the same sums without hiding a wrong formula.
E_WALK = 2.5e-12
E_DOF1 = 3.0e-8
E_ODD = 2.0e-9
FACTOR = 4.0


def group(name):
    return {"odd": "odd", "ramp": "odd", "k": "dof1"}.get(name.split("/")[0], "walk")


def tolerance(name):
    """The GPU tolerance of the input `name`: the ill-conditioned groups have their own (larger) measured error, so that they do not
    widen the bound of every other input."""
    return FACTOR * {"walk": E_WALK, "dof1": E_DOF1, "odd": E_ODD}[group(name)]


def close_end_points(ref, tol):
    """End points whose best and runner-up statistics are finite and lie within 2 * tol (relative to max(1, |best|)) -> bool per end
    point: there the device may take any start whose reference statistic lies in that band."""
    with np.errstate(invalid="ignore"):
        best, second = ref["stat"], ref["runner_up"]
        return np.isfinite(best) & np.isfinite(second) & (best - second <= 2 * tol * np.maximum(1, np.abs(best)))


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_centring_changes_nothing():
    """A handful of windows of each family against numpy.linalg.lstsq on UNCENTRED regressors (y_{i-1} itself, the trend as i): the
    statistic is the same up to what least squares on uncentred columns loses (most on the level-10^5 walk)."""
    for fam, bound in (("logwalk", 1e-8), ("bubble", 1e-8), ("level1e5", 1e-6)):
        y = walk(fam)
        for lags, trend in ((0, "c"), (1, "c"), (4, "ct")):
            ref = R.sadf(y, [60, 200, 399], 12, 40, 7, lags, trend)
            for e, t in enumerate(ref["end"]):
                for c, m in enumerate(ref["lengths"]):
                    want = R.lstsq_adf(y, t - m + 1, t, lags, trend)
                    assert abs(float(ref["table"][e, c]) - want) <= bound * max(1, abs(want)), (fam, lags, trend, t, m)


def test_by_hand():
    """lags = 0, "c", y = 0, 1, 3, 2, 2 at t = 4 over the rows i = 2, 3, 4: dy = 2, -1, 0 on the levels
    y_{i-1} - y_4 = -1, 1, 0.  Level mean 0, dy mean 1/3: beta = sum(level * dy) / sum(level^2) = -3/2; residuals dy - 1/3 - beta *
    level = 1/6, 1/6, -1/3: SSR = 1/6, sigma^2 = SSR / (3 - 2), se = sqrt(1/6 / 2): ADF = -1.5 / sqrt(1/12) = -3 sqrt(3)."""
    r = R.sadf(np.array([0.0, 1.0, 3.0, 2.0, 2.0]), [4], 3, 3, 1, 0, "c")
    assert abs(float(r["stat"][0]) + 3 * np.sqrt(3)) < 1e-15 and r["start"][0] == 2 and r["n_skipped"] == 0
    r = R.sadf(np.array([0.0, 1.0, 3.0, 2.0, 2.0]), None, 3, 4, 1, 0, "c")
    assert list(r["start"][:3]) == [-1, -1, -1] and r["start"][3] == 1 and r["start"][4] in (1, 2)
    assert np.isnan(r["stat"][:3]).all() and np.isfinite(r["stat"][3:]).all() and r["n_skipped"] == 3


def test_special_cases_of_the_definition():
    const = R.sadf(np.full(40, 4.6), None, 4, 20, 1, 1, "c")
    assert np.isnan(const["stat"]).all() and (const["start"] == -1).all() and const["n_skipped"] == 40
    geo = R.sadf(100.0 * 1.03 ** np.arange(40), [39], 4, 20, 1, 0, "c")
    assert np.isposinf(geo["stat"][0]) and geo["start"][0] == 36                     # the shortest window among the +inf
    decay = R.sadf(100.0 * 0.97 ** np.arange(40), [39], 4, 20, 1, 0, "ct")
    assert np.isneginf(decay["stat"][0]) and decay["start"][0] == 36
    ramp = R.sadf(4.5 + 0.0078125 * np.arange(40), None, 5, 20, 1, 1, "ct")
    assert np.isnan(ramp["stat"]).all() and np.isnan(R.sadf(4.5 + 0.0078125 * np.arange(40), None, 4, 20, 1, 1, "c")["stat"]).all()
    y = walk("logwalk", 300).copy()
    y[100] = np.inf
    hole = R.sadf(y, None, 12, 30, 1, 1, "c")
    # a window reads y[s - lags - 1 .. t]: with the hole at 100 the end points 100 .. 113 have no window of 12 rows left
    assert np.isnan(hole["stat"][100:114]).all() and np.isfinite(hole["stat"][114:]).all() and np.isfinite(hole["stat"][14:100]).all()
    assert (hole["start"][114:131] >= 103).all()                                    # no window reaches back to the hole


# ---------------------------------------------------------------------------------------------- argument rules
def test_every_argument_error_is_raised_with_no_library_loaded():
    code = r"""
import numpy as np, pytest
from finmlkit_amd import _ffi
from finmlkit_amd.feature.core import structural_break as P
from finmlkit_amd.feature.core.structural_break import adf
from finmlkit_amd.feature import transforms as T
y = np.linspace(4.0, 5.0, 50)
for kw, msg in ((dict(lags=5), adf.LAGS_MESSAGE), (dict(lags=-1), adf.LAGS_MESSAGE), (dict(trend="nc"), adf.TREND_MESSAGE),
                (dict(trend=1), adf.TREND_MESSAGE), (dict(min_len=3), "min_len must be at least 4"),
                (dict(min_len=4, trend="ct"), "min_len must be at least 5"), (dict(min_len=7, lags=4, trend="ct"), "at least 8"),
                (dict(max_len=11), adf.MAX_LEN_MESSAGE), (dict(step=0), adf.STEP_MESSAGE), (dict(min_len=12.5), adf.INTEGER_MESSAGE),
                (dict(end_idxs=np.array([0, 50])), "1 end points outside [0, 50)"),
                (dict(end_idxs=np.array([-1, 3, 77])), "2 end points outside [0, 50)"),
                (dict(end_idxs=np.array([0.5])), adf.END_IDXS_MESSAGE),
                (dict(lags=9, trend="x", min_len=0, step=0), adf.LAGS_MESSAGE)):                   # the library's order
    args = dict(y=y, min_len=12, max_len=None, lags=1, trend="c", step=1, end_idxs=None)
    args.update(kw)
    with pytest.raises(ValueError) as ei:
        P.sadf(**args)
    assert msg in str(ei.value), (msg, str(ei.value))
with pytest.raises(ValueError, match="min_len must be at least 4"):
    P.adf_rolling(y, 3)
with pytest.raises(ValueError, match="min_len must be at least 4"):
    P.adf_stat(y[:5])                                         # 5 elements are 3 rows
with pytest.raises(ValueError, match="lags must be between"):
    T.SADF(12, 64, lags=7)
assert adf.check_arguments(50, None, 12, None, 1, "c", 1) == (12, 50, 1, 0, 1)
assert adf.check_arguments(5, None, np.int64(12), None, 4, "ct", 3) == (12, 12, 4, 1, 3)
stat, start = P.sadf(y, 12, end_idxs=np.zeros(0, np.int64))      # no end point, and an empty series: answered on the host
assert stat.shape == start.shape == (0,) and stat.dtype == np.float64 and start.dtype == np.int64
assert [len(o) for o in P.sadf(y[:0], 12)] == [0, 0] and len(P.adf_rolling(y[:0], 12)) == 0
assert T.SADF(12, 64).output_name == "close_sadf_12_64" and T.SADF(12, input_col="x").output_name == "x_sadf_12_all"
assert _ffi._lib is None and _ffi._default_ctx is None
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_header_declares_and_library_exports_the_entry_points():
    from finmlkit_amd import _ffi
    from finmlkit_amd.feature import core
    from finmlkit_amd.feature.core import structural_break as P
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmk.h")).read(), flags=re.S)
    for s in ("fmk_sadf_dev", "fmk_sadf"):
        assert re.search(r"\b%s\s*\(" % s, txt) and hasattr(_ffi.lib(), s), s
    assert "fmk_sadf.hip" in open(os.path.join(ROOT, "finmlkit_amd", "csrc", "Makefile")).read()
    assert {"sadf", "adf_rolling", "adf_stat"} <= set(P.__all__) and "min_ffd_d" in core.__all__


def test_no_cpu_fallback():
    from finmlkit_amd import _ffi
    from finmlkit_amd.feature.core import structural_break as P
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_ffi.FmkError):
        P.sadf(np.linspace(4.0, 5.0, 50), 12)


# ---------------------------------------------------------------------------------------------- min_ffd_d's bookkeeping
def test_min_ffd_d_picks_the_first_d_below_crit(monkeypatch):
    from finmlkit_amd.feature.core import fracdiff as P
    calls = []

    def stub(x, ds, threshold, lags):
        calls.append((len(x), tuple(ds), threshold, lags))
        return np.array([-1.0, np.nan, -2.9, -2.5, -3.5])[:len(ds)]
    monkeypatch.setattr(P, "ffd_adf_stats", stub)
    ds = [0.0, 0.2, 0.4, 0.6, 0.8]
    d, stats = P.min_ffd_d(np.arange(10.0), ds)
    assert d == 0.4 and np.array_equal(stats, [-1.0, np.nan, -2.9, -2.5, -3.5], equal_nan=True)
    assert calls == [(10, tuple(ds), 1e-5, 1)] and P.ADF_CRIT_95 == -2.8623
    assert P.min_ffd_d(np.arange(10.0), ds, crit=-3.0)[0] == 0.8                  # the first below, not the lowest
    assert P.min_ffd_d(np.arange(10.0), ds, crit=-2.9)[0] == 0.8                  # strictly below
    assert P.min_ffd_d(np.arange(10.0), ds, crit=-4.0)[0] is None                 # NaN never passes, and nothing else does
    assert P.min_ffd_d(np.arange(10.0), ds[:2], threshold=1e-3, lags=2)[0] is None and calls[-1][2:] == (1e-3, 2)
    assert len(P.min_ffd_d(np.arange(10.0))[1]) == 5 and len(calls[-1][1]) == 11 and calls[-1][1][1] == 0.1


def test_ffd_adf_stats_needs_no_device_for_a_series_too_short():
    """Every d leaves fewer rows than one degree of freedom: NaN everywhere, answered on the host (this machine has no device)."""
    from finmlkit_amd.feature.core import fracdiff as P
    stats = P.ffd_adf_stats(np.linspace(4.0, 5.0, 5), [0.0, 0.5, 1.0], 1e-2, 1)
    assert stats.shape == (3,) and np.isnan(stats).all()
    with pytest.raises(ValueError, match="lags must be between"):
        P.ffd_adf_stats(np.linspace(4.0, 5.0, 50), [0.5], 1e-2, 5)


# ---------------------------------------------------------------------------------------------- the conditions of the comparison
def test_inputs_are_what_the_issue_asks_for():
    names = [item[0] for item in all_inputs()]
    assert len(names) == len(set(names))
    assert {R.regressors(l, t) for l, t in CONFIGS} == set(range(2, 8)) and len(CONFIGS) == 10
    assert all(input_of(f"k/{l}{t}")[2] == R.regressors(l, t) + 1 for l, t in CONFIGS)
    assert set(MAX_LENS) == {12, 63, 64, 65, 128, 129, 200}
    y = odd_tape()
    assert np.isnan(y[[0, 700, 1499]]).all() and np.isposinf(y[300]) and np.isneginf(y[1000])
    assert len(set(y[400:480])) == 1 and len(set(y[1100:1120])) == 1
    for count in END_COUNTS:
        ev = end_points(count)
        assert len(ev) == count and (count < 3 or (len(np.unique(ev)) < count and np.any(np.diff(ev) < 0)))
    assert max(len(item[1]) for item in all_inputs()) <= 4000


def test_no_input_sits_on_a_threshold_and_close_end_points_are_few():
    """On the reference alone: every window of every input has its relative pivots above 2^-20 or one below 2^-32, and its
    SSR / sum dy^2 likewise; end points whose best and runner-up lie within twice the tolerance are at most 2 % of an input."""
    shares, smallest = {}, {"pivot": np.inf, "fit": np.inf, "gap": np.inf}
    for name, *_ in all_inputs():
        ref = reference(name)
        assert ref["band"].sum() == 0, (name, np.flatnonzero(ref["band"])[:5])
        close = close_end_points(ref, tolerance(name))
        assert close.sum() * 50 <= max(len(close), 1), (name, int(close.sum()), len(close))
        if close.any():
            shares[name] = (int(close.sum()), len(close))
        if len(close):
            smallest["pivot"] = min(smallest["pivot"], ref["min_pivot"].min())
            smallest["fit"] = min(smallest["fit"], ref["min_fit"].min())
            with np.errstate(invalid="ignore"):
                gap = ((ref["stat"] - ref["runner_up"]) / np.maximum(1, np.abs(ref["stat"])))[np.isfinite(ref["runner_up"]) &
                                                                                            np.isfinite(ref["stat"])]
            if len(gap):
                smallest["gap"] = min(smallest["gap"], float(gap.min()))
    print("close end points:", shares, "smallest above the bands:", smallest)
    assert smallest["pivot"] > R.BAND_HIGH and smallest["fit"] > R.BAND_HIGH


def test_special_values_of_the_hand_built_inputs():
    """The hand-built stretches decide what the comments say they decide."""
    ref = reference("odd/0c")
    assert np.isposinf(ref["stat"][1365:1450]).all()                               # windows inside the geometric stretch: exact fit
    assert (ref["start"][1365:1450] == np.arange(1365, 1450) - 11).all()           # the shortest window among the +inf
    assert np.isnan(ref["stat"][463:480]).all() and (ref["start"][463:480] == -1).all()         # y[t-64 .. t] is constant
    assert np.isfinite(ref["stat"][1119]) and ref["start"][1119] < 1100            # the short stretch: longer windows see past it
    assert np.isnan(ref["stat"][[0, 300, 700, 1000, 1499]]).all() and ref["n_skipped"] > 50
    for cfg in ("1c", "0ct", "4ct"):
        r = reference(f"ramp/{cfg}")
        assert np.isnan(r["stat"][:100]).all(), cfg                                # windows inside the ramp are degenerate
        assert np.isfinite(r["stat"][200:]).all()
    assert np.isnan(reference("odd/1c")["stat"][1414:1450]).all()                   # y[t-65 .. t] geometric, a lag: collinear columns
    for n in (1, 4, 5, 13):
        assert np.isnan(reference(f"tiny/{n}")["stat"]).all()
    assert np.isfinite(reference("tiny/14")["stat"][13]) and reference("tiny/14")["n_skipped"] == 13


def test_recorded_tolerance_is_the_measured_one():
    """Re-measures E on every input: the recorded constant covers the measurement and exceeds it by no more than a factor 2.5 (it is
    the measurement rounded up); the float64 restatement moves a start only at close end points."""
    worst, compared, per = dict.fromkeys(("walk", "dof1", "odd"), 0.0), dict.fromkeys(("walk", "dof1", "odd"), 0), {}
    for name, *args in all_inputs():
        ref = reference(name)
        err, cnt, moved = R.relative_error(*args, ref=ref)
        if moved:
            got = R.sadf(*args, dtype=np.float64)
            assert np.all(close_end_points(ref, tolerance(name))[ref["start"] != got["start"]]), name
        per[name.split("/")[0]] = max(per.get(name.split("/")[0], 0.0), err)
        worst[group(name)] = max(worst[group(name)], err)
        compared[group(name)] += cnt
    print("measured E:", worst, "over", compared, "finite statistics;", per)
    assert min(compared.values()) > 50000
    for key, recorded in (("walk", E_WALK), ("dof1", E_DOF1), ("odd", E_ODD)):
        assert worst[key] <= recorded <= 2.5 * worst[key], key
