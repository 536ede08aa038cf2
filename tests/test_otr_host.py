"""CPU-only: the optimal-trading-rule mesh (finmlkit_amd/label/otr.py) without a device.  The generator of the
reference (tests/_otr_ref.py) against the normal distribution, the untouched node against the closed forms of the O-U process, the
rule header on the host (tools/otr_check.cpp: the record walk against the book's loop, and its mesh against the reference's, bit for
bit), ou_fit, the mesh object, everything the Python layer refuses, and that the cases tests/test_gpu_otr.py and
tests/test_gpu_otr_edges.py run hold what they are there for."""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

from finmlkit_amd import label
from finmlkit_amd.label import otr as P
from tests import _otr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
PHI5 = 2.0 ** (-1.0 / 5.0)
MESH4 = np.array([0.5, 1.0, 1.5, 2.0])
FIELDS = ("mean", "std", "sharpe", "n_profit", "n_stop", "n_time", "hold")
GEO = P.geometry()
B, TILE = GEO["block"], GEO["tile"]


# ---------------------------------------------------------------------------------------------- the cases of the GPU tests
def seam_case(n_paths, max_hp=24):
    """Two parameter sets (mean reverting towards a forecast, and a random walk) on a 4 x 4 mesh; the seed is the path count."""
    return dict(forecast=[0.5, 0.0], phi=[PHI5, 1.0], sigma=[1.0, 0.75], pt=MESH4, sl=MESH4, max_hp=max_hp, n_paths=n_paths, seed=n_paths)


PATH_SEAMS = (1, 63, 64, 65, TILE - 1, TILE + 1, B - 1, B, B + 1, 2 * B + TILE + 3)
STEP_SEAMS = (1, 2, 3, 24, 25)


def mesh_levels(n, kind):
    """n levels: "plain" 0.25 apart from 0.25; "edges" with pt[0] = 0, a repeated level and +inf last (where n allows)."""
    v = 0.25 * np.arange(1, n + 1)
    if kind == "edges":
        v[0] = 0.0
        if n >= 3:
            v[2] = v[1]
        if n >= 2:
            v[-1] = INF
    return v


MESH_SHAPES = {"1x1": (1, 1), "1x32": (1, 32), "32x1": (32, 1), "32x32": (32, 32), "21x21": (21, 21)}


def mesh_case(name, kind):
    n_pt, n_sl = MESH_SHAPES[name]
    if name == "21x21" and kind == "plain":
        pt = sl = np.linspace(0.0, 10.0, 21)                         # the book's mesh
    else:
        pt, sl = mesh_levels(n_pt, kind), mesh_levels(n_sl, kind)
    return dict(forecast=[0.5], phi=[PHI5], sigma=[2.0], pt=pt, sl=sl, max_hp=24, n_paths=TILE + 1, seed=13)


ULP = 2.0 ** -52
STEER_PT, STEER_SL = np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0])
STEER_ROWS = np.array([
    [1.0, 0.0, 0.0, 0.0],            # 0: on pt[0] from step 1: not passed, every node a time exit at 1.0
    [1.0 + ULP, 0.0, 0.0, 0.0],      # 1: one ulp above pt[0]: passed at step 1
    [0.0, 0.0, 0.0, 1.5],            # 2: passes pt[0] at h = max_hp: the barrier's
    [2.5, 0.0, 0.0, 0.0],            # 3: pt[0] and pt[1] in one step
    [3.5, 0.0, 0.0, 0.0],            # 4: all pt levels at step 1: the walk stops
    [-1.0, 0.0, 0.0, 0.0],           # 5: on -sl[0]: not passed
    [-1.0 - ULP, 0.0, 0.0, 0.0],     # 6: one ulp below -sl[0]
    [0.5, -3.0, 0.0, 0.0],           # 7: both sl levels at step 2: the walk stops
    [0.5, 0.5, 0.5, 0.5],            # 8: passes pt[0] at step 3 and ends on pt[1]
])


def steer_case():
    z = np.tile(STEER_ROWS, (8, 1))                                  # 72 paths: more than one tile
    return dict(forecast=[0.0], phi=[1.0], sigma=[1.0], pt=STEER_PT, sl=STEER_SL, max_hp=4, n_paths=len(z), seed=0), z


def no_noise_case():
    """sigma = 0: a constant path that sits on the zero levels, and drifts that pass levels at the same step on every path."""
    return dict(forecast=[0.0, 2.0, -2.0], phi=[0.5, 0.5, 0.5], sigma=[0.0, 0.0, 0.0], pt=np.array([0.0, 1.0, 1.5]),
                sl=np.array([0.0, 1.0, 1.5]), max_hp=6, n_paths=TILE + 5, seed=3)


BOOK_FORECASTS, BOOK_HALF_LIVES = (10.0, 5.0, 0.0, -5.0, -10.0), (5.0, 10.0, 25.0, 50.0, 100.0)


def book_case():
    f = [x for x in BOOK_FORECASTS for _ in BOOK_HALF_LIVES]
    hl = [h for _ in BOOK_FORECASTS for h in BOOK_HALF_LIVES]
    lv = np.linspace(0.5, 10.0, 7)
    phi = 2.0 ** (-1.0 / np.asarray(hl, dtype=np.float64))
    return dict(forecast=f, half_life=hl, phi=list(phi), sigma=[1.0] * 25, pt=lv, sl=lv, max_hp=20, n_paths=B + 1, seed=1313)


def reference(case, z=None):
    return R.mesh(case["forecast"], case["phi"], case["sigma"], case["pt"], case["sl"], case["max_hp"], case["n_paths"], case["seed"], B, z)


# ---------------------------------------------------------------------------------------------- the cases of tests/test_gpu_otr_edges.py
NPL_STEPS = (1, 4, 8)              # csrc/fmk_otr.hip: ceil(nodes / tile) <= 1, <= 4, <= 8 pick k_otr_walk<1>, <4>, <8>, more <NPL_MAX>
NPL_MAX = GEO["max_levels"] ** 2 // TILE
EDGE_SHAPES = {"8x8": (8, 8), "5x13": (5, 13), "13x5": (13, 5), "16x16": (16, 16), "13x20": (13, 20), "20x13": (20, 13), "16x32": (16, 32),
               "19x27": (19, 27), "27x19": (27, 19)}
EDGE_NORMALS = ("5x13", "20x13", "27x19")           # one shape of every bucket above 1, once more through normals=
EDGE_LEVEL_SHAPES = ("32x32", "13x20")
EDGE_LEVEL_KINDS = ("equal", "sl off")
SWEEP_PHI, SWEEP_FORECAST = (0.0, 0.5, 1.0), (-0.5, 0.0, 0.5)
LONG_HP = (255, 256, 257, 4095, 4096)
LONG_LEVELS = np.array([0.5, 1.0, 2.0, 3.0, 4.0])
LATE = 2048                        # a record step above it needs the high byte of its 16-bit slot and a pair number above 1023


def npl_of(nodes):
    """The nodes a lane owns in the instantiation of k_otr_walk that a mesh of `nodes` nodes gets."""
    rows = -(-nodes // TILE)
    return next((s for s in NPL_STEPS if rows <= s), NPL_MAX)


def shape_of(name):
    return tuple(int(x) for x in name.split("x"))


def edge_levels(n, kind, side):
    if kind == "equal":
        return np.full(n, 0.75)                                      # one step passes every level of a side
    if kind == "sl off" and side == "sl":
        return np.full(n, INF)                                       # that side is never done: every exit is profit or time
    v = 0.25 * np.arange(1, n + 1)
    if kind == "open":
        v[-1] = INF                                                  # neither side is ever done: every path is walked to max_hp
    return v


def edge_mesh_case(name, kind="plain", max_hp=24):
    """mesh_case's parameter set on an n_pt x n_sl mesh."""
    n_pt, n_sl = shape_of(name)
    return dict(forecast=[0.5], phi=[PHI5], sigma=[2.0], pt=edge_levels(n_pt, kind, "pt"), sl=edge_levels(n_sl, kind, "sl"), max_hp=max_hp,
                n_paths=TILE + 1, seed=13)


def sweep_case():
    """Nine parameter sets on 5 x 13: no memory, mean reversion and a random walk, each towards a forecast below, at and above 0."""
    case = edge_mesh_case("5x13")
    phi = [p for p in SWEEP_PHI for _ in SWEEP_FORECAST]
    return dict(case, forecast=[f for _ in SWEEP_PHI for f in SWEEP_FORECAST], phi=phi, sigma=[2.0] * len(phi))


def long_case(max_hp):
    """Two slow parameter sets whose paths still pass levels late in a long horizon."""
    return dict(forecast=[0.5, 0.0], phi=[2.0 ** -0.001, 1.0], sigma=[0.1, 0.05], pt=LONG_LEVELS, sl=LONG_LEVELS, max_hp=max_hp,
                n_paths=TILE + 1, seed=5)


def long_steer_rows(max_hp):
    """One shock per path (phi = 1, sigma = 1, forecast 0: the path is the shock from its step on), at steps counted from max_hp."""
    shocks = ((max_hp - 1, 1.5),       # 0: passes pt[0] at the step before the last
              (max_hp, 1.5),           # 1: ... at the last step
              (max_hp - 1, -1.5),      # 2, 3: the same below -sl[0]
              (max_hp, -1.5),
              (None, 0.0),             # 4: never moves
              (LATE + 1, 1.5),         # 5: the first step of a pair in the middle
              (LATE + 2, -1.5),        # 6: the second step of that pair
              (max_hp, 1.0),           # 7: on pt[0] at the last step: not passed
              (max_hp - 1, 3.5))       # 8: every pt level one step before the last: the walk stops there
    z = np.zeros((len(shocks), max_hp))
    for p, (h, v) in enumerate(shocks):
        if h is not None:
            z[p, h - 1] = v
    return z


def long_steer_case(max_hp):
    z = np.tile(long_steer_rows(max_hp), (8, 1))                     # 72 paths: more than one tile
    return dict(forecast=[0.0], phi=[1.0], sigma=[1.0], pt=STEER_PT, sl=STEER_SL, max_hp=max_hp, n_paths=len(z), seed=0), z


def long_steer_node00(max_hp):
    """Node (0, 0) of long_steer_case by hand -> (hold, n_profit, n_stop, n_time): rows 0, 1, 5, 8 profit, 2, 3, 6 stop, 4, 7 time."""
    steps = (max_hp - 1, max_hp, max_hp - 1, max_hp, max_hp, LATE + 1, LATE + 2, max_hp, max_hp - 1)
    return 8 * sum(steps), 8 * 4, 8 * 3, 8 * 2


SPLIT_CFG, SPLIT_PERIOD = 1024, 61


def split_case():
    """What one launch's partials cannot hold: 1024 parameter sets (set c has the parameters of set c % 61) on 32 x 32 over 17
    blocks of paths."""
    rng = np.random.default_rng(1361)
    f, phi, sg = rng.uniform(-1.0, 1.0, SPLIT_PERIOD), rng.uniform(0.5, 1.0, SPLIT_PERIOD), rng.uniform(0.5, 2.0, SPLIT_PERIOD)
    pick = np.arange(SPLIT_CFG) % SPLIT_PERIOD
    lv = 0.25 * np.arange(1, 33)
    return dict(forecast=f[pick], phi=phi[pick], sigma=sg[pick], pt=lv, sl=lv, max_hp=2, n_paths=16 * B + 1, seed=17)


def split_cpl(case):
    """Parameter sets per launch, from the cap in csrc/fmk_otr.hip."""
    txt = open(os.path.join(ROOT, "finmlkit_amd", "csrc", "fmk_otr.hip")).read()
    a, s = re.search(r"OTR_PARTIAL_CAP\s*=\s*\(size_t\)\s*(\d+)\s*<<\s*(\d+)\s*;", txt).groups()
    n_blocks = -(-case["n_paths"] // B)
    return (int(a) << int(s)) // (n_blocks * len(case["pt"]) * len(case["sl"]) * 16)


def one_set(case, c):
    return dict(case, forecast=[case["forecast"][c]], phi=[case["phi"][c]], sigma=[case["sigma"][c]])


def edge_cases():
    """name -> case: every generated mesh of the edge tests that has a reference of its own."""
    out = {name: edge_mesh_case(name) for name in EDGE_SHAPES}
    out.update({f"{name} max_hp 25": edge_mesh_case(name, max_hp=25) for name in EDGE_NORMALS})
    out["5x13 open max_hp 25"] = edge_mesh_case("5x13", "open", 25)  # 5 x 13's own levels are all passed before step 25
    out.update({f"{name} {kind}": edge_mesh_case(name, kind) for name in EDGE_LEVEL_SHAPES for kind in EDGE_LEVEL_KINDS})
    out["sweep"] = sweep_case()
    out.update({f"long {hp}": long_case(hp) for hp in LONG_HP})
    return out


EDGE_CASES = edge_cases()


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """The reference of EDGE_CASES[name], computed once and read-only."""
    m = reference(EDGE_CASES[name])
    for v in m.values():
        v.setflags(write=False)
    return m


# ---------------------------------------------------------------------------------------------- the generator
N_STAT, HP_STAT = 1 << 16, 24


def test_generator_moments_and_independence():
    z = R.normals(20260113, N_STAT, HP_STAT)
    n = z.size
    mean, var = z.mean(), z.var()
    print("mean", mean, "var", var)
    assert abs(mean) < 6.0 / math.sqrt(n)
    assert abs(var - 1.0) < 6.0 * math.sqrt(2.0 / n)
    kurt = ((z - mean) ** 4).mean() / var ** 2
    print("kurtosis", kurt)
    assert abs(kurt - 3.0) < 6.0 * math.sqrt(24.0 / n)
    steps = np.corrcoef(z[:, :-1].ravel(), z[:, 1:].ravel())[0, 1]           # also the two members of a pair
    rows = np.corrcoef(z[:-1].ravel(), z[1:].ravel())[0, 1]
    print("corr steps", steps, "corr paths", rows)
    assert abs(steps) < 6.0 / math.sqrt(z[:, 1:].size)
    assert abs(rows) < 6.0 / math.sqrt(z[1:].size)


def test_attempt_counts():
    a = R.attempts(20260113, N_STAT, HP_STAT)
    share, q = (a == 1).mean(), math.pi / 4.0
    print("accepted at attempt 0", share)
    assert abs(share - q) < 6.0 * math.sqrt(q * (1.0 - q) / a.size)
    assert a.max() <= R.ATTEMPTS and (a >= 2).any()


def test_the_words_are_the_bootstraps():
    from tests import _seqboot_ref
    assert R.word(0, 0) == 0xE220A8397B1DCDAF                            # splitmix64's first output from state 0
    for seed, i in ((5, 77), ((1 << 64) - 1, (1 << 51) - 1)):
        assert _seqboot_ref.word(seed, i) == R.word(seed, i)
    assert R.index(3, 5, 2, 1) == ((((3 << 12) | 5) << 6 | 2) << 1) | 1
    assert R.uniform(0) == -1.0 and R.uniform((1 << 64) - 1) == 1.0 - 2.0 ** -52


# ---------------------------------------------------------------------------------------------- the untouched node
def test_untouched_node_against_the_closed_forms():
    n, T, f, phi, sg = 8259, 24, 1.25, PHI5, 0.9
    m = R.mesh([f], [phi], [sg], [INF], [INF], T, n, 99, B)
    want_mean = f * (1.0 - phi ** T)
    want_var = sg * sg * (1.0 - phi ** (2 * T)) / (1.0 - phi * phi)
    mean, var = m["mean"][0, 0, 0], m["std"][0, 0, 0] ** 2
    print("mean", mean, want_mean, "var", var, want_var)
    assert abs(mean - want_mean) < 6.0 * math.sqrt(want_var / n)
    assert abs(var - want_var) < 6.0 * want_var * math.sqrt(2.0 / n)
    assert m["n_time"][0, 0, 0] == n and m["n_profit"][0, 0, 0] == 0 and m["n_stop"][0, 0, 0] == 0 and m["hold"][0, 0, 0] == n * T


# ---------------------------------------------------------------------------------------------- the header on the host
@pytest.fixture(scope="module")
def otr_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("otr") / "otr_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "otr_check.cpp"), "-o", exe])
    return exe


def test_record_walk_against_the_per_node_loop(otr_check):
    """tools/otr_check.cpp, built from csrc/fmk_otr_rule.h with the host compiler alone, in its quick form."""
    r = subprocess.run([otr_check, "quick"], capture_output=True, text=True)
    assert r.returncode == 0 and "failed checks 0" in r.stdout, r.stdout
    paths, nodes, early = (int(x) for x in re.search(r"paths (\d+) nodes (\d+) early (\d+)", r.stdout).groups())
    assert paths > 3000 and nodes > 100000 and early > 100


@pytest.mark.parametrize("c", [0, 1])
def test_rule_header_mesh_equals_the_reference(otr_check, c):
    """The rule's text (record walk, block sums, statistics) on the host against the independent reference, bit for bit."""
    case = seam_case(2 * B + TILE + 3, max_hp=25)
    want = reference(case)
    args = [str(case["n_paths"]), str(case["max_hp"]), str(case["seed"])]
    args += [float(case[k][c]).hex() for k in ("forecast", "phi", "sigma")] + [str(len(case["pt"])), str(len(case["sl"]))]
    args += [float(v).hex() for v in list(case["pt"]) + list(case["sl"])]
    out = subprocess.run([otr_check, "mesh"] + args, capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.splitlines():
        w = line.split()
        if w[0] != "node":
            continue
        i, j = int(w[1]), int(w[2])
        got = [float.fromhex(x) for x in w[3:6]] + [int(x) for x in w[6:]]
        for k, g in zip(FIELDS, got):
            r = want[k][c, i, j]
            assert g == r or (g != g and r != r), (k, i, j, g, r)
        seen += 1
    assert seen == 16


# ---------------------------------------------------------------------------------------------- ou_fit
def test_ou_fit_recovers_a_simulated_path():
    f, phi, sg, n = 100.0, 0.9, 0.5, 4000
    p = R.simulate(f, phi, sg, n, seed=4, start=f)
    got_phi, got_sigma = P.ou_fit(p, f)
    print("phi", got_phi, "sigma", got_sigma)
    assert abs(got_phi - phi) < 6.0 * math.sqrt((1.0 - phi * phi) / n)       # the least-squares slope of an AR(1)
    assert abs(got_sigma - sg) < 6.0 * sg / math.sqrt(2.0 * n)


def test_ou_fit_is_exact_without_noise():
    p = 3.0 + 8.0 * 0.5 ** np.arange(12)                                # dyadic: every product and sum is exact
    phi, sigma = P.ou_fit(p, 3.0)
    assert phi == 0.5 and sigma == 0.0
    assert label.ou_fit is P.ou_fit


@pytest.mark.parametrize("prices, forecast", [([1.0, 2.0], 0.0), ([[1.0, 2.0, 3.0]], 0.0), ([1.0, NAN, 2.0], 0.0), ([1.0, INF, 2.0], 0.0),
                                              ([1.0, 2.0, 3.0], NAN), ([2.0, 2.0, 5.0], 2.0)])
def test_ou_fit_refuses(prices, forecast):
    with pytest.raises(ValueError, match="ou_fit"):
        P.ou_fit(np.array(prices), forecast)


# ---------------------------------------------------------------------------------------------- the mesh object
def hand_mesh(sharpe, pt, sl):
    s = np.asarray(sharpe, np.float64)
    z, zi = np.zeros(s.shape), np.zeros(s.shape, np.int64)
    one = np.zeros(s.shape[0])
    return P.OTRMesh(z, z, s, zi, zi, zi, zi + 30, np.asarray(pt, float), np.asarray(sl, float), one, one, one, 10, 20, 0)


def test_best_is_the_first_largest_finite_sharpe():
    m = hand_mesh([[[0.1, INF, 0.7], [NAN, 0.7, -INF]], [[NAN, NAN, NAN], [-2.0, -1.0, -1.0]]], [1.0, 2.0], [0.5, 1.5, 2.5])
    assert m.best() == (1.0, 2.5, 0.7) and m.best(0) == m.best()
    assert m.best(1) == (2.0, 1.5, -1.0)
    assert m.horizontal_barriers(0.5) == (5.0, 2.0) and m.horizontal_barriers(2.0, cfg=1) == (0.75, 1.0)
    assert np.array_equal(m.mean_hold, np.full((2, 2, 3), 1.5))
    with pytest.raises(ValueError, match="finite Sharpe"):
        hand_mesh([[[NAN, INF]]], [1.0], [1.0, 2.0]).best()
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="target"):
            m.horizontal_barriers(bad)


def test_horizontal_barriers_are_what_tbmlabel_takes():
    m = hand_mesh([[[0.1, 0.9]]], [1.0], [0.5, 1.5])
    idx = pd.date_range("2024-01-01", periods=8, freq="min")
    label.TBMLabel._check(pd.DataFrame({"ret": np.full(8, 0.01)}, index=idx), "ret", 0.0, m.horizontal_barriers(0.5), False)


# ---------------------------------------------------------------------------------------------- what Python refuses
GOOD = dict(forecast=0.0, half_life=5.0, sigma=1.0, profit_taking=[1.0], stop_loss=[1.0], max_hp=4, n_paths=2, seed=0)
REFUSED = {
    "no phi": dict(half_life=None), "both": dict(phi=0.5), "half_life 0": dict(half_life=0.0), "half_life nan": dict(half_life=NAN),
    "phi low": dict(half_life=None, phi=-0.1), "phi high": dict(half_life=None, phi=1.5), "phi nan": dict(half_life=None, phi=NAN),
    "forecast inf": dict(forecast=INF), "sigma nan": dict(sigma=NAN), "sigma negative": dict(sigma=-1.0),
    "no broadcast": dict(forecast=[0.0, 1.0], sigma=[1.0, 2.0, 3.0]), "two dimensions": dict(forecast=[[0.0, 1.0]]),
    "too many sets": dict(forecast=np.zeros(1025)), "no sets": dict(forecast=np.zeros(0)),
    "no pt": dict(profit_taking=[]), "33 pt": dict(profit_taking=np.arange(33.0)), "no sl": dict(stop_loss=[]),
    "33 sl": dict(stop_loss=np.arange(33.0)), "negative level": dict(profit_taking=[-1.0, 1.0]), "nan level": dict(stop_loss=[1.0, NAN]),
    "decreasing": dict(stop_loss=[2.0, 1.0]), "levels 2-d": dict(profit_taking=[[1.0, 2.0]]),
    "max_hp 0": dict(max_hp=0), "max_hp 4097": dict(max_hp=4097), "max_hp float": dict(max_hp=4.0),
    "n_paths 0": dict(n_paths=0), "n_paths 2^32 + 1": dict(n_paths=(1 << 32) + 1), "seed float": dict(seed=1.5),
    "normals shape": dict(normals=np.zeros((2, 3))), "normals nan": dict(normals=np.array([[0.0, NAN, 0.0, 0.0], [0.0] * 4])),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_python_refuses_before_a_device_is_touched(name, monkeypatch):
    from finmlkit_amd import _ffi

    def no_device():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    with pytest.raises(ValueError, match="optimal_trading_rule"):
        P.optimal_trading_rule(**{**GOOD, **REFUSED[name]})


def test_geometry_and_exports():
    assert GEO == {"block": B, "tile": TILE, "max_levels": 32, "max_hp": 4096}
    assert B % TILE == 0 and TILE == 64 and B >= 2 * TILE
    assert (P.MAX_LEVELS, P.MAX_HP, P.MAX_PATHS, P.MAX_CFG) == (32, 4096, 1 << 32, 1024)
    assert label.optimal_trading_rule is P.optimal_trading_rule and label.OTRMesh is P.OTRMesh
    assert {"optimal_trading_rule", "ou_fit", "OTRMesh"} <= set(label.__all__)


# ---------------------------------------------------------------------------------------------- what the GPU cases hold
def test_seam_cases_hold_every_exit_kind_an_early_stop_and_a_second_attempt():
    case = seam_case(B + 1)
    m = reference(case)
    for k in ("n_profit", "n_stop", "n_time"):
        assert (m[k] > 0).any(), k
    assert np.array_equal(m["n_profit"] + m["n_stop"] + m["n_time"], np.full(m["hold"].shape, B + 1))
    # some path passes every profit-taking level (or every stop-loss level) before the last step: the walk stops early
    z = R.normals(case["seed"], case["n_paths"], case["max_hp"])
    for c in range(2):
        Pth = R.paths(case["forecast"][c], case["phi"][c], case["sigma"][c], z)
        assert ((Pth[:, :-1] > MESH4[-1]).any(axis=1) | (Pth[:, :-1] < -MESH4[-1]).any(axis=1)).any()
    for n in PATH_SEAMS[-4:]:
        assert (R.attempts(n, n, 24) >= 2).any()
    assert sorted(set(PATH_SEAMS)) == sorted({1, 63, 64, 65, TILE - 1, TILE + 1, B - 1, B, B + 1, 2 * B + TILE + 3})


def test_steered_cases_put_values_on_levels():
    case, z = steer_case()
    Pth = R.paths(0.0, 1.0, 1.0, z)
    assert np.array_equal(Pth, np.cumsum(z, axis=1))                     # dyadic: exact
    assert Pth[0, 0] == STEER_PT[0] and Pth[5, 0] == -STEER_SL[0] and Pth[8, 3] == STEER_PT[1]
    assert Pth[1, 0] == np.nextafter(1.0, 2.0) and Pth[6, 0] == np.nextafter(-1.0, -2.0)
    m = reference(case, z)
    x, step, kind = R.node_exits(Pth[:9], STEER_PT[0], STEER_SL[0])
    assert list(kind) == [2, 0, 0, 0, 0, 2, 1, 1, 0] and list(step) == [4, 1, 4, 1, 1, 4, 1, 2, 3]
    assert list(x) == [1.0, 1.0 + ULP, 1.5, 2.5, 3.5, -1.0, -1.0 - ULP, -2.5, 1.5]
    x, step, kind = R.node_exits(Pth[:9], STEER_PT[1], STEER_SL[1])
    assert list(kind) == [2, 2, 2, 0, 0, 2, 2, 1, 2] and step[3] == 1 and step[7] == 2 and x[8] == 2.0
    assert m["n_profit"][0, 0, 0] == 8 * 5 and m["n_stop"][0, 0, 0] == 8 * 2 and m["n_time"][0, 0, 0] == 8 * 2


def test_no_noise_cases_have_zero_deviation():
    m = reference(no_noise_case())
    assert (m["std"] == 0.0).all()
    assert np.isnan(m["sharpe"][0]).all() and (m["n_time"][0] == TILE + 5).all()            # 0 is on the zero levels: never passed
    assert (m["sharpe"][1] == INF).all() and (m["n_profit"][1] == TILE + 5).all()
    assert (m["sharpe"][2] == -INF).all() and (m["n_stop"][2] == TILE + 5).all()
    assert m["hold"][1, 2, 0] == 3 * (TILE + 5)                          # 1, 1.5, 1.75: the first value above 1.5 is the third


# ---------------------------------------------------------------------------------------------- what the edge cases hold
def test_edge_shapes_reach_every_walk_from_both_sides_of_its_boundaries():
    assert all(shape_of(name) == s for name, s in EDGE_SHAPES.items())
    nodes = {name: s[0] * s[1] for name, s in EDGE_SHAPES.items()}
    npl = {name: npl_of(n) for name, n in nodes.items()}
    assert NPL_MAX == 16 and set(npl.values()) == set(NPL_STEPS) | {NPL_MAX}
    for step in NPL_STEPS:                                               # the last node count of a bucket, and the first of the next
        edge = step * TILE
        assert any(edge - 4 <= n <= edge and npl_of(n) == step for n in nodes.values()), edge
        assert any(edge < n <= edge + 4 and npl_of(n) > step for n in nodes.values()), edge
    # every bucket above 1 has a mesh and its transpose, with and without normals=: node / n_sl against node % n_sl
    for bucket in (4, 8, NPL_MAX):
        names = [name for name in EDGE_SHAPES if npl[name] == bucket]
        assert any(f"{b}x{a}" in names and a != b for a, b in (shape_of(name) for name in names)), bucket
        assert sum(name in EDGE_NORMALS for name in names) == 1
    assert all(a != b for a, b in (shape_of(name) for name in EDGE_NORMALS))
    assert {npl_of(a * b) for a, b in (shape_of(name) for name in EDGE_LEVEL_SHAPES)} == {8, NPL_MAX}
    # the levels are distinct on both sides, so a transposed node index gives another mesh
    m, t = edge_reference("5x13"), edge_reference("13x5")
    assert not np.array_equal(m["n_profit"][0], t["n_profit"][0].T) and not np.array_equal(m["mean"][0, :, :5], m["mean"][0, :, :5].T)
    for name in EDGE_SHAPES:
        m = edge_reference(name)
        assert (m["n_profit"] > 0).all() and (m["n_stop"] > 0).all(), name
        assert (m["n_time"] > 0).any() == (npl[name] >= 8), name       # the far levels of the larger meshes: all three exit kinds


def test_edge_normals_cases_end_on_the_first_step_of_a_pair():
    for name in EDGE_NORMALS:
        case = EDGE_CASES[f"{name} max_hp 25"]
        z = R.normals(case["seed"], case["n_paths"], case["max_hp"])
        assert z.shape == (TILE + 1, 25) and np.array_equal(z[:, :24], R.normals(case["seed"], case["n_paths"], 24))
        Pth = R.paths(case["forecast"][0], case["phi"][0], case["sigma"][0], z[:, :24])
        alive = int(((Pth.max(axis=1) <= case["pt"][-1]) & (Pth.min(axis=1) >= -case["sl"][-1])).sum())      # paths walked to step 25
        m = edge_reference(f"{name} max_hp 25")
        print(name, "paths at step 25", alive)
        assert (alive > 0) == (name != "5x13") and (alive > 0) == (not np.array_equal(m["hold"], edge_reference(name)["hold"]))
    m = edge_reference("5x13 open max_hp 25")                            # ... and 5 x 13 with open ends: every path is
    assert (m["n_time"][0, -1, -1] == TILE + 1) and m["hold"][0, -1, -1] == 25 * (TILE + 1) and (m["n_profit"][0, 0] > 0).all()


def test_edge_level_lists_fill_a_side_at_once_and_switch_a_side_off():
    for name in EDGE_LEVEL_SHAPES:
        m = edge_reference(f"{name} equal")
        for k in FIELDS:
            assert (m[k] == m[k][0, 0, 0]).all(), (name, k)              # every node is the same node
        assert m["n_profit"][0, 0, 0] > 0 and m["n_stop"][0, 0, 0] > 0
        m = edge_reference(f"{name} sl off")
        assert (m["n_stop"] == 0).all() and (m["n_profit"] > 0).any() and (m["n_time"] > 0).any()
        assert (np.diff(m["n_profit"], axis=1) <= 0).all() and (m["n_profit"][:, :, :1] == m["n_profit"]).all()


def test_repeated_infinite_levels_are_taken_without_a_warning():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(P._levels("stop_loss", np.full(3, INF)), [INF] * 3)
        assert np.array_equal(P._levels("stop_loss", EDGE_CASES["13x20 sl off"]["sl"]), np.full(20, INF))
    for bad in ([INF, 1.0], [1.0, INF, 2.0], [2.0, 1.0]):
        with pytest.raises(ValueError, match="non-decreasing"):
            P._levels("stop_loss", bad)


def test_sweep_sets_are_nine_different_processes():
    case = sweep_case()
    sets = set(zip(case["forecast"], case["phi"], case["sigma"]))
    assert len(sets) == 9 and {p for _, p, _ in sets} == set(SWEEP_PHI) and {f for f, _, _ in sets} == set(SWEEP_FORECAST)
    m = edge_reference("sweep")
    means = {m["mean"][c].tobytes() for c in range(9)}
    assert len(means) == 7                     # at phi = 1 the forecast has no pull: (1 - phi) * forecast = 0, three equal sets
    assert np.array_equal(m["mean"][6], m["mean"][7]) and np.array_equal(m["mean"][6], m["mean"][8])


LONG_FIGURES = ((52, 35, 0, 9), (125, 147, 0, 35))          # late profit exits, late stop exits, least and most n_time of a set's nodes


@pytest.mark.parametrize("max_hp", [4095, 4096])
def test_long_cases_hold_late_records_on_both_barriers(max_hp):
    case = long_case(max_hp)
    z = R.normals(case["seed"], case["n_paths"], max_hp)
    m = edge_reference(f"long {max_hp}")
    for c in range(2):
        Pth = R.paths(case["forecast"][c], case["phi"][c], case["sigma"][c], z)
        late = [0, 0]
        for pt in LONG_LEVELS:
            for sl in LONG_LEVELS:
                _, step, kind = R.node_exits(Pth, pt, sl)
                late[0] += int(((kind == 0) & (step > LATE)).sum())
                late[1] += int(((kind == 1) & (step > LATE)).sum())
        print("set", c, "late profit", late[0], "late stop", late[1], "n_time", m["n_time"][c].min(), m["n_time"][c].max())
        assert late[0] > 0 and late[1] > 0
        assert m["n_time"][c].min() == 0 and m["n_time"][c].max() > 0
        assert (late[0], late[1], m["n_time"][c].min(), m["n_time"][c].max()) == LONG_FIGURES[c]
        assert m["hold"][c].max() > 1 << 16                              # a sum of large steps, itself past 16 bits
    assert {255, 256, 257} <= set(LONG_HP) and max_hp in LONG_HP and GEO["max_hp"] == 4096


@pytest.mark.parametrize("max_hp", [4095, 4096])
def test_long_steered_cases_pass_levels_in_the_last_pair(max_hp):
    case, z = long_steer_case(max_hp)
    assert z.shape == (72, max_hp) and (np.count_nonzero(z, axis=1) <= 1).all()
    Pth = R.paths(0.0, 1.0, 1.0, z)
    assert np.array_equal(Pth, np.cumsum(z, axis=1))                     # one shock: exact
    x, step, kind = R.node_exits(Pth[:9], STEER_PT[0], STEER_SL[0])
    H = max_hp
    assert list(kind) == [0, 0, 1, 1, 2, 0, 1, 2, 0] and list(step) == [H - 1, H, H - 1, H, H, LATE + 1, LATE + 2, H, H - 1]
    assert list(x) == [1.5, 1.5, -1.5, -1.5, 0.0, 1.5, -1.5, 1.0, 3.5]
    # the pair of a step: steps 2k + 1 and 2k + 2 are the first and the second of pair k
    first = [h % 2 == 1 for h in step[:4]]
    assert first == ([True, False, True, False] if H % 2 == 0 else [False, True, False, True])
    m = reference(case, z)
    node = tuple(int(m[k][0, 0, 0]) for k in ("hold", "n_profit", "n_stop", "n_time"))
    assert node == long_steer_node00(max_hp) and node[0] == 8 * (7 * H + 2 * LATE)
    assert m["n_profit"][0, 2, 0] == 8 and m["n_stop"][0, 0, 1] == 0     # row 8 alone passes pt[2]; nothing passes -sl[1]


def test_split_case_needs_two_launches_that_do_not_share_a_period():
    case = split_case()
    cpl = split_cpl(case)
    n_cfg = len(case["forecast"])
    print("sets per launch", cpl)
    assert n_cfg == SPLIT_CFG == P.MAX_CFG and 1 < cpl < n_cfg <= 2 * cpl and cpl % SPLIT_PERIOD != 0
    assert case["n_paths"] == 16 * B + 1 and len(case["pt"]) == len(case["sl"]) == GEO["max_levels"]
    sets = list(zip(case["forecast"], case["phi"], case["sigma"]))
    assert len(set(sets[:SPLIT_PERIOD])) == SPLIT_PERIOD and all(sets[c] == sets[c % SPLIT_PERIOD] for c in range(n_cfg))
    f, phi, sg = (np.asarray(case[k]) for k in ("forecast", "phi", "sigma"))
    assert (np.abs(f) <= 1.0).all() and (phi >= 0.5).all() and (phi <= 1.0).all() and (sg >= 0.5).all() and (sg <= 2.0).all()
    assert one_set(case, cpl)["forecast"] == [f[cpl % SPLIT_PERIOD]]


# ---------------------------------------------------------------------------------------------- the header on the host, on the edge cases
def tool_mesh(exe, case, c):
    """tools/otr_check.cpp's mesh of parameter set c -> {field: (n_pt, n_sl) array}"""
    args = [str(case["n_paths"]), str(case["max_hp"]), str(case["seed"])]
    args += [float(case[k][c]).hex() for k in ("forecast", "phi", "sigma")] + [str(len(case["pt"])), str(len(case["sl"]))]
    args += [float(v).hex() for v in list(case["pt"]) + list(case["sl"])]
    out = subprocess.run([exe, "mesh"] + args, capture_output=True, text=True, check=True).stdout
    shape = (len(case["pt"]), len(case["sl"]))
    got = {k: np.full(shape, NAN if k in FIELDS[:3] else -1, np.float64 if k in FIELDS[:3] else np.int64) for k in FIELDS}
    seen = 0
    for line in out.splitlines():
        w = line.split()
        if w[0] != "node":
            continue
        i, j = int(w[1]), int(w[2])
        for k, v in zip(FIELDS, [float.fromhex(x) for x in w[3:6]] + [int(x) for x in w[6:]]):
            got[k][i, j] = v
        seen += 1
    assert seen == shape[0] * shape[1]
    return got


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_rule_header_mesh_equals_the_reference_on_the_edge_cases(otr_check, name):
    """The generated meshes of tests/test_gpu_otr_edges.py through the rule's text on the host: a mismatch on the GPU is the kernel's."""
    case, want = EDGE_CASES[name], edge_reference(name)
    for c in range(len(case["forecast"])):
        got = tool_mesh(otr_check, case, c)
        for k in FIELDS:
            assert np.array_equal(got[k], want[k][c], equal_nan=(k == "sharpe")), (name, c, k)
