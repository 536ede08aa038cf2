"""GPU: the optimal-trading-rule mesh (finmlkit_amd/label/otr.py, csrc/fmk_otr.hip) against tests/_otr_ref.py.
"equal" is bit-equal on all seven outputs (the NaN of a Sharpe ratio by position).  Path counts over the seams of tile and block,
odd and single-step horizons, the mesh shapes up to 32 x 32 with zero, repeated and infinite levels, paths steered onto levels,
sigma = 0, many parameter sets against their one-set calls, seeds, the closed forms on 2^20 paths, every refusal of the C layer and
the way from ou_fit to TBMLabel."""
import ctypes as C
import math

import numpy as np
import pandas as pd
import pytest

from finmlkit_amd import _ffi, label
from finmlkit_amd.label import otr as P
from tests import _otr_ref as R
from tests.test_otr_host import (B, FIELDS, MESH_SHAPES, PATH_SEAMS, PHI5, STEP_SEAMS, TILE, book_case, mesh_case, no_noise_case, reference,
                                 seam_case, steer_case)

pytestmark = pytest.mark.gpu
INF = math.inf


def run(case, z=None):
    return P.optimal_trading_rule(case["forecast"], None, case["sigma"], case["pt"], case["sl"], case["max_hp"], case["n_paths"],
                                  case["seed"], phi=case["phi"], normals=z)


def assert_same(got, want, what=""):
    for k in FIELDS:
        g, w = getattr(got, k) if not isinstance(got, dict) else got[k], want[k] if isinstance(want, dict) else getattr(want, k)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        if k == "sharpe":
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
            g, w = np.where(np.isnan(g), 0.0, g), np.where(np.isnan(w), 0.0, w)
        assert np.array_equal(g, w), (what, k, g.ravel()[:4], w.ravel()[:4])


@pytest.mark.parametrize("n_paths", PATH_SEAMS)
def test_seams_of_the_path_axis(n_paths):
    case = seam_case(n_paths)
    assert_same(run(case), reference(case), n_paths)


@pytest.mark.parametrize("max_hp", STEP_SEAMS)
def test_seams_of_the_step_axis(max_hp):
    case = seam_case(2 * B + 1, max_hp)
    got = run(case)
    assert_same(got, reference(case), max_hp)
    if max_hp == 1:
        assert (got.hold == 2 * B + 1).all()


@pytest.mark.parametrize("kind", ["plain", "edges"])
@pytest.mark.parametrize("name", list(MESH_SHAPES))
def test_mesh_shapes(name, kind):
    case = mesh_case(name, kind)
    got = run(case)
    assert got.sharpe.shape == (1,) + MESH_SHAPES[name]
    assert_same(got, reference(case), (name, kind))


def test_steered_paths():
    case, z = steer_case()
    got = run(case, z)
    assert_same(got, reference(case, z))
    assert got.n_profit[0, 0, 0] == 40 and got.n_stop[0, 0, 0] == 16 and got.n_time[0, 0, 0] == 16
    # on a level is not past it: with only the paths that sit on pt[0] and -sl[0], nothing is ever passed
    on = np.tile(z[[0, 5]], (TILE, 1))
    only = P.optimal_trading_rule(0.0, None, 1.0, case["pt"], case["sl"], 4, len(on), 0, phi=1.0, normals=on)
    assert (only.n_time == len(on)).all() and (only.mean == 0.0).all() and (only.std == 1.0).all() and (only.hold == 4 * len(on)).all()


def test_no_noise():
    case = no_noise_case()
    got = run(case)
    assert_same(got, reference(case))
    assert (got.std == 0.0).all() and np.isnan(got.sharpe[0]).all() and (got.sharpe[1] == INF).all() and (got.sharpe[2] == -INF).all()


def test_many_parameter_sets_share_the_random_numbers():
    case = book_case()
    got = run(case)
    assert_same(got, reference(case))
    for c in (0, 7, 12, 24):
        one = P.optimal_trading_rule(case["forecast"][c], None, case["sigma"][c], case["pt"], case["sl"], case["max_hp"], case["n_paths"],
                                     case["seed"], phi=case["phi"][c])
        assert_same({k: getattr(got, k)[c:c + 1] for k in FIELDS}, one, c)
    # the half-life form gives the same phi
    hl = P.optimal_trading_rule(case["forecast"], case["half_life"], 1.0, case["pt"], case["sl"], case["max_hp"], case["n_paths"], case["seed"])
    assert np.array_equal(hl.phi, case["phi"]) and hl.sigma.shape == (25,)
    assert_same(got, hl)


def test_seeds():
    base = dict(seam_case(B + 1), seed=0)
    meshes = {}
    for seed in (0, 1, (1 << 64) - 1):
        case = dict(base, seed=seed)
        meshes[seed] = run(case)
        assert_same(meshes[seed], reference(case), seed)
    assert_same(run(base), meshes[0])
    assert not np.array_equal(meshes[0].mean, meshes[1].mean) and not np.array_equal(meshes[1].mean, meshes[(1 << 64) - 1].mean)
    assert_same(run(dict(base, seed=-1)), meshes[(1 << 64) - 1])         # seeds count modulo 2^64


def test_against_the_closed_forms():
    n, T, f, phi, sg = 1 << 20, 16, 1.25, PHI5, 0.9
    got = P.optimal_trading_rule(f, None, sg, [0.5, INF], [0.75, INF], T, n, 2026, phi=phi)
    want_mean = f * (1.0 - phi ** T)
    want_var = sg * sg * (1.0 - phi ** (2 * T)) / (1.0 - phi * phi)
    mean, var = got.mean[0, 1, 1], got.std[0, 1, 1] ** 2
    print("mean", mean, want_mean, "var", var, want_var)
    assert abs(mean - want_mean) < 6.0 * math.sqrt(want_var / n)
    assert abs(var - want_var) < 6.0 * want_var * math.sqrt(2.0 / n)
    assert np.array_equal(got.n_profit + got.n_stop + got.n_time, np.full((1, 2, 2), n))
    assert got.hold[0, 1, 1] == T * n and got.n_time[0, 1, 1] == n
    assert got.n_profit[0, 0, 0] > 0 and got.n_stop[0, 0, 0] > 0 and got.hold[0, 0, 0] < T * n
    assert np.array_equal(got.mean_hold, got.hold / n)


def c_call(n_cfg=1, forecast=(0.0,), phi=(0.5,), sigma=(1.0,), pt=(1.0,), sl=(1.0,), n_pt=None, n_sl=None, max_hp=4, n_paths=8, seed=0,
           normals=None, outputs=True):
    arr = [np.ascontiguousarray(v, dtype=np.float64) for v in (forecast, phi, sigma, pt, sl)]
    n_pt, n_sl = len(arr[3]) if n_pt is None else n_pt, len(arr[4]) if n_sl is None else n_sl
    cells = max(1, n_cfg) * max(1, min(n_pt, 32)) * max(1, min(n_sl, 32))
    out = [np.zeros(cells, np.float64) for _ in range(3)] + [np.zeros(cells, np.int64) for _ in range(4)]
    nz = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
    ctx = _ffi.default_context()
    rc = _ffi.lib().fmk_otr_mesh(ctx.handle, _ffi.ptr(arr[0]), _ffi.ptr(arr[1]), _ffi.ptr(arr[2]), C.c_int64(n_cfg), _ffi.ptr(arr[3]),
                                 C.c_int64(n_pt), _ffi.ptr(arr[4]), C.c_int64(n_sl), C.c_int64(max_hp), C.c_int64(n_paths),
                                 C.c_uint64(seed), _ffi.ptr(nz), *[(_ffi.ptr(o) if outputs else None) for o in out])
    return rc, out


REFUSALS = {
    "n_cfg 0": dict(n_cfg=0), "n_cfg 1025": dict(n_cfg=1025, forecast=np.zeros(1025), phi=np.zeros(1025), sigma=np.zeros(1025)),
    "n_pt 0": dict(n_pt=0), "n_pt 33": dict(pt=np.arange(33.0)), "n_sl 0": dict(n_sl=0), "n_sl 33": dict(sl=np.arange(33.0)),
    "max_hp 0": dict(max_hp=0), "max_hp 4097": dict(max_hp=4097), "n_paths 0": dict(n_paths=0), "n_paths 2^32 + 1": dict(n_paths=(1 << 32) + 1),
    "phi 1.5": dict(phi=(1.5,)), "phi negative": dict(phi=(-0.5,)), "phi nan": dict(phi=(math.nan,)), "sigma negative": dict(sigma=(-1.0,)),
    "sigma inf": dict(sigma=(INF,)), "forecast nan": dict(forecast=(math.nan,)), "pt negative": dict(pt=(-1.0, 1.0)),
    "pt decreasing": dict(pt=(2.0, 1.0)), "sl nan": dict(sl=(1.0, math.nan)), "normals inf": dict(normals=np.full((8, 4), INF)),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_of_the_c_layer(name):
    rc, _ = c_call(**REFUSALS[name])
    assert rc == _ffi.E_ARG, name
    assert b"otr_mesh" in _ffi.lib().fmk_last_error(_ffi.default_context().handle)


def test_the_limits_themselves_and_null_outputs_are_accepted():
    rc, full = c_call()
    assert rc == _ffi.OK
    rc, _ = c_call(outputs=False)
    assert rc == _ffi.OK
    lv = 0.125 * np.arange(32)
    rc, out = c_call(pt=lv, sl=lv, max_hp=4096, n_paths=3, phi=(1.0,), sigma=(0.0,))
    assert rc == _ffi.OK and (out[5] == 3).all() and (out[6] == 3 * 4096).all()
    want = R.mesh([0.0], [0.5], [1.0], [1.0], [1.0], 4, 8, 0, B)
    for k, o in zip(FIELDS, full):
        assert o[0] == want[k][0, 0, 0] or (o[0] != o[0] and np.isnan(want[k][0, 0, 0])), k


def test_from_ou_fit_to_tbmlabel():
    forecast, phi, sigma, n = 100.0, 0.9, 0.5, 2000
    prices = R.simulate(forecast, phi, sigma, n, seed=8, start=forecast + 1.0)
    fit_phi, fit_sigma = label.ou_fit(prices, forecast)
    levels = fit_sigma * np.linspace(0.5, 4.0, 8)
    mesh = label.optimal_trading_rule(forecast - prices[-1], None, fit_sigma, levels, levels, 20, B + 1, 5, phi=fit_phi)
    pt, sl, sharpe = mesh.best()
    assert math.isfinite(sharpe) and pt in levels and sl in levels
    barriers = mesh.horizontal_barriers(fit_sigma)
    assert barriers == (sl / fit_sigma, pt / fit_sigma)
    idx = pd.date_range("2024-01-01", periods=n, freq="min")
    features = pd.DataFrame({"ret": np.full(n, fit_sigma / forecast)}, index=idx)
    kit = label.TBMLabel(features, "ret", 0.0, barriers, pd.Timedelta(minutes=20))
    assert kit.horizontal_barriers == barriers
