"""The optimal trading rules of Advances in Financial Machine Learning, chapter 13: which profit-taking and stop-loss levels, and
which maximum holding period, to hand to the triple-barrier labels.  A discrete Ornstein-Uhlenbeck process is fitted to the prices
(`ou_fit`, equation 13.2), many paths are simulated from it, each path is closed at a profit-taking level, a stop-loss level or the
maximum holding period, and the Sharpe ratio of every pair on a mesh of levels is read off (`optimal_trading_rule`, snippets 13.1 and
13.2).  The reference has no such function: the definition is this project's, with counter-based random
numbers and a fixed summing order, so that a mesh is a function of its arguments and nothing else.  The paths are walked on the
MI355X (csrc/fmk_otr.hip), one walk per path for the whole mesh."""
from __future__ import annotations

import ctypes as C
import operator
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
from numpy.typing import NDArray

from .. import _ffi
from .._ffi import c_i64, ptr

MAX_LEVELS, MAX_HP, MAX_PATHS, MAX_CFG = 32, 4096, 1 << 32, 1024


def geometry() -> dict:
    """The kernel's geometry (fmk_otr_geometry): needs no device.  block: the paths of one block of the sums (the definition's B);
    tile: the paths walked at once; max_levels, max_hp: the limits."""
    out = (C.c_int64 * 4)()
    _ffi.check(_ffi.lib().fmk_otr_geometry(out))
    return dict(zip(("block", "tile", "max_levels", "max_hp"), (int(v) for v in out)))


def ou_fit(prices: NDArray[np.float64], forecast: float) -> Tuple[float, float]:
    """Equation 13.2 on the host: with X = P[:-1] - forecast and Z = P[1:] - forecast, phi = sum(X Z) / sum(X X) and sigma is the
    root mean square of Z - phi X -> (phi, sigma).  ValueError: fewer than 3 prices, a price or a forecast that is not finite, or
    sum(X X) == 0 (every price but the last on the forecast)."""
    p = np.asarray(prices, dtype=np.float64)
    if p.ndim != 1 or p.size < 3:
        raise ValueError("ou_fit: prices must be a one-dimensional array of at least 3 elements.")
    forecast = float(forecast)
    if not np.isfinite(forecast) or not np.isfinite(p).all():
        raise ValueError("ou_fit: the prices and the forecast must be finite.")
    x, z = p[:-1] - forecast, p[1:] - forecast
    sxx = float(np.dot(x, x))
    if sxx == 0.0:
        raise ValueError("ou_fit: every price before the last equals the forecast: phi is not determined.")
    phi = float(np.dot(x, z)) / sxx
    resid = z - phi * x
    return phi, float(np.sqrt(np.dot(resid, resid) / resid.size))


@dataclass(frozen=True)
class OTRMesh:
    """The mesh of one `optimal_trading_rule` call.  The seven arrays have the shape (n_cfg, n_pt, n_sl): mean, std and sharpe of
    the closing values (float64); n_profit, n_stop and n_time, the paths that closed at each barrier (int64, their sum is n_paths);
    hold, the sum of the exit steps (int64).  profit_taking and stop_loss are the level lists; forecast, phi and sigma the parameter
    sets, each of n_cfg elements."""
    mean: NDArray[np.float64]
    std: NDArray[np.float64]
    sharpe: NDArray[np.float64]
    n_profit: NDArray[np.int64]
    n_stop: NDArray[np.int64]
    n_time: NDArray[np.int64]
    hold: NDArray[np.int64]
    profit_taking: NDArray[np.float64]
    stop_loss: NDArray[np.float64]
    forecast: NDArray[np.float64]
    phi: NDArray[np.float64]
    sigma: NDArray[np.float64]
    max_hp: int
    n_paths: int
    seed: int

    @property
    def mean_hold(self) -> NDArray[np.float64]:
        """The mean holding period of every node, in steps."""
        return self.hold / self.n_paths

    def best(self, cfg: int = 0) -> Tuple[float, float, float]:
        """-> (profit_taking, stop_loss, sharpe) of the node with the largest finite Sharpe ratio of parameter set `cfg`, the
        smallest flat index among equals.  ValueError when no Sharpe ratio of the set is finite."""
        s = self.sharpe[cfg].reshape(-1)
        finite = np.isfinite(s)
        if not finite.any():
            raise ValueError("OTRMesh.best: no node of this parameter set has a finite Sharpe ratio.")
        k = int(np.argmax(np.where(finite, s, -np.inf)))
        i, j = divmod(k, len(self.stop_loss))
        return float(self.profit_taking[i]), float(self.stop_loss[j]), float(s[k])

    def horizontal_barriers(self, target: float, cfg: int = 0) -> Tuple[float, float]:
        """The best node of parameter set `cfg` as the tuple TBMLabel and triple_barrier take, (bottom, top) in multiples of the
        target return: (stop_loss / target, profit_taking / target).  `target` is the target return in the units of the prices
        that were fitted.  ValueError unless target is finite and positive."""
        target = float(target)
        if not (np.isfinite(target) and target > 0.0):
            raise ValueError("OTRMesh.horizontal_barriers: target must be finite and positive.")
        pt, sl, _ = self.best(cfg)
        return sl / target, pt / target


def _levels(name, v):
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.float64)))
    if a.ndim != 1 or not 1 <= a.size <= MAX_LEVELS:
        raise ValueError(f"optimal_trading_rule: {name} must hold between 1 and 32 levels.")
    if np.isnan(a).any() or (a < 0.0).any() or (a[1:] < a[:-1]).any():           # not np.diff: inf - inf warns
        raise ValueError(f"optimal_trading_rule: the {name} levels must be non-negative and non-decreasing, without NaN.")
    return a


def optimal_trading_rule(forecast, half_life, sigma, profit_taking, stop_loss, max_hp: int = 100, n_paths: int = 100_000,
                         seed: int = 0, *, phi=None, normals: Optional[NDArray[np.float64]] = None) -> OTRMesh:
    """-> the OTRMesh of the profit_taking x stop_loss levels for every parameter set.  forecast, half_life and sigma are scalars or
    one-dimensional arrays, broadcast to n_cfg sets; the autoregressive coefficient is phi = 2 ** (-1 / half_life), or phi= is given
    and half_life is None.  A path starts at 0, so forecast and the levels are distances from the entry price, in the units of sigma's
    prices.  profit_taking, stop_loss: non-negative, non-decreasing lists of 1 .. 32 levels (+inf: that barrier is off); max_hp: the
    maximum holding period in steps (1 .. 4096); n_paths: 1 .. 2^32; seed: equal seeds give equal meshes, and all parameter sets
    of a call see the same random numbers; normals: an (n_paths, max_hp) float64 array that replaces the generator's variates
    (tests steer paths with it).
    ValueError: a limit above, parameters that do not broadcast, a forecast or sigma that is not finite, sigma < 0, phi outside
    [0, 1], half_life <= 0, both or neither of half_life and phi, levels that are negative, decreasing or NaN, normals of another
    shape or not finite."""
    what = "optimal_trading_rule"
    if (half_life is None) == (phi is None):
        raise ValueError(f"{what}: give half_life or phi=, not both (with phi=, half_life must be None).")
    if phi is None:
        hl = np.asarray(half_life, dtype=np.float64)
        if not (np.isfinite(hl).all() and (hl > 0.0).all()):
            raise ValueError(f"{what}: half_life must be finite and positive.")
        phi = 2.0 ** (-1.0 / hl)
    try:
        f, ph, sg = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (forecast, phi, sigma)))
    except ValueError:
        raise ValueError(f"{what}: forecast, half_life (or phi) and sigma must broadcast to one length.") from None
    if f.ndim != 1:
        raise ValueError(f"{what}: forecast, half_life (or phi) and sigma must be scalars or one-dimensional.")
    if not 1 <= f.size <= MAX_CFG:
        raise ValueError(f"{what}: between 1 and 1024 parameter sets.")
    f, ph, sg = (np.ascontiguousarray(v, dtype=np.float64) for v in (f, ph, sg))
    if not (np.isfinite(f).all() and np.isfinite(sg).all()):
        raise ValueError(f"{what}: forecast and sigma must be finite.")
    if (sg < 0.0).any():
        raise ValueError(f"{what}: sigma must not be negative.")
    if not ((ph >= 0.0) & (ph <= 1.0)).all():
        raise ValueError(f"{what}: phi must lie in [0, 1].")
    pt, sl = _levels("profit_taking", profit_taking), _levels("stop_loss", stop_loss)
    try:
        max_hp, n_paths, seed = operator.index(max_hp), operator.index(n_paths), operator.index(seed)
    except TypeError:
        raise ValueError(f"{what}: max_hp, n_paths and seed must be integers.") from None
    if not 1 <= max_hp <= MAX_HP:
        raise ValueError(f"{what}: max_hp must be between 1 and 4096.")
    if not 1 <= n_paths <= MAX_PATHS:
        raise ValueError(f"{what}: n_paths must be between 1 and 2^32.")
    seed &= (1 << 64) - 1
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        if normals.shape != (n_paths, max_hp):
            raise ValueError(f"{what}: normals must have the shape (n_paths, max_hp).")
        if not np.isfinite(normals).all():
            raise ValueError(f"{what}: the normals must be finite.")
    shape = (f.size, pt.size, sl.size)
    out = [np.empty(shape, np.float64) for _ in range(3)] + [np.empty(shape, np.int64) for _ in range(4)]
    _ffi.default_context().call("fmk_otr_mesh", ptr(f), ptr(ph), ptr(sg), c_i64(f.size), ptr(pt), c_i64(pt.size), ptr(sl),
                                c_i64(sl.size), c_i64(max_hp), c_i64(n_paths), C.c_uint64(seed), ptr(normals),
                                *(ptr(o) for o in out))
    return OTRMesh(*out, pt, sl, f, ph, sg, max_hp, n_paths, seed)
