"""GPU: the running extrema of the order-flow columns at the reference's start values, on every order-flow schedule.

comp_bar_directional_features starts cum_volumes_min / max and cum_dollars_min / max at 1e9 / -1e9 (base.py:459-464): a bar whose
running signed volume or dollar sum stays above 1e9 (below -1e9) from its first tick reports exactly 1e9 (-1e9).  Whale-sized trades
(amounts of 1e9 .. 4e9, or more than 1e9 in dollars per trade) reach that on every bar that is all buys or all sells.  The tape below
runs through cfg 4's one-pass kernels (FMK_FUSED=2: integer units, direct stores; 3: float64 volumes, deferred stores), its two-pass
form (0), each with and without the forced tick-order redo, and through the stand-alone order-flow schedules (one lane per bar, one
wave per bar, a workgroup per bar) -- all against the oracle, which tests/test_oracle_golden.py pins to the reference's own vectors of
tests/golden/extrema_clamp.npz; that tape runs here too."""
import numpy as np
import pytest

from tests import _golden as G
from tests.test_gpu_features import _check_dir
from tests.test_gpu_fused import _check_all, _fused

pytestmark = pytest.mark.gpu

FU_MAXT = 1536          # csrc/fmk_fused.h: longer bars take k_fu_long
BFW_MIN = 16384         # csrc/fmk_barflow.hip: longer bars take k_bar_dir_wide


def whale_tape(n=300_000, seed=5):
    """-> (px, am float32, sd, ci, kinds): bars of 150 .. 900 ticks, a dozen of 1 600 .. 6 000 (k_fu_long) and three of 17 000 ..
    20 000 (k_bar_dir_wide); each bar holds one kind of amounts -- 0 ordinary dyadic sizes, 1 whale sizes (whole multiples of 2^20 in
    [1e9, 4e9)), 2 full-mantissa whale sizes, 3 sizes of ~1.1e7 that are whole multiples of 2^6 (at a price of ~100 the dollar sum
    passes 1e9 from the first trade) -- and about 30 % of the bars are all buys or all sells."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(150, 900, n // 500)
    at = rng.choice(len(lens) // 2, 15, replace=False)          # (in the first half: they survive the cut at n - 1)
    lens[at[:12]] = rng.integers(FU_MAXT + 64, 6000, 12)
    lens[at[12:]] = rng.integers(BFW_MIN + 600, 20000, 3)
    ci = np.concatenate([[-1], np.cumsum(lens) - 1])
    ci = ci[ci <= n - 1].astype(np.int64)
    nb = len(ci) - 1
    kinds = rng.integers(0, 4, nb)
    kinds[at[:8]] = [1, 2] * 4                                    # most long bars of whale sizes, and one-sided (below)
    kinds[at[12:]] = 1
    bar_of = np.full(n, -1, np.int64)
    bar_of[:ci[-1] + 1] = np.repeat(np.arange(nb), np.diff(ci))
    kind_of = np.where(bar_of >= 0, kinds[np.maximum(bar_of, 0)], 0)
    am = np.select([kind_of == 1, kind_of == 2, kind_of == 3],
                   [rng.integers(954, 3815, n) * 2.0 ** 20, rng.uniform(1e9, 4e9, n), rng.integers(160_000, 190_000, n) * 64.0],
                   rng.integers(1, 4097, n) / 1024.0).astype(np.float32)
    one_sided = rng.random(nb) < 0.3
    one_sided[at[:8]] = one_sided[at[12:14]] = True
    sign = np.where(rng.random(nb) < 0.5, 1, -1)
    sd = rng.choice(np.array([-1, 1], np.int8), n)
    fixed = (bar_of >= 0) & one_sided[np.maximum(bar_of, 0)]
    sd[fixed] = sign[bar_of[fixed]]
    px = np.round(100.0 + np.cumsum(rng.integers(-1, 2, n)) * 0.01, 2)
    return px, am, sd, ci, kinds


def _clamped(want):
    """bars at the start value in each of the four columns"""
    return [int((want[i] == np.float32(v)).sum()) for i, v in ((10, 1e9), (11, -1e9), (12, 1e9), (13, -1e9))]


def test_whale_tape_reaches_the_start_values(orc):
    px, am, sd, ci, kinds = whale_tape()
    want = orc.comp_bar_directional_features(px, am, ci, sd, raise_on_zero_div=False)
    nb = len(ci) - 1
    for c in _clamped(want):
        assert 0.04 * nb < c < 0.5 * nb
    # ... from bars of each kind of amounts, and from long bars
    vol_at, dol_at = want[10] == np.float32(1e9), want[12] == np.float32(1e9)
    assert vol_at[kinds == 1].any() and vol_at[kinds == 2].any()
    assert dol_at[kinds == 3].any() and not vol_at[kinds == 3].any()
    assert vol_at[np.diff(ci) > FU_MAXT].any()


@pytest.mark.parametrize("redo", ["0", "1"])
@pytest.mark.parametrize("fused", ["0", "2", "3"])
def test_whale_extrema_cfg4(orc, monkeypatch, fused, redo):
    """cfg 4 (bars_fused) on the whale tape: every output against the oracle, and the separate reducers' bits (_check_all).
    redo 1: every bar's float32 order-flow columns are recomputed in tick order (FMK_DIR_FORCE_REDO)."""
    monkeypatch.setenv("FMK_FUSED", fused)
    monkeypatch.setenv("FMK_DIR_FORCE_REDO", redo)
    px, am, sd, ci, _ = whale_tape()
    mode = _check_all(orc, px, am, sd, ci, f"whales FMK_FUSED={fused} redo={redo}")
    assert mode[0] == {"0": 0, "2": 1, "3": 2}[fused]


@pytest.mark.parametrize("knobs", [
    {"FMK_DIR_LANES": "2"},                     # one lane per bar (k_bar_dir_lanes), longer bars by list to k_bar_dir / k_bar_dir_wide
    {"FMK_DIR_LANES": "0"},                     # one wave per bar (k_bar_dir) and k_bar_dir_wide
    {"FMK_DIR_LANES": "0", "FMK_DIR_FORCE_REDO": "1"},      # ... every bar then redone in tick order
    {"FMK_DIR_LANES": "2", "FMK_DIR_FORCE_REDO": "2"},      # the wave-per-bar redo kernel instead of the parallel one
])
def test_whale_extrema_directional_schedules(orc, monkeypatch, knobs):
    from finmlkit_amd import engine
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    px, am, sd, ci, _ = whale_tape()
    assert (np.diff(ci) > BFW_MIN).sum() == 3
    t = engine.DeviceTrades.from_numpy(np.zeros(len(px), np.int64), px, am, sd)
    cid = engine.DeviceArray.from_host(t.ctx, ci)
    d, nz = t.bar_directional(cid)
    d = engine.to_host(d)
    want = orc.comp_bar_directional_features(px, am, ci, sd, raise_on_zero_div=False)
    assert int(nz.to_host()[0]) == 0
    _check_dir(tuple(d[k] for k in G.DIR_KEYS), want, f"whales {knobs}")


@pytest.mark.parametrize("fused", ["0", "2", "3"])
def test_extrema_reference_tape(orc, monkeypatch, fused):
    """the reference's own vectors (tests/golden/extrema_clamp.npz) from cfg 4 and from the stand-alone order-flow call"""
    monkeypatch.setenv("FMK_FUSED", fused)
    d = G.load("extrema_clamp")
    px, am, sd, ci = d["price"], d["amount"], d["side"], d["close_idx"]
    want = tuple(d["dir_" + k] for k in G.DIR_KEYS)
    t, cid, o, dr, nz, off, flat, bar, bad = _fused(px, am, sd, ci)
    assert bad == 0 and nz == 0
    _check_dir(tuple(dr[k] for k in G.DIR_KEYS), want, f"reference tape FMK_FUSED={fused}")
    from finmlkit_amd import engine
    d2, _ = t.bar_directional(cid)
    d2 = engine.to_host(d2)
    _check_dir(tuple(d2[k] for k in G.DIR_KEYS), want, "reference tape, comp_bar_directional")
    _check_all(orc, px, am, sd, ci, f"reference tape FMK_FUSED={fused}")
