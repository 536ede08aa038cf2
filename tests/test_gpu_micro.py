"""GPU: the per-bar microstructure features (Kyle, Amihud, Hasbrouck, Roll) against the definition in
tests/_micro_ref.py, through the host-pointer function and the resident form: every bar length around the schedules' switches, the
group edges of the lane-per-bar schedule, hand-built bars with known answers at every alignment, bad ticks, independence from the
partition, the kits and the refusals.  "Equal" is R.assert_equal: NaN / inf / exact zero bit for bit, roll_spread the function of
the returned serial_cov, serial_cov and lambda inside their derived bounds, t-values within the tolerance measured in
tests/test_micro_host.py."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest

from tests import _micro_ref as R
from tests.test_micro_host import HAND_LENGTHS, T_TOL, closes, hand_bars, lengths_to_closes, rows, tape

pytestmark = pytest.mark.gpu

LANE_MAX = 32                  # csrc/fmk_micro.hip MC_LANE_MAX: bars of up to 32 ticks go a lane per bar, longer ones a wave per bar
TILE = 1024                    # MC_TILE: ticks of a wave's LDS tile
SWEEP = (0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 191, 193, 255, 257, 1000, 70001)


def host_form(p, v, sd, ci):
    from finmlkit_amd.bar.base import comp_bar_microstructure_features
    out = comp_bar_microstructure_features(p, v, ci, sd)
    assert isinstance(out, tuple) and len(out) == 8
    return dict(zip(R.COLS, out))


def resident_form(p, v, sd, ci):
    from finmlkit_amd._ffi import DeviceArray
    from finmlkit_amd.engine import DeviceTrades
    t = DeviceTrades.from_numpy(np.arange(len(p), dtype=np.int64), p, v, sd)
    out = t.bar_microstructure(DeviceArray.from_host(t.ctx, np.ascontiguousarray(ci, np.int64)))
    assert list(out) == list(R.COLS) and all(isinstance(a, DeviceArray) for a in out.values())
    return {k: a.to_host() for k, a in out.items()}


def both_forms(p, v, sd, ci):
    a, b = host_form(p, v, sd, ci), resident_form(p, v, sd, ci)
    for k in R.COLS:
        assert R.same_bits(a[k], b[k]), k
    return a


# ---------------------------------------------------------------------------------------------- the bar-length sweep
@functools.lru_cache(maxsize=None)
def sweep_case(name, first):
    p, v, sd = tape(name)
    ci = lengths_to_closes(SWEEP, first)
    n = int(ci[-1]) + 1 + 5                                   # a few ticks behind the last bar
    p, v, sd = p[:n], v[:n], sd[:n]
    return p, v, sd, ci, both_forms(p, v, sd, ci)


@pytest.mark.parametrize("first", [-1, 37])
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_bar_length_sweep(name, first):
    assert LANE_MAX in SWEEP and LANE_MAX + 1 in SWEEP
    p, v, sd, ci, got = sweep_case(name, first)
    assert v.dtype == (np.float32 if name == "f32" else np.float64)
    ref = R.reference(p, v, sd, ci)
    for b in range(3):                                        # 0, 1 and 2 ticks: NaN rows
        assert all(np.isnan(got[c][b]) for c in R.COLS)
    assert not np.isnan(got["serial_cov"][3:]).any()
    R.assert_equal(got, ref, T_TOL[name], f"sweep {name} {first}")


def test_a_bar_is_a_function_of_the_bar_alone():
    p, v, sd, ci, got = sweep_case("f32", -1)
    s, e = int(ci[-2]) + 1, int(ci[-1])
    assert e - s + 1 == 70001
    alone = both_forms(p[s:e + 1].copy(), v[s:e + 1].copy(), sd[s:e + 1].copy(), np.array([-1, e - s]))
    for c in R.COLS:
        assert R.same_bits(alone[c], got[c][-1:]), c
    # and of nothing around it: the same bars behind another first close
    other = sweep_case("f32", 37)[4]
    p2, v2, sd2 = tape("f32")
    shifted = both_forms(p2[38:38 + int(ci[-1]) + 1].copy(), v2[38:38 + int(ci[-1]) + 1].copy(), sd2[38:38 + int(ci[-1]) + 1].copy(), ci)
    for c in R.COLS:
        assert R.same_bits(shifted[c], other[c]), c


# ---------------------------------------------------------------------------------------------- group edges of the lane schedule
@pytest.mark.parametrize("nbars", [63, 64, 65, 129])
def test_lane_groups_of_short_bars(nbars):
    rng = np.random.default_rng(nbars)
    ci = lengths_to_closes(rng.integers(1, 9, nbars), 11)
    p, v, sd = (a[:int(ci[-1]) + 1] for a in tape("f32"))
    R.assert_equal(both_forms(p, v, sd, ci), R.reference(p, v, sd, ci), T_TOL["f32"], f"{nbars} short bars")


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_a_group_that_overflows_the_tile_is_split(name):
    # 70 bars of 28 .. 32 ticks: 64 of them hold about 1 900 ticks, the tile 1 024; then a bar longer than the tile between short ones
    rng = np.random.default_rng(5)
    lengths = list(rng.integers(28, 33, 70)) + [3, TILE + 1, 7, TILE, 9, TILE - 1, 2, 30]
    ci = lengths_to_closes(lengths)
    p, v, sd = (a[:int(ci[-1]) + 1] for a in tape(name))
    R.assert_equal(both_forms(p, v, sd, ci), R.reference(p, v, sd, ci), T_TOL[name], "split group")


# ---------------------------------------------------------------------------------------------- hand-built bars, every alignment
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("lane", [0, 1, 63])
def test_hand_built_bars_wherever_their_first_tick_falls(lane, f32):
    fp, fv, fs = tape("f64")
    ps, vs, ss, lengths, marks = [], [], [], [], []
    at = 0
    for L in HAND_LENGTHS:
        for label, p, v, sd, chk in hand_bars(L):
            fill = (lane - at) % 64 + 64                      # filler ticks in front: a bar of their own
            ps += [fp[at:at + fill], p]; vs += [fv[at:at + fill], v]; ss += [fs[at:at + fill], sd]
            lengths += [fill, L]
            at += fill
            assert at % 64 == lane
            marks.append((len(lengths) - 1, label, chk))
            at += L
    p, v, sd = np.concatenate(ps), np.concatenate(vs), np.concatenate(ss).astype(np.int8)
    v = v.astype(np.float32) if f32 else v
    ci = lengths_to_closes(lengths)
    got = both_forms(p, v, sd, ci)
    r = rows(got)
    for b, label, chk in marks:
        chk(r[b])
    # the measured t-value tolerance speaks for the tape's bars (the fillers); a hand-built bar has its known answers and the derived bounds
    tape_bars = np.ones(len(lengths), bool)
    tape_bars[[b for b, _, _ in marks]] = False
    R.assert_equal(got, R.reference(p, v, sd, ci), T_TOL["f32" if f32 else "f64"], f"hand-built bars at lane {lane}", t_bars=tape_bars)


# ---------------------------------------------------------------------------------------------- bad ticks
BAD = {"nan price": ("p", np.nan), "zero price": ("p", 0.0), "negative price": ("p", -101.5), "inf amount": ("v", np.inf),
       "nan amount": ("v", np.nan)}


@pytest.mark.parametrize("kind", list(BAD))
def test_bad_ticks(kind):
    name = "f32" if kind in ("zero price", "inf amount") else "f64"
    p0, v0, sd0 = tape(name)
    ci = closes(name)[:60]
    n = int(ci[-1]) + 1
    p0, v0, sd0 = p0[:n], v0[:n], sd0[:n]
    base = both_forms(p0, v0, sd0, ci)
    L = np.diff(ci)
    short = int(np.flatnonzero((L >= 5) & (L <= LANE_MAX))[3])
    long_ = int(np.flatnonzero(L > 70)[1])
    col, val = BAD[kind]
    for b in (short, long_):
        s, e = int(ci[b]) + 1, int(ci[b + 1])
        for t in (s, (s + e) // 2, s + 64 if e - s > 70 else s + 1, e):
            p, v, sd = p0.copy(), v0.copy(), sd0.copy()
            (p if col == "p" else v)[t] = val
            got = host_form(p, v, sd, ci) if t != e else both_forms(p, v, sd, ci)
            R.assert_equal(got, R.reference(p, v, sd, ci), T_TOL[name], f"{kind} at tick {t} of bar {b}")
            if col == "p":
                assert np.isnan(got["amihud_lambda"][b]) and np.isnan(got["hasbrouck_t"][b])
            others = np.arange(len(L)) != b
            for c in R.COLS:
                assert R.same_bits(got[c][others], base[c][others]), (kind, t, c, "a neighbouring bar changed")


# ---------------------------------------------------------------------------------------------- kits and resident forms
def kit_trades(n, with_side=True):
    from finmlkit_amd.bar.data_model import TradesData
    p, v, sd = (a[:n] for a in tape("f32"))
    ts = 1_600_000_000_000_000_000 + np.arange(n, dtype=np.int64) * 250_000_000
    return TradesData(ts, p.copy(), v.copy(), np.arange(n), side=sd.copy() if with_side else None)


def test_time_bar_kit_and_the_resident_form_agree_with_the_function():
    from finmlkit_amd.bar.kit import TimeBarKit
    kit = TimeBarKit(kit_trades(20_000), pd.Timedelta(minutes=1))
    df = kit.build_microstructure_features()
    assert list(df.columns) == list(R.COLS) and df.index.name == "timestamp"
    np.testing.assert_array_equal(df.index.values.astype(np.int64), kit.bar_close_timestamps)
    t = kit.trades_df
    p, v, sd, ci = t["price"].values, t["amount"].values, t["side"].values, kit._close_indices
    assert len(df) == len(ci) - 1 > 50
    want = host_form(p, v, sd, ci)
    res = {k: a.to_host() for k, a in kit._device().bar_microstructure(kit._d_close_idx).items()}
    for c in R.COLS:
        assert df[c].dtype == np.float64 and R.same_bits(df[c].values, want[c]) and R.same_bits(res[c], want[c]), c
    R.assert_equal(want, R.reference(p, v, sd, ci), T_TOL["f32"], "one-minute bars")


def test_imbalance_bar_kit_end_to_end():
    from finmlkit_amd.bar import ImbalanceBarKit
    kit = ImbalanceBarKit(kit_trades(20_000), 12.0)
    df = kit.build_microstructure_features()
    t = kit.trades_df
    p, v, sd, ci = t["price"].values, t["amount"].values, t["side"].values, kit._close_indices
    assert len(df) == len(ci) - 1 > 20 and list(df.columns) == list(R.COLS)
    np.testing.assert_array_equal(df.index.values.astype(np.int64), kit.bar_close_timestamps)
    R.assert_equal({c: df[c].values for c in R.COLS}, R.reference(p, v, sd, ci), T_TOL["f32"], "imbalance bars")


def test_refusals_leave_the_context_usable():
    from finmlkit_amd import _ffi
    from finmlkit_amd._ffi import DeviceArray, c_i64, ptr
    from finmlkit_amd.bar.kit import TimeBarKit
    from finmlkit_amd.engine import DeviceTrades
    p, v, sd = (np.ascontiguousarray(a[:500]) for a in tape("f32"))
    ci = lengths_to_closes([40, 3, 200, 17])
    good = host_form(p, v, sd, ci)
    ctx = _ffi.default_context()
    outs = {k: np.empty(len(ci) - 1) for k in R.COLS}

    def call(ci_, n_idx=None, **alias):
        st = _ffi.MicrostructureOut(**{k: alias.get(k, a.ctypes.data) for k, a in outs.items()})
        ctx.call("fmk_comp_bar_microstructure", ptr(p), ptr(v), C.c_int(0), c_i64(len(p)), ptr(ci_), c_i64(len(ci_) if n_idx is None else n_idx),
                 ptr(sd), C.byref(st))
    for bad in (np.array([-1, 39, 500]), np.array([-2, 39, 100]), np.array([-1, 39, 2 ** 40])):
        with pytest.raises(ValueError, match="close index"):
            call(bad)
    with pytest.raises(ValueError, match="negative dimensions"):
        call(ci, n_idx=0)
    with pytest.raises(ValueError, match="alias"):
        call(ci, kyle_t=p.ctypes.data)
    with pytest.raises(ValueError, match="alias"):
        call(ci, roll_spread=ci.ctypes.data + 8)
    call(ci[:1])                                              # one close index: zero bars, succeeds
    # the resident form: a bad close index is found on the device and the bar is not read; an aliased output is refused up front
    t = DeviceTrades.from_numpy(np.arange(500, dtype=np.int64), p, v, sd)
    for bad in (np.array([-1, 39, 500]), np.array([-7, 39, 100]), np.array([-1, 39, 2 ** 40, 60])):
        with pytest.raises(ValueError, match="close index"):
            t.bar_microstructure(DeviceArray.from_host(t.ctx, bad))
    d_ci = DeviceArray.from_host(t.ctx, ci)
    d_out = {k: DeviceArray(t.ctx, len(ci) - 1, np.float64) for k in R.COLS}
    st = _ffi.MicrostructureOut(**{**{k: a.ptr for k, a in d_out.items()}, "serial_cov": t.price.ptr + 16})
    with pytest.raises(ValueError, match="alias"):
        t.ctx.call("fmk_comp_bar_microstructure_dev", t.price.p, t.amount.p, C.c_int(0), c_i64(500), d_ci.p, c_i64(len(ci)), t.side.p, C.byref(st))
    with pytest.raises(KeyError, match="side"):
        TimeBarKit(kit_trades(2_000, with_side=False), pd.Timedelta(minutes=1)).build_microstructure_features()
    # both contexts still work
    again = both_forms(p, v, sd, ci)
    for c in R.COLS:
        assert R.same_bits(again[c], good[c]), c
    res = {k: a.to_host() for k, a in t.bar_microstructure(d_ci).items()}
    for c in R.COLS:
        assert R.same_bits(res[c], good[c]), c
