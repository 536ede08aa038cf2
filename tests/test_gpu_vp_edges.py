"""The rolling volume profile on the MI355X (csrc/fmk_volprofile.hip) on the hand-built footprints of tests/_vp_ref.py: windows of
1 .. 190 bars round the 63-bar chunks of the offsets, bars of 0 .. 200 levels round the 64 prefetched ones, windows of 1 .. 20 000
levels through the three LDS capacities and the global-scratch mode, a wave's histogram serving a second bar, ties of the tick
rounding, every bin rule, the argmax across lanes, the walk's exits, NaN and inf volumes, and what is refused.  Every output is
compared with the restatement on dtype, shape and bits (NaN at the same places); no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _vp_ref as H

pytestmark = pytest.mark.gpu

KEYS = ("poc", "hva", "lva", "pct")
GROUPS = ("winlen", "chunk_empties", "bar_widths", "feeder", "place", "levels", "one_wide", "half_tick", "near_half_cent", "bins",
          "bincount", "walk", "special")
I32_SENTINEL, F32_SENTINEL = 0x5A5A5A5A, np.float32(-7.5e33)


def _group(g):
    return [n for n in H.CASES if n.split(".")[0] == g]


def test_groups_cover_the_table():
    assert sorted(n for g in GROUPS for n in _group(g)) == sorted(H.CASES)


def _ctx():
    from finmlkit_amd import _ffi
    return _ffi.default_context()


def _n_cu(ctx):
    v = C.c_int64()
    ctx.call("fmk_diag_n_cu", C.byref(v))
    return int(v.value)


def _compare(got, want, what):
    for k, a, b in zip(KEYS, got, want):
        H.same(a, b, f"{what}:{k}")
    return 4 * len(want[0])


# ---------------------------------------------------------------------------------------------- every case, CSR entry
@pytest.mark.parametrize("group", GROUPS)
def test_every_case_csr(group):
    from finmlkit_amd.feature.core.volume import volume_profile_rolling_csr
    n = 0
    classes = set()
    for name in _group(group):
        (want, info) = H.expected(name)
        n += _compare(volume_profile_rolling_csr(*H.args(name)), want, name)
        if info["L"]:
            classes.add(H.capacity_class(max(info["L"])))
    if group == "levels":                                        # all three LDS capacities and the scratch mode were used
        assert classes == {1024, 4096, 8192, "scratch"}
    if group == "one_wide":
        assert classes == {4096, "scratch"}
    _counts.record(f"vp_edges/csr/{group}", cases=len(_group(group)), outputs_compared=n)


# ---------------------------------------------------------------------------------------------- the ragged signature
RAGGED = ("winlen.63.k1", "winlen.64.k2", "winlen.190.k2", "chunk_empties.k2", "bar_widths.k1", "bar_widths.w0.k2", "place.dup.w2.k1",
          "place.gaps.w5.k2", "levels.1025.b27", "levels.8193.raw", "one_wide.8193.b5", "half_tick.0.5.w20", "bins.r20.5", "walk.sym.va150.0",
          "special.nan_two.va68.34", "special.roll_inf.64")


def test_ragged_signature():
    from finmlkit_amd.feature.core.volume import volume_profile_rolling
    n = 0
    for name in RAGGED:
        ts, hi, lo, off, lv, bv, sv, window, n_bins, tick, va = H.args(name)
        split = lambda a: [a[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        n += _compare(volume_profile_rolling(ts, hi, lo, split(lv), split(bv), split(sv), window, n_bins, tick, va), H.expected(name)[0], name)
    _counts.record("vp_edges/ragged", cases=len(RAGGED), outputs_compared=n)


# ---------------------------------------------------------------------------------------------- resident arrays, raw ABI
def _raw(ctx, fn, *a):
    from finmlkit_amd import _ffi
    rc = getattr(_ffi.lib(), fn)(ctx.handle, *a)
    return rc, _ffi.lib().fmk_last_error(ctx.handle).decode(errors="replace")


def _params(ts, window, n_bins, tick, va, n_bars=None):
    return (C.c_int64(len(ts) if n_bars is None else n_bars), C.c_int64(H.first_bar(ts, window) if len(ts) else 0),
            C.c_int64(int(window * 1e9)), C.c_int64(-1 if n_bins is None else n_bins), C.c_double(tick), C.c_double(va))


def _dev(ctx, data, window, n_bins, tick, va, n_bars=None):
    """fmk_volume_profile_rolling_dev on resident arrays, every output prefilled with a sentinel -> (status, message, outputs)."""
    from finmlkit_amd._ffi import DeviceArray
    nb = len(data[0])
    ins = [DeviceArray.from_host(ctx, a) for a in data]
    outs = [DeviceArray.from_host(ctx, np.full(nb, I32_SENTINEL, np.int32)) for _ in range(3)]
    outs.append(DeviceArray.from_host(ctx, np.full(nb, F32_SENTINEL, np.float32)))
    rc, msg = _raw(ctx, "fmk_volume_profile_rolling_dev", *[d.p for d in ins], *_params(data[0], window, n_bins, tick, va, n_bars),
                   *[o.p for o in outs])
    got = [o.to_host() for o in outs] if rc == 0 else None
    for d in ins + outs:
        d.free()
    return rc, msg, got


def _host(ctx, data, window, n_bins, tick, va, n_bars=None):
    from finmlkit_amd._ffi import ptr
    nb = len(data[0])
    outs = [np.full(nb, I32_SENTINEL, np.int32) for _ in range(3)] + [np.full(nb, F32_SENTINEL, np.float32)]
    rc, msg = _raw(ctx, "fmk_volume_profile_rolling", *[ptr(np.ascontiguousarray(a)) for a in data],
                   *_params(data[0], window, n_bins, tick, va, n_bars), *[ptr(o) for o in outs])
    return rc, msg, outs


DEV = ("winlen.1.k1", "winlen.63.k2", "winlen.64.k1", "winlen.65.k2", "winlen.127.k1", "winlen.190.k1", "chunk_empties.k1", "bar_widths.k2",
       "feeder.w190", "place.regular.w100.k1", "place.regular.w100.k2", "place.regular.w39.k1", "place.dup.w0.k2", "levels.1.raw",
       "levels.1024.b27", "levels.4097.raw", "levels.8192.b27.k2", "levels.20000.b27", "one_wide.1025.raw", "one_wide.8193.raw",
       "bins.r16.5", "bincount.129.1000000.k2", "walk.all_zero.va68.34", "walk.max_63_64.va68.34", "walk.ones_8192.va100.0",
       "special.nan_70_of_140.va68.34", "special.inf_two.b2", "special.roll_nan.190")


def test_resident_arrays_every_output_element_written():
    ctx = _ctx()
    n = 0
    for name in DEV:
        c = H.CASES[name]
        rc, msg, got = _dev(ctx, H.inputs(name), c["window"], c["n_bins"], c["tick"], c["va"])
        assert rc == 0, (name, rc, msg)
        n += _compare(got, H.expected(name)[0], name + " (_dev)")   # (a sentinel left behind differs from the zero the bar keeps)
    (out, info) = H.expected("place.regular.w100.k1")            # the window is longer than the series: nothing computed, all zero
    assert info["first"] == len(out[0]) and not any(a.any() for a in out)
    _counts.record("vp_edges/dev", cases=len(DEV), outputs_compared=n)


# ---------------------------------------------------------------------------------------------- a wave's histogram reused
@pytest.mark.parametrize("wide,n_bins", [(1024, 3), (1024, None), (4096, 3), (8192, None), (8193, 3), (8193, None)])
def test_a_wave_serves_a_second_bar(wide, n_bins):
    """More bars than one launch has waves (the launch caps: n_cu * 32 workgroups, of 4 waves in the 1024-level class; n_cu * 8 in the
    scratch mode): the waves that served the wide windows of bars 2, 3, 6 and 7, with volume at the top level, then serve narrow
    windows, and a slice that a narrow window used serves a wide one."""
    from finmlkit_amd.feature.core.volume import volume_profile_rolling_csr
    ctx = _ctx()
    n_cu = _n_cu(ctx)
    assert n_cu > 0
    cls = H.capacity_class(wide)
    waves = H.waves_per_launch(cls, n_cu)
    data = H.reuse(waves, wide)
    info = {}
    want = H.volume_profile_rolling(*data, 1.0, n_bins, 1.0, 68.34, info=info)
    L = np.array(info["L"])
    assert len(L) > waves + 12 and L.max() == wide and H.capacity_class(int(L.max())) == cls
    assert (L[[1, 2, 5, 6]] == wide).all() and (L[[1 + waves, 2 + waves, 5 + waves, 6 + waves]] == 5).all()   # computed bar i is L[i - 1]
    assert L[11] == 5 and L[11 + waves] == wide
    n = _compare(volume_profile_rolling_csr(*data, 1.0, n_bins, 1.0, 68.34), want, f"reuse {wide} {n_bins}")
    _counts.record(f"vp_edges/reuse/{wide}.{n_bins}", bars=len(L), waves=waves, n_cu=n_cu, outputs_compared=n)


# ---------------------------------------------------------------------------------------------- the stage functions
class _Product:
    """The product's stage functions under the restatement's CSR argument order."""

    @staticmethod
    def aggregate_footprint(ts, hi, lo, off, lv, bv, sv, start_ts, end_ts, tick):
        from finmlkit_amd.feature.core import volume
        return volume.aggregate_footprint(ts, hi, lo, lv, bv, sv, start_ts, end_ts, tick, level_offsets=off)

    def __getattr__(self, name):
        from finmlkit_amd.feature.core import volume
        return getattr(volume, name)


@pytest.mark.parametrize("group", ("levels", "bins", "bincount", "walk", "special"))
def test_stage_functions_on_the_one_window_cases(group):
    from finmlkit_amd.feature.core import volume
    n = cases = 0
    for name in _group(group):
        c = H.CASES[name]
        if not c["one"]:
            continue
        want = H.stage_outputs(H, H.inputs(name), c["n_bins"], c["tick"], c["va"])
        got = H.stage_outputs(_Product(), H.inputs(name), c["n_bins"], c["tick"], c["va"])
        assert len(got) == len(want)
        for j, (a, b) in enumerate(zip(got, want)):
            H.same(a, b, f"{name}: stage output {j}")
            n += a.size
        levels, tot = (want[3], want[4]) if c["n_bins"] is not None else (want[0], want[1] + want[2])
        share = H.calc_volume_percentage_above_poc(levels, tot, int(want[-2][0]))      # the float64 the typed function returns
        H.same(np.float64(volume.calc_volume_percentage_above_poc(levels, tot, int(want[-2][0]))), np.float64(share), name + ": share")
        n += 1
        cases += 1
    assert cases > 0
    _counts.record(f"vp_edges/stages/{group}", cases=cases, outputs_compared=n)


# ---------------------------------------------------------------------------------------------- refusals
def _good(ctx):
    """A good call on the same context right after a refusal: the status word is cleared per call."""
    name = "bins.r20.5"
    c = H.CASES[name]
    for fn in (_host, _dev):
        rc, msg, got = fn(ctx, H.inputs(name), c["window"], c["n_bins"], c["tick"], c["va"])
        assert rc == 0, (rc, msg)
        _compare(got, H.expected(name)[0], name + " after a refusal")


@pytest.mark.parametrize("name", sorted(H.REFUSALS))
def test_refusals_through_the_raw_abi(name):
    from finmlkit_amd import _ffi
    from finmlkit_amd.feature.core.volume import volume_profile_rolling_csr
    ctx = _ctx()
    c = H.REFUSALS[name]
    for fn in (_host, _dev):
        rc, msg, _ = fn(ctx, c["inputs"], c["window"], c["n_bins"], c["tick"], c["va"])
        assert rc == getattr(_ffi, c["code"]) and c["message"] in msg, (name, fn.__name__, rc, msg)
        _good(ctx)
    with pytest.raises(c["error"]):
        volume_profile_rolling_csr(*c["inputs"], c["window"], c["n_bins"], c["tick"], c["va"])
    _counts.record(f"vp_edges/refused/{name}", calls=3)


def test_no_bars_and_the_nan_rule():
    """n_bars 0 is refused in both flavours; a NaN low or high is refused in the rolling call and in aggregate_footprint (the
    reference's int(round(nan)) raises ValueError), also when every low and high of a window is NaN and its bars are empty -- no
    numbers come out of fmin / fmax skipping the NaN; a NaN in a bar that no computed window holds is not looked at."""
    from finmlkit_amd import _ffi
    from finmlkit_amd.feature.core.volume import aggregate_footprint, volume_profile_rolling_csr
    ctx = _ctx()
    ok = H.three_bars(40, 1, 1)
    for fn in (_host, _dev):
        rc, msg, _ = fn(ctx, ok, 2.0, None, 1.0, 68.34, n_bars=0)
        assert rc == _ffi.E_ARG and "non-empty" in msg, (rc, msg)
    with pytest.raises(AssertionError):
        volume_profile_rolling_csr(*(a[:0] for a in ok[:3]), np.zeros(1, np.int64), *(a[:0] for a in ok[4:]), 2.0, None, 1.0)
    for which in ("nan_low", "nan_high", "nan_all", "nan_all.empty_bars"):
        ts, hi, lo, off, lv, bv, sv = H.REFUSALS[which]["inputs"]
        with pytest.raises(ValueError, match="NaN"):
            aggregate_footprint(ts, hi, lo, lv, bv, sv, int(ts[4]), int(ts[6]), 1.0, level_offsets=off)
        got = aggregate_footprint(ts, hi, lo, lv, bv, sv, int(ts[0]), int(ts[3]), 1.0, level_offsets=off)   # bars 0 .. 3 hold no NaN
        for a, b in zip(got, H.aggregate_footprint(ts, hi, lo, off, lv, bv, sv, int(ts[0]), int(ts[3]), 1.0)):
            H.same(a, b, which + ": window in front of the NaN")
    n = _compare(volume_profile_rolling_csr(*H.NAN_UNUSED, 2.0, None, 1.0), H.volume_profile_rolling(*H.NAN_UNUSED, 2.0, None, 1.0), "nan_unused")
    _counts.record("vp_edges/nan_rule", outputs_compared=n)
