"""The developing volume profile on the MI355X (csrc/fmk_volprofile_dev.hip) on the hand-built footprints of tests/_vpdev_ref.py: ranges
round the chunk lengths, the order of the float32 adds across snapshots, bars of 0 .. 200 levels, ranges of 1 .. 20 000 levels through
the three LDS capacities and the global-scratch mode, the trim and its rounding, the one-level rule, every bin rule, the walk's exits,
NaN and inf volumes, many ranges a call, and what is refused.  Every case runs under automatic chunking and under chunks forced to 1,
2, 7 and 64 bars; every output is compared with the restatement on dtype, shape and bits; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import _counts
from tests import _vp_ref as H
from tests import _vpdev_ref as D

pytestmark = pytest.mark.gpu

KEYS = ("ts", "poc", "hva", "lva")
I32_SENTINEL = 0x5A5A5A5A


def _ctx():
    from finmlkit_amd import _ffi
    return _ffi.default_context()


def _compare(got, want, what):
    for k, a, b in zip(KEYS, got, want):
        H.same(a, b, f"{what}:{k}")
    return 3 * len(want[1])


# ---------------------------------------------------------------------------------------------- every case, CSR entry, every chunk length
@pytest.mark.parametrize("group", D.GROUPS)
def test_every_case_csr_under_every_chunk_length(group):
    from finmlkit_amd.feature.core.volume import volume_profile_developing_csr
    n = 0
    classes = set()
    assert len(D.CHUNKS) >= 4 and D.CHUNKS[0] == 0
    for name in D.group(group):
        want, info = D.expected(name)
        classes.add(D.capacity_class(max(info["L"])))
        for (a, b), w in zip(D.stamps(name), want):
            for cb in D.CHUNKS:
                n += _compare(volume_profile_developing_csr(*D.inputs(name), a, b, *D.params(name), chunk_bars=cb), w, f"{name} chunk_bars {cb}")
    if group == "levels":                                        # all three LDS capacities and the scratch mode were used
        assert classes == {1024, 4096, 8192, "scratch"}
    _counts.record(f"vpdev/csr/{group}", cases=len(D.group(group)), chunk_lengths=len(D.CHUNKS), outputs_compared=n)


# ---------------------------------------------------------------------------------------------- the other entries
SAMPLE = ("chunk.n15", "chunk.n129", "feeder.b3", "bar_widths.b27.k2", "empties.raw.k1", "levels.1025.b27", "levels.8193.raw", "trim.by_one.5",
          "trim.round_to_zero.2", "one_level.several.b3", "bins.r20.5", "walk.sym_long.va150.0", "special.nan.middle.2", "ranges.start5",
          "ranges.overlapping", "ranges.fifty", "ranges.duplicate_stamps", "half_tick.0.5.b3")


def test_ragged_signature():
    from finmlkit_amd.feature.core.volume import volume_profile_developing
    n = 0
    for name in SAMPLE:
        ts, hi, lo, off, lv, bv, sv = D.inputs(name)
        split = lambda a: [a[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        for (a, b), w in zip(D.stamps(name), D.expected(name)[0]):
            n += _compare(volume_profile_developing(ts, hi, lo, split(lv), split(bv), split(sv), a, b, *D.params(name)), w, name)
    _counts.record("vpdev/ragged", cases=len(SAMPLE), outputs_compared=n)


@pytest.mark.parametrize("chunk_bars", (0, 2))
def test_sessions_entry_equals_one_call_per_range(chunk_bars):
    from finmlkit_amd.feature.core.volume import volume_profile_developing_sessions_csr
    n = 0
    for name in SAMPLE:
        ts, hi, lo, off, lv, bv, sv = D.inputs(name)
        r = D.bar_ranges(name)
        out_off, poc, hva, lva = volume_profile_developing_sessions_csr(hi, lo, off, lv, bv, sv, [s for s, _ in r], [e for _, e in r], *D.params(name),
                                                                        chunk_bars=chunk_bars)
        H.same(out_off, np.concatenate([[0], np.cumsum([e - s for s, e in r])]).astype(np.int64), name + ": out_offsets")
        for j, w in enumerate(D.expected(name)[0]):
            a, b = out_off[j], out_off[j + 1]
            n += _compare((w[0], poc[a:b], hva[a:b], lva[a:b]), w, f"{name} range {j}")
    _counts.record(f"vpdev/sessions/chunk{chunk_bars}", cases=len(SAMPLE), outputs_compared=n)


def test_volumepro_compute_developing():
    import pandas as pd
    from types import SimpleNamespace
    from finmlkit_amd.feature.core.volume import VolumePro
    name = "ranges.fifty"
    ts, hi, lo, off, lv, bv, sv = D.inputs(name)
    n_bins, tick, va = D.params(name)
    r = D.bar_ranges(name)
    tick = 0.25                                                 # prices are levels * tick; the level range comes from highs / lows over the tick
    bars = pd.DataFrame(dict(high=hi * tick, low=lo * tick))
    fp = SimpleNamespace(bar_timestamps=ts, level_offsets=off, flat=dict(price_levels=lv, buy_volumes=bv, sell_volumes=sv), price_tick=tick)
    vp = VolumePro(pd.Timedelta(seconds=60), n_bins=n_bins, va_pct=va)
    edges = [int(ts[s]) for s, _ in r] + [int(ts[-1]) + 1]
    got = vp.compute_developing(bars, fp, session_edges=edges)
    want = D.expected(name)[0]
    H.same(got[0], np.concatenate([w[0] for w in want]), "session rows")
    for j, k in enumerate(KEYS[1:], 1):
        H.same(got[j], np.concatenate([w[j] for w in want]) * tick, "session " + k)
    ragged = SimpleNamespace(bar_timestamps=ts, price_levels=[lv[off[i]:off[i + 1]] for i in range(len(ts))],
                             buy_volumes=[bv[off[i]:off[i + 1]] for i in range(len(ts))],
                             sell_volumes=[sv[off[i]:off[i + 1]] for i in range(len(ts))], price_tick=tick)
    one = vp.compute_developing(bars, ragged)                    # no edges: one session over everything
    whole = D.developing_range(hi, lo, off, lv, bv, sv, 0, len(ts), n_bins, 1.0, va)
    H.same(one[0], ts, "one session rows")
    for j in range(3):
        H.same(one[j + 1], whole[j] * tick, "one session " + KEYS[j + 1])
    _counts.record("vpdev/volumepro", outputs_compared=3 * (len(got[0]) + len(ts)))


# ---------------------------------------------------------------------------------------------- resident arrays, raw ABI
def _raw(ctx, fn, *a):
    from finmlkit_amd import _ffi
    rc = getattr(_ffi.lib(), fn)(ctx.handle, *a)
    return rc, _ffi.lib().fmk_last_error(ctx.handle).decode(errors="replace")


def _layout(ranges, pad):
    """Output offsets with `pad` unused elements in front of, between and behind the ranges."""
    offs, at = [], pad
    for s, e in ranges:
        offs.append(at)
        at += (e - s) + pad
    return np.array(offs, np.int64), at


def _args(data, ranges, offs, n_bins, tick, va, cb):
    from finmlkit_amd._ffi import ptr
    rs, re_ = np.array([s for s, _ in ranges], np.int64), np.array([e for _, e in ranges], np.int64)
    keep = (rs, re_, offs)
    return keep, (C.c_int64(len(data[0])), ptr(rs), ptr(re_), ptr(offs), C.c_int64(len(ranges)), C.c_int64(-1 if n_bins is None else n_bins),
                  C.c_double(tick), C.c_double(va), C.c_int64(cb))


def _dev(ctx, data, ranges, n_bins, tick, va, cb=0, pad=3):
    """fmk_volume_profile_developing_dev on resident arrays, every output prefilled with a sentinel -> (status, message, outputs, offsets)."""
    from finmlkit_amd._ffi import DeviceArray
    offs, n_out = _layout(ranges, pad)
    ins = [DeviceArray.from_host(ctx, a) for a in data[1:]]
    outs = [DeviceArray.from_host(ctx, np.full(n_out, I32_SENTINEL, np.int32)) for _ in range(3)]
    keep, a = _args(data, ranges, offs, n_bins, tick, va, cb)
    rc, msg = _raw(ctx, "fmk_volume_profile_developing_dev", *[d.p for d in ins], *a, *[o.p for o in outs])
    got = [o.to_host() for o in outs] if rc == 0 else None
    for d in ins + outs:
        d.free()
    return rc, msg, got, offs


def _host(ctx, data, ranges, n_bins, tick, va, cb=0, pad=3):
    from finmlkit_amd._ffi import ptr
    offs, n_out = _layout(ranges, pad)
    outs = [np.full(n_out, I32_SENTINEL, np.int32) for _ in range(3)]
    keep, a = _args(data, ranges, offs, n_bins, tick, va, cb)
    rc, msg = _raw(ctx, "fmk_volume_profile_developing", *[ptr(np.ascontiguousarray(x)) for x in data[1:]], *a, *[ptr(o) for o in outs],
                   C.c_int64(n_out))
    return rc, msg, outs, offs


def _check_slots(got, offs, ranges, want, what):
    """Every slot of every range holds the expected value, every other element still the sentinel."""
    n = 0
    for j in range(3):
        exp = np.full(len(got[j]), I32_SENTINEL, np.int32)
        for o, (s, e), w in zip(offs, ranges, want):
            exp[o:o + (e - s)] = w[j + 1]
        H.same(got[j], exp, f"{what}:{KEYS[j + 1]}")
        n += len(exp)
    return n


DEV = ("chunk.n1", "chunk.n8", "chunk.n129", "chunk.auto200.b27", "feeder.raw", "bar_widths.raw.k2", "empties.b5.k1", "levels.1.b27",
       "levels.4097.raw", "levels.20000.b27", "trim.down.5", "trim.nan_ends.2", "one_level.first.b1", "bincount.129.1000000.k2",
       "walk.all_zero.va68.34", "special.inf.last.2", "ranges.single_bar", "ranges.touching", "ranges.fifty")


@pytest.mark.parametrize("chunk_bars", (0, 7))
def test_resident_arrays_every_slot_written_and_nothing_beyond(chunk_bars):
    ctx = _ctx()
    n = 0
    for name in DEV:
        r = D.bar_ranges(name)
        for fn in (_dev, _host):
            rc, msg, got, offs = fn(ctx, D.inputs(name), r, *D.params(name), cb=chunk_bars)
            assert rc == 0, (name, fn.__name__, rc, msg)
            n += _check_slots(got, offs, r, D.expected(name)[0], f"{name} ({fn.__name__})")
    _counts.record(f"vpdev/dev/chunk{chunk_bars}", cases=len(DEV), outputs_compared=n)


# ---------------------------------------------------------------------------------------------- refusals
def _good(ctx):
    """A good call on the same context right after a refusal: the status words are cleared per call."""
    name = "bins.r20.5"
    for fn in (_host, _dev):
        rc, msg, got, offs = fn(ctx, D.inputs(name), D.bar_ranges(name), *D.params(name))
        assert rc == 0, (rc, msg)
        _check_slots(got, offs, D.bar_ranges(name), D.expected(name)[0], name + " after a refusal")


@pytest.mark.parametrize("name", sorted(D.REFUSALS))
def test_refusals(name):
    from finmlkit_amd import _ffi
    from finmlkit_amd.feature.core.volume import volume_profile_developing_csr
    ctx = _ctx()
    c = D.REFUSALS[name]
    for fn in (_host, _dev):
        rc, msg, _, _ = fn(ctx, c["inputs"], [c["span"]], c["n_bins"], c["tick"], c["va"])
        assert rc == getattr(_ffi, c["code"]) and c["message"] in msg, (name, fn.__name__, rc, msg)
        _good(ctx)
    with pytest.raises(c["error"], match=c["message"] if c["code"] != "E_ZERODIV" and not name.startswith("level_") else None):
        volume_profile_developing_csr(*c["inputs"], *D.refusal_stamps(c), c["n_bins"], c["tick"], c["va"])
    _counts.record(f"vpdev/refused/{name}", calls=3)


def test_first_all_zero_bar_is_named_and_what_is_not_refused():
    """Among several ranges the message names the lowest range, then the lowest bar, whatever the chunk length; a NaN low or high outside
    every range, and an all-zero first bar without bucketing, are not refused."""
    from finmlkit_amd import _ffi
    from finmlkit_amd.feature.core.volume import volume_profile_developing_csr, volume_profile_developing_sessions_csr
    ctx = _ctx()
    data = D.REFUSALS["all_zero_first_bar.bins"]["inputs"]     # bars 0 and 3 are empty
    for cb in (0, 1, 2):
        rc, msg, _, _ = _dev(ctx, data, [(1, 3), (3, 5), (0, 2)], 5, 1.0, 68.34, cb=cb)
        assert rc == _ffi.E_LEVEL and "range 1, bar 0 of the range" in msg, (cb, rc, msg)
    with pytest.raises(ValueError, match="range 2, bar 0 of the range"):
        volume_profile_developing_sessions_csr(*data[1:], [1, 2, 0], [3, 3, 2], 5, 1.0)
    with pytest.raises(AssertionError, match="non-empty"):
        volume_profile_developing_csr(*(a[:0] for a in data[:3]), np.zeros(1, np.int64), *(a[:0] for a in data[4:]), 0, 1, None, 1.0)
    n = 0
    for name, c in D.RETURNS.items():
        s, e = c["span"]
        ts = c["inputs"][0]
        want = (ts[s:e],) + D.developing_range(*c["inputs"][1:], s, e, c["n_bins"], c["tick"], c["va"])
        n += _compare(volume_profile_developing_csr(*c["inputs"], int(ts[s]), int(ts[e - 1]), c["n_bins"], c["tick"], c["va"]), want, name)
    _counts.record("vpdev/returns", outputs_compared=n)
