"""Plain sequential restatement of the reference's rolling volume profile -- aggregate_footprint, bucket_price_levels,
comp_poc_hva_lva, calc_volume_percentage_above_poc and volume_profile_rolling (feature/core/volume.py:134-456) -- on CSR footprints,
in the typed semantics that include/fmk.h states as the contract, with builders of hand-made footprints and the table of edge cases
that tools/gen_vp_edges_golden.py, tests/test_vp_host.py and tests/test_gpu_vp_edges.py share.

  window        searchsorted left of end - window, right of end; an empty window falls back on the bar in front
  level range   int(round(x / tick)) of min(lows), max(highs): Python's round, half to even; a NaN low or high in the window makes
                the minimum or maximum NaN and the conversion raises ValueError (an infinite one OverflowError)
  aggregation   bars one after another, per level `np.float32 +=`; a level outside [min, max] is refused (LevelError)
  total volume  buy + sell in float32
  bins          width max(1, range // n_bins) made odd, edges from the minimum in steps of the width up to max + width (exclusive),
                float32 sums in level order, a leftover bin (priced at the maximum) iff the LAST level falls past the bins;
                a one-level profile cannot be bucketed (ValueError, as the reference's broadcast error)
  total         np.sum of the float32 array (NumPy's pairwise sum)
  POC           np.argmax: the first maximum, the first NaN wins
  walk          Python floats (float64): threshold float(total) * (va_pct / 100.0), two levels a step, `-1.0` for an exhausted side
  share         float64 running sum over the levels above the POC, float64 quotient, stored as float32
Reads nothing outside the repository."""
import functools
import hashlib
import math

import numpy as np

ONE_LEVEL_MESSAGE = "a one-level profile cannot be bucketed"
LEVEL_MESSAGE = "footprint level outside its window"

LDS_CAPS = (1024, 4096, 8192)            # levels a wave's histogram holds in LDS; 4 waves per workgroup at the first, else one
MAX_LEVELS = 1 << 24                     # above: refused with the capacity error


class LevelError(ValueError):
    """A footprint level outside its window's level range (the reference raises IndexError above the range and folds a level
    below it onto the lowest one; include/fmk.h refuses both)."""


# ====================================================================================================== the restatement
def level_of(x, tick):
    return int(round(float(x) / float(tick)))


def window_of(ts, start_ts, end_ts):
    s = int(np.searchsorted(ts, start_ts, side="left"))
    e = int(np.searchsorted(ts, end_ts, side="right"))
    if s == e:
        s = max(0, s - 1)
    return s, e


def aggregate_footprint(ts, highs, lows, off, levels, buy, sell, start_ts, end_ts, tick):
    """-> (complete levels int32, buy float32, sell float32) of the bars in [start_ts, end_ts]."""
    s, e = window_of(ts, start_ts, end_ts)
    lo, hi = np.min(lows[s:e]), np.max(highs[s:e])               # NaN propagates; an empty window raises ValueError
    minl, maxl = level_of(lo, tick), level_of(hi, tick)
    n = max(0, maxl - minl + 1)
    ab, as_ = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(s, e):
        r0, r1 = int(off[t]), int(off[t + 1])
        if r0 == r1:
            continue
        idx = levels[r0:r1].astype(np.int64) - minl
        if idx.min() < 0 or idx.max() >= n:
            raise LevelError(LEVEL_MESSAGE)
        ab[idx] += buy[r0:r1]                                    # a bar's levels are distinct: one float32 add per level
        as_[idx] += sell[r0:r1]
    return np.arange(minl, minl + n, dtype=np.int32), ab, as_


def bin_layout(mn, mx, n_bins):
    """-> (width, full bins): the odd width and the number of bins the edges mn, mn + width, ... < mx + width enclose."""
    rng = int(mx) - int(mn)
    width = max(1, rng // int(n_bins))                           # n_bins == 0: ZeroDivisionError
    if width % 2 == 0:
        width += 1
    n_edges = len(range(int(mn), int(mx) + width, width))
    return width, n_edges - 1


def bucket_price_levels(levels, volumes, n_bins):
    levels = np.asarray(levels)
    mn, mx = int(np.min(levels)), int(np.max(levels))
    width, nb = bin_layout(mn, mx, n_bins)
    if nb < 1:
        raise ValueError(ONE_LEVEL_MESSAGE)
    which = np.minimum((levels.astype(np.int64) - mn) // width, nb)   # edges at or below the level, less one
    leftover = int(which[-1]) == nb
    out_v = np.zeros(nb + leftover, np.float32)
    out_l = np.zeros(nb + leftover, np.int32)
    for k in range(nb):
        e0 = mn + k * width
        out_l[k] = (e0 + e0 + width - 1) // 2
    if leftover:
        out_l[nb] = mx
    elif int(which.max()) == nb:
        raise IndexError("a level past the last bin in front of the last element")
    for k in range(nb + leftover):                                # every bin's elements in element order
        sel = volumes[which == k]
        if len(sel):
            out_v[k] = np.cumsum(sel, dtype=np.float32)[-1]      # float32 adds one after another (0.0 + the first is the first)
    return out_l, out_v


def _pair(v, i, step, n):
    """The volume of levels i and i + step, -1.0 when i is outside."""
    if not 0 <= i < n:
        return -1.0
    x = float(v[i])
    if 0 <= i + step < n:
        x += float(v[i + step])
    return x


def comp_poc_hva_lva(levels, volumes, va_pct=68.34, trace=None):
    """-> (poc, hva, lva) as ints.  `trace`: a list that receives (cum, threshold) at every test of the loop's condition."""
    n = len(levels)
    total = np.sum(volumes)
    pi = int(np.argmax(volumes))
    poc = int(levels[pi])
    thr = float(total) * (va_pct / 100.0)
    cum = float(volumes[pi])
    hva = lva = poc
    up, down = pi + 1, pi - 1
    cu = cd = 0.0
    if up < n:
        cu = _pair(volumes, up, 1, n)
    if down >= 0:
        cd = _pair(volumes, down, -1, n)
    while True:
        if trace is not None:
            trace.append((cum, thr))
        if not cum < thr:
            break
        if cu > cd:
            cum += cu
            hva = int(levels[min(up + 1, n - 1)])
            up += 2
            cu = _pair(volumes, up, 1, n)
        elif cu < cd:
            cum += cd
            lva = int(levels[max(down - 1, 0)])
            down -= 2
            cd = _pair(volumes, down, -1, n)
        elif cu == cd and cd != -1.0:
            cum += cu + cd
            hva = int(levels[min(up + 1, n - 1)])
            lva = int(levels[max(down - 1, 0)])
            up += 2
            down -= 2
            cu = _pair(volumes, up, 1, n)
            cd = _pair(volumes, down, -1, n)
        else:
            break
    return poc, hva, lva


def calc_volume_percentage_above_poc(levels, volumes, poc):
    total = np.sum(volumes)
    if total <= 0:
        return 0.0
    sel = np.asarray(volumes)[np.asarray(levels) > poc].astype(np.float64)
    above = float(np.cumsum(sel)[-1]) if len(sel) else 0.0      # cumsum adds one after another, from 0.0 + the first
    if above <= 0.0:
        return 0.0
    return above / float(total)


def first_bar(ts, window_size_sec):
    return int(np.searchsorted(ts, ts[0] + int(window_size_sec * 1e9)))


def volume_profile_rolling(ts, highs, lows, off, levels, buy, sell, window_size_sec, n_bins=None, price_tick=None, va_pct=68.34,
                           info=None):
    """-> (poc, hva, lva int32, share float32).  `info`: a dict that receives first, and per computed bar s, e and the levels."""
    nb = len(ts)
    if not (nb == len(highs) == len(lows) == len(off) - 1) or nb == 0:
        raise AssertionError("Input arrays should have the same length and be non-empty.")
    if not price_tick > 0:
        raise ValueError("price_tick must be > 0")
    poc, hva, lva = (np.zeros(nb, np.int32) for _ in range(3))
    pct = np.zeros(nb, np.float32)
    window_ns = int(window_size_sec * 1e9)
    first = first_bar(ts, window_size_sec)
    if info is not None:
        info.update(first=first, s=[], e=[], L=[])
    for i in range(first, nb):
        end_ts = int(ts[i])
        lv, ab, as_ = aggregate_footprint(ts, highs, lows, off, levels, buy, sell, end_ts - window_ns, end_ts, price_tick)
        if info is not None:
            s, e = window_of(ts, end_ts - window_ns, end_ts)
            info["s"].append(s), info["e"].append(e), info["L"].append(len(lv))
        if len(lv) < 1:
            raise LevelError(LEVEL_MESSAGE)                      # high below low: no level range
        tot = ab + as_
        if n_bins is not None:
            lv, tot = bucket_price_levels(lv, tot, n_bins)
        poc[i], hva[i], lva[i] = comp_poc_hva_lva(lv, tot, va_pct)
        pct[i] = calc_volume_percentage_above_poc(lv, tot, int(poc[i]))
    return poc, hva, lva, pct


def capacity_class(max_levels):
    """What the widest window of a call selects: 1024, 4096 or 8192 levels in LDS, "scratch" above, "refused" above 1 << 24."""
    if max_levels > MAX_LEVELS:
        return "refused"
    for c in LDS_CAPS:
        if max_levels <= c:
            return c
    return "scratch"


def waves_per_launch(cls, n_cu):
    """The most waves one launch has: n_cu * 32 workgroups of 4 waves (1024 levels) or one, n_cu * 8 of one in the scratch mode."""
    return n_cu * 32 * 4 if cls == 1024 else n_cu * 8 if cls == "scratch" else n_cu * 32


# ====================================================================================================== builders
def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def volumes(rng, n, kind):
    """kind 1: multiples of 2**-4 below 16 (every float32 sum on the way is exact); kind 2 and 3: lognormal float32."""
    if kind == 1:
        return (rng.integers(0, 256, n) / 16.0).astype(np.float32)
    return rng.lognormal(0.0, 1.5, n).astype(np.float32)


def csr(bar_ts, low_levels, high_levels, bar_levels, bar_buy, bar_sell, tick=1.0):
    """-> (ts, highs, lows, off, levels, buy, sell): prices are level * tick."""
    nb = len(bar_ts)
    off = np.zeros(nb + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in bar_levels])
    cat = lambda parts, dt: (np.concatenate([np.asarray(p, dtype=dt) for p in parts]) if off[-1] else np.empty(0, dt)).astype(dt)
    return (np.asarray(bar_ts, np.int64), np.asarray(high_levels, np.float64) * tick, np.asarray(low_levels, np.float64) * tick, off,
            cat(bar_levels, np.int32), cat(bar_buy, np.float32), cat(bar_sell, np.float32))


def regular_ts(n, step_s=1):
    return 1_700_000_000_000_000_000 + np.arange(n, dtype=np.int64) * (step_s * 1_000_000_000)


def bars_from_counts(seed, counts, kind, ts=None, tick=1.0, base=1000, wander=6):
    """One bar per entry of `counts` with that many ascending distinct levels between its low and high (which wander round `base`
    and leave one or two levels unused)."""
    rng = np.random.default_rng(seed)
    lo_l, hi_l, lv, bv, sv = [], [], [], [], []
    for c in counts:
        lo = base + int(rng.integers(-wander, wander + 1))
        hi = lo + max(c, 1) - 1 + int(rng.integers(1, 3))
        lo_l.append(lo), hi_l.append(hi)
        lv.append(np.sort(rng.choice(np.arange(lo, hi + 1), size=c, replace=False)))
        bv.append(volumes(rng, c, kind)), sv.append(volumes(rng, c, kind))
    return csr(regular_ts(len(counts)) if ts is None else ts, lo_l, hi_l, lv, bv, sv, tick)


def window_length(k, kind, seed):
    """Regular 1 s stamps, k + 6 bars of 1 .. 5 levels: with a window of k - 1 seconds every window from bar k - 1 on holds k bars."""
    rng = np.random.default_rng(seed)
    return bars_from_counts(seed + 1, rng.integers(1, 6, k + 6), kind)


def chunk_empties(kind, seed):
    """140 bars, windows of 130: empty bars at the first, an interior and the last place of a 63-bar chunk, sliding through them."""
    counts = np.random.default_rng(seed).integers(1, 5, 140)
    counts[[0, 10, 11, 30, 62, 63, 72, 73, 125, 126, 129, 139]] = 0
    return bars_from_counts(seed + 1, counts, kind)


def feeder(kind, seed):
    """200 bars that all feed level 1000 with 1e8 and 1 in turn (another order of the float32 adds gives other bits) beside
    a few levels of their own."""
    d = list(bars_from_counts(seed, np.full(200, 3), 2, wander=0))
    ts, hi, lo, off, lv, bv, sv = d
    for t in range(200):
        r = int(off[t])
        lv[r] = 1000                                             # the bar's lowest level (wander 0: its low)
        bv[r] = 1e8 if t % 2 == 0 else 1.0
        sv[r] = 1.0 if t % 3 else 3e7
    assert all(np.all(np.diff(lv[off[t]:off[t + 1]]) > 0) for t in range(200))
    return tuple(d)


def placement(which, kind, seed):
    rng = np.random.default_rng(seed)
    n = 40
    if which == "gaps":                                          # windows of 5 s over gaps of 1 .. 20 s: some hold one bar
        ts = regular_ts(1)[0] + np.cumsum(rng.choice([1, 2, 3, 7, 20], n)).astype(np.int64) * 1_000_000_000
    elif which == "edge":                                        # gaps of 2 and 3 s, window 5 s: a bar exactly at end - window
        ts = regular_ts(1)[0] + np.cumsum(np.tile([2, 3], n // 2)).astype(np.int64) * 1_000_000_000
    elif which == "dup":                                         # every stamp three times
        ts = np.repeat(regular_ts(n // 3 + 1), 3)[:n]
    else:
        ts = regular_ts(n)
    return bars_from_counts(seed + 1, rng.integers(0, 5, n), kind, ts=ts)


def three_bars(n_levels, kind, seed, base=-40, tick=1.0, lone=5):
    """Three bars in one window of `n_levels` levels that highs and lows alone set: the first bar holds the lowest level, the second
    the highest, the third up to `lone` levels between."""
    rng = np.random.default_rng(seed)
    lo, hi = base, base + n_levels - 1
    mid = np.unique(rng.integers(lo, hi + 1, min(lone, n_levels)))
    lv = [np.array([lo]), np.array([hi]), mid]
    return csr(regular_ts(3), [lo, hi, lo], [lo, hi, hi], lv, [volumes(rng, len(a), kind) for a in lv],
               [volumes(rng, len(a), kind) for a in lv], tick)


def one_wide(wide, kind, seed):
    """12 bars of 5 levels, windows of two bars; bar 5 alone spans `wide` levels (volume at both ends and in the middle)."""
    rng = np.random.default_rng(seed)
    lo = [1000] * 12
    hi = [1004] * 12
    lv = [np.sort(rng.choice(np.arange(1000, 1005), 3, replace=False)) for _ in range(12)]
    hi[5] = 1000 + wide - 1
    lv[5] = np.array([1000, 1003, 1000 + wide // 2, 1000 + wide - 1])
    return csr(regular_ts(12), lo, hi, lv, [volumes(rng, len(a), kind) for a in lv], [volumes(rng, len(a), kind) for a in lv])


def bar_widths(kind, seed):
    """Levels per bar through 0, 1, 63, 64, 65, 127, 128, 129 and 200, each wide bar between narrow ones; windows of 3 bars."""
    return bars_from_counts(seed, [1, 200, 1, 0, 63, 2, 64, 0, 65, 1, 127, 3, 128, 1, 129, 0, 200, 200, 1, 64, 64, 2], kind)


def profile(total, seed=0, levels_base=500, split=True):
    """ONE bar in one window whose aggregated total volumes are `total` exactly (entries: multiples of 2**-3, NaN or inf): buy
    takes the part rounded down to a multiple of a half, sell the rest, or buy takes all (split=False)."""
    v = np.asarray(total, np.float32)
    n = len(v)
    with np.errstate(invalid="ignore"):
        b = np.where(np.isfinite(v) & split, np.floor(v) / 2, v).astype(np.float32)
        s = np.where(np.isfinite(v) & split, v - b, 0).astype(np.float32)
    lv = np.arange(levels_base, levels_base + n)
    return csr(regular_ts(1), [levels_base], [levels_base + n - 1], [lv], [b], [s])


def half_ticks(tick, kind, seed):
    """Lows and highs at k + 0.5 ticks for even and odd k (the quotient is exact: a true tie, rounded to even), windows of one bar and
    of three; every bar holds its own lowest and highest level."""
    rng = np.random.default_rng(seed)
    ks = [(10, 13), (11, 14), (-4, 1), (-3, 2), (-1, 0), (21, 22), (20, 23), (0, 5)]
    lows = np.array([(a + 0.5) * tick for a, _ in ks])
    highs = np.array([(b + 0.5) * tick for _, b in ks])
    assert all(float(x) / tick - math.floor(float(x) / tick) == 0.5 for x in np.concatenate([lows, highs]))
    lv = [np.arange(level_of(lo, tick), level_of(hi, tick) + 1) for lo, hi in zip(lows, highs)]
    ts, _, _, off, l, b, s = csr(regular_ts(len(ks), 10), [0] * len(ks), [0] * len(ks), lv, [volumes(rng, len(a), kind) for a in lv],
                                [volumes(rng, len(a), kind) for a in lv])
    return ts, highs, lows, off, l, b, s


def near_half_cent(kind, seed):
    """Tick 0.01: prices whose quotient by the tick lands one unit in the last place below and above k + 0.5."""
    rng = np.random.default_rng(seed)
    tick, lows, highs = 0.01, [], []
    for k, side in ((1203, -1), (1210, +1), (1204, +1), (1211, -1), (1207, -1), (1215, -1), (1206, +1), (1214, +1)):
        x = (k + 0.5) * tick
        for _ in range(64):                                      # walk to the first price whose quotient is on the wanted side
            q = x / tick
            if (side < 0 and q < k + 0.5) or (side > 0 and q > k + 0.5):
                break
            x = math.nextafter(x, side * math.inf)
        assert abs(x / tick - (k + 0.5)) <= 2 * math.ulp(k + 0.5) and x / tick != k + 0.5
        (lows if len(lows) == len(highs) else highs).append(x)
    lows, highs = np.array(lows), np.array(highs)
    lv = [np.arange(level_of(lo, tick), level_of(hi, tick) + 1) for lo, hi in zip(lows, highs)]
    ts, _, _, off, l, b, s = csr(regular_ts(4, 10), [0] * 4, [0] * 4, lv, [volumes(rng, len(a), kind) for a in lv],
                                [volumes(rng, len(a), kind) for a in lv])
    return ts, highs, lows, off, l, b, s


def reuse(n_waves, wide, n_extra=24, narrow=5):
    """More bars than a launch has waves, one or two levels a bar, windows of two bars: bars 2 and 6 span `wide` levels with volume
    at the top, so the windows of bars 2, 3, 6, 7 are wide and the waves that served them meet the narrow windows of bars
    2 + n_waves ...; bar n_waves + 12 is wide again, in a slice that a narrow window used."""
    n = n_waves + n_extra
    rng = np.random.default_rng(n_waves * 31 + wide)
    lo = np.full(n, 1000)
    hi = np.full(n, 1000 + narrow - 1)
    first = 1000 + rng.integers(0, narrow, n)
    lv = [np.array([a]) for a in first]
    for j in (2, 6, n_waves + 12):
        hi[j] = 1000 + wide - 1
        lv[j] = np.array([1001, 1000 + wide - 1])
    b = [(rng.integers(1, 256, len(a)) / 16.0) for a in lv]
    s = [(rng.integers(0, 256, len(a)) / 16.0) for a in lv]
    return csr(regular_ts(n), lo, hi, lv, b, s)


def plant(data, row, value, sell=False):
    d = [a.copy() for a in data]
    d[6 if sell else 5][row] = value
    return tuple(d)


BUILDERS = dict(window_length=window_length, chunk_empties=chunk_empties, feeder=feeder, placement=placement, three_bars=three_bars,
                one_wide=one_wide, bar_widths=bar_widths, profile=profile, half_ticks=half_ticks, near_half_cent=near_half_cent)


# ====================================================================================================== the case table
# name -> dict(build=(builder, kwargs), window=seconds, n_bins, tick, va, kind, one=True where the call computes ONE window from
# ONE bar range [0, n_bars) (the stage functions then run on it), plant=[(row, value, sell)])
CASES = {}


def _case(name, builder, kwargs, window, n_bins=None, tick=1.0, va=68.34, kind=1, one=False, plants=()):
    assert name not in CASES, name
    CASES[name] = dict(build=(builder, dict(kwargs)), window=float(window), n_bins=n_bins, tick=tick, va=va, kind=kind, one=one,
                       plants=tuple(plants))


def _table():
    # ---- window length in bars: the 63-bar chunks of the offsets
    for k in (1, 2, 62, 63, 64, 65, 125, 126, 127, 190):
        for kind in (1, 2):
            _case(f"winlen.{k}.k{kind}", "window_length", dict(k=k, kind=kind, seed=100 + k), k - 1, None if k % 2 else 5, kind=kind)
    for kind in (1, 2):
        _case(f"chunk_empties.k{kind}", "chunk_empties", dict(kind=kind, seed=7), 129, 5, kind=kind)
        _case(f"bar_widths.k{kind}", "bar_widths", dict(kind=kind, seed=9), 2, 27, kind=kind)
        _case(f"bar_widths.w0.k{kind}", "bar_widths", dict(kind=kind, seed=10), 0, None, kind=kind)
    _case("feeder.w190", "feeder", dict(kind=2, seed=3), 189, None, kind=2)
    _case("feeder.w64.b3", "feeder", dict(kind=2, seed=4), 63, 3, kind=2)
    # ---- window placement
    for which, window in (("gaps", 5), ("edge", 5), ("dup", 2), ("dup", 0), ("regular", 0), ("regular", 100), ("regular", 39)):
        for kind in (1, 2):
            _case(f"place.{which}.w{window}.k{kind}", "placement", dict(which=which, kind=kind, seed=20 + window), window,
                  None if kind == 1 else 3, kind=kind)
    # ---- levels per window, sparsely populated
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 20_000):
        _case(f"levels.{n}.raw", "three_bars", dict(n_levels=n, kind=1, seed=n), 2, None, one=True)
        if n > 1:
            _case(f"levels.{n}.b27", "three_bars", dict(n_levels=n, kind=1, seed=n + 1), 2, 27, one=True)
            _case(f"levels.{n}.b27.k2", "three_bars", dict(n_levels=n, kind=2, seed=n + 2, lone=40), 2, 27, kind=2, one=True)
    for wide in (1025, 8193):
        for nb in (None, 5):
            _case(f"one_wide.{wide}.{'raw' if nb is None else 'b5'}", "one_wide", dict(wide=wide, kind=1, seed=wide), 1, nb)
    # ---- tick rounding
    for tick in (1.0, 0.5, 0.25):
        for window in (0, 20):
            _case(f"half_tick.{tick}.w{window}", "half_ticks", dict(tick=tick, kind=1, seed=5), window, 3 if window else None, tick=tick)
    _case("near_half_cent.w0", "near_half_cent", dict(kind=1, seed=6), 0, None, tick=0.01)
    _case("near_half_cent.w10.b2", "near_half_cent", dict(kind=1, seed=6), 10, 2, tick=0.01)
    # ---- bins: widths raised from 0, 2 and 4, odd already, dividing the range or not; one lane per bin in strides of 64
    for rng_ in (1, 4, 10, 15, 16, 20, 26, 199, 200):
        for nb in dict.fromkeys((None, 1, 2, 3, 5, 27, 200, rng_, rng_ + 1, 10 ** 6)):
            _case(f"bins.r{rng_}.{nb}", "three_bars", dict(n_levels=rng_ + 1, kind=1, seed=rng_, lone=40), 2, nb, one=True)
    for n, nb in ((63, 10 ** 6), (64, 10 ** 6), (65, 10 ** 6), (129, 10 ** 6), (193, 64), (190, 63), (385, 128)):
        for kind in (1, 2):
            _case(f"bincount.{n}.{nb}.k{kind}", "three_bars", dict(n_levels=n, kind=kind, seed=n, lone=300), 2, nb, kind=kind, one=True)
    # ---- POC and the walk, the share above the POC: explicit profiles
    one = np.ones
    z = np.zeros
    def spike(n, at, v=7.0, fill=1.0):
        a = np.full(n, fill)
        a[list(at)] = v
        return a
    profiles = {
        "poc_first": [9, 1, 2, 3, 1], "poc_last": [1, 2, 3, 1, 9], "one_level": [5], "two_levels": [2, 2],
        "max_10_74": spike(100, (10, 74)), "max_63_64": spike(130, (63, 64)), "max_three": spike(150, (10, 74, 138)),
        "max_64_0_fill0": spike(130, (64, 128), fill=0.0), "all_zero": z(9), "sym": [1, 2, 9, 2, 1], "sym_long": [0, 0, 3, 3, 9, 3, 3, 0, 0],
        "zeros_both": [5, 5, 0, 0, 0, 0, 9, 0, 0, 0, 0, 5, 5], "zeros_up": [5, 5, 1, 1, 9, 0, 0, 0, 0, 0, 0],
        "zeros_down": [0, 0, 0, 0, 0, 9, 1, 1, 5, 5], "zeros_unequal": [4, 0, 0, 9, 0, 0, 0, 0, 0, 0, 4, 4],
        "up_short": [1, 1, 1, 1, 1, 1, 1, 9, 2], "down_short": [2, 9, 1, 1, 1, 1, 1, 1, 1], "up_odd": [1, 1, 9, 5], "down_odd": [5, 9, 1, 1],
        "exact8": [0, 0, 4, 1, 1, 2], "exact16": [1, 1, 2, 8, 2, 1, 1], "exact64": [4, 4, 8, 32, 8, 4, 2, 2],
        "ones_4096": one(4096), "ones_8192": one(8192), "top_heavy": [3, 2, 2, 2, 2, 2, 2, 2],
        "ramp_up": np.arange(1, 70) / 8.0, "ramp_down": np.arange(70, 1, -1) / 8.0,
    }
    for pname, vols in profiles.items():
        for va in ((0.0, 25.0, 50.0, 68.34, 75.0, 100.0, 150.0) if len(vols) < 200 else (68.34, 100.0)):
            _case(f"walk.{pname}.va{va}", "profile", dict(total=[float(x) for x in vols], split=pname not in ("ones_4096", "ones_8192")), 0,
                  None, va=va, one=True)
        if len(vols) > 1:
            for nb in (2, 3):
                _case(f"walk.{pname}.b{nb}", "profile", dict(total=[float(x) for x in vols]), 0, nb, one=True)
    # ---- NaN and +inf in one level's volume (kind 3)
    nan, inf = math.nan, math.inf
    special = {
        "nan_mid": [1, 2, nan, 9, 1], "nan_first": [nan, 2, 3], "nan_last": [1, 2, nan], "nan_two": [1, nan, 5, nan, 2],
        "nan_70_of_140": [nan if i in (70, 133) else (i % 7) / 2 for i in range(140)], "nan_after_max": [9, 1, nan],
        "inf_max": [1, 2, inf, 9, 1], "inf_first": [inf, 1, 1], "inf_two": [1, inf, 3, inf], "inf_and_nan": [1, inf, 3, nan, 2],
    }
    for pname, vols in special.items():
        for va in (0.0, 68.34, 100.0):
            _case(f"special.{pname}.va{va}", "profile", dict(total=[float(x) for x in vols], split=False), 0, None, va=va, kind=3, one=True)
        _case(f"special.{pname}.b2", "profile", dict(total=[float(x) for x in vols], split=False), 0, 2, kind=3, one=True)
    for k in (2, 64, 190):                                       # one NaN / inf planted in a rolling call: every window from its bar on
        _case(f"special.roll_nan.{k}", "window_length", dict(k=k, kind=2, seed=300 + k), k - 1, None, kind=3, plants=[(7, nan, False)])
        _case(f"special.roll_inf.{k}", "window_length", dict(k=k, kind=2, seed=400 + k), k - 1, 5, kind=3, plants=[(9, inf, True)])


_table()


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASES[name]
    d = BUILDERS[c["build"][0]](**c["build"][1])
    for row, value, sell in c["plants"]:
        d = plant(d, row, value, sell)
    for a in d:
        a.setflags(write=False)
    return d


def input_hash(name):
    c = CASES[name]
    return sha256(*inputs(name), np.array([c["window"], -1.0 if c["n_bins"] is None else c["n_bins"], c["tick"], c["va"]]))


def args(name):
    c = CASES[name]
    return inputs(name) + (c["window"], c["n_bins"], c["tick"], c["va"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's outputs and the window facts of a case (computed once, shared, read-only)."""
    info = {}
    out = volume_profile_rolling(*args(name), info=info)
    for a in out:
        a.setflags(write=False)
    return out, info


def names(kind=None, one=None):
    return [n for n, c in CASES.items() if (kind is None or c["kind"] == kind) and (one is None or c["one"] == one)]


def same(got, want, what):
    """dtype, shape and bits equal, NaN at the same places."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        ok = np.isnan(want) | (got.view(np.uint32 if got.itemsize == 4 else np.uint64) == want.view(np.uint32 if want.itemsize == 4 else np.uint64))
        assert ok.all(), (what, np.flatnonzero(~ok)[:5], got[~ok][:5], want[~ok][:5])
    else:
        assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:5], got[got != want][:5], want[got != want][:5])


def stage_outputs(mod, data, n_bins, tick, va, as_lists=None):
    """The stage functions of `mod` chained on the one window [ts[0], ts[-1]] -> [levels, buy, sell, (bin levels, bin volumes,)
    (poc, hva, lva) int64, share as float32 (as the rolling call stores it)].  `as_lists`: turns (off, flat array) into the
    per-bar lists the reference's signature takes; without it `mod` takes the restatement's CSR arguments."""
    ts, hi, lo, off, lv, bv, sv = data
    if as_lists is not None:
        a = mod.aggregate_footprint(ts, hi, lo, as_lists(off, lv), as_lists(off, bv), as_lists(off, sv), int(ts[0]), int(ts[-1]), tick)
    else:
        a = mod.aggregate_footprint(ts, hi, lo, off, lv, bv, sv, int(ts[0]), int(ts[-1]), tick)
    levels, tot = a[0], a[1] + a[2]
    out = list(a)
    if n_bins is not None:
        levels, tot = mod.bucket_price_levels(levels, tot, n_bins)
        out += [levels, tot]
    p = mod.comp_poc_hva_lva(levels, tot, va)
    out.append(np.array([int(x) for x in p], np.int64))
    out.append(np.array([mod.calc_volume_percentage_above_poc(levels, tot, p[0])], np.float32))
    return [np.asarray(x) for x in out]


def stages_hash(outs):
    """sha256 of stage outputs, every NaN made one value."""
    return sha256(*[np.where(np.isnan(x), x.dtype.type(-12345.0), x) if x.dtype.kind == "f" else x for x in outs])


# ====================================================================================================== refused calls
# name -> dict(inputs, window, n_bins, tick, va, error=the exception the Python entry raises, code=the C status name,
# message=a part of fmk_last_error).  The reference's own behaviour on each is recorded in tests/golden/vp_edges.json.
def _bad_level(pos, value):
    """Three bars in one window of levels 1000 .. 1131; the middle bar has 130 levels, the one at `pos` replaced by `value`."""
    rng = np.random.default_rng(pos)
    lv = [np.array([1000]), np.arange(1001, 1131), np.array([1005, 1131])]
    lv[1][pos] = value
    return csr(regular_ts(3), [1000] * 3, [1131] * 3, lv, [volumes(rng, len(a), 1) for a in lv], [volumes(rng, len(a), 1) for a in lv])


def _with_nan(which):
    """Ten bars of three levels, windows of three bars: the low of bar 5, its high, or every low and high from bar 4 on is NaN."""
    d = [a.copy() for a in bars_from_counts(77, [3] * 10, 1)]
    if which == "low":
        d[2][5] = math.nan
    elif which == "high":
        d[1][5] = math.nan
    elif which == "unused":                                      # 100 s between bars 0 and 1, windows of 2 s: no window holds bar 0
        d[0][1:] += 100_000_000_000
        d[2][0] = math.nan
    else:
        d[1][4:] = math.nan
        d[2][4:] = math.nan
    return tuple(d)


NAN_MESSAGE = "NaN"
REFUSALS = {}


def _refusals():
    def add(name, data, window, n_bins, tick, error, code, message, va=68.34):
        REFUSALS[name] = dict(inputs=data, window=float(window), n_bins=n_bins, tick=tick, va=va, error=error, code=code, message=message)
    for where, pos in (("first64", 10), ("rest", 100)):
        add(f"level_below.{where}", _bad_level(pos, 999), 2, None, 1.0, ValueError, "E_LEVEL", "level outside")
        add(f"level_above.{where}", _bad_level(pos, 1132), 2, 5, 1.0, ValueError, "E_LEVEL", "level outside")
    ok = three_bars(40, 1, 1)
    add("n_bins_0", ok, 2, 0, 1.0, ZeroDivisionError, "E_ZERODIV", "division")
    add("tick_0", ok, 2, None, 0.0, ValueError, "E_ARG", "price_tick")
    add("tick_negative", ok, 2, None, -1.0, ValueError, "E_ARG", "price_tick")
    add("tick_nan", ok, 2, None, math.nan, ValueError, "E_ARG", "price_tick")
    add("one_level_bins", three_bars(1, 1, 1), 2, 27, 1.0, ValueError, "E_LEVEL", "single price level")
    lv = [np.array([1000, 1002, 1003]), np.array([1001, 1003]), np.array([1000]), np.array([1000, 1001, 1003])]
    vol = [np.ones(len(x)) for x in lv]
    add("one_level_bins.among_others", csr(regular_ts(4), [1000] * 4, [1003, 1003, 1000, 1003], lv, vol, vol), 0, 3, 1.0, ValueError,
        "E_LEVEL", "single price level")
    wide = [a.copy() for a in three_bars(40, 1, 1)]
    wide[1][1] = float((1 << 24) + 100)
    add("above_16m_levels", tuple(wide), 2, None, 1.0, ValueError, "E_CAPACITY", "price levels")
    add("nan_low", _with_nan("low"), 2, None, 1.0, ValueError, "E_ARG", NAN_MESSAGE)
    add("nan_high", _with_nan("high"), 2, 3, 1.0, ValueError, "E_ARG", NAN_MESSAGE)
    add("nan_all", _with_nan("all"), 2, None, 1.0, ValueError, "E_ARG", NAN_MESSAGE)
    add("nan_all.empty_bars", tuple(a if k != 3 else np.zeros_like(a) for k, a in enumerate(_with_nan("all")[:4])) +
        (np.empty(0, np.int32), np.empty(0, np.float32), np.empty(0, np.float32)), 2, None, 1.0, ValueError, "E_ARG", NAN_MESSAGE)


_refusals()
NAN_UNUSED = _with_nan("unused")                                 # a NaN low in a bar that no computed window holds: not refused
