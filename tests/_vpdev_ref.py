"""Plain sequential restatement of the reference's developing volume profile -- trim_trailing_zeros and volume_profile_developing
(feature/core/volume.py:459-569) -- on CSR footprints, in the contract include/fmk.h states (items 1-8 there), with the table of
hand-built cases that tools/gen_vpdev_golden.py, tests/test_vpdev_host.py and tests/test_gpu_vpdev.py share.  The stage functions and
the builders are those of tests/_vp_ref.py.

  range         bars searchsorted(ts, start_ts) .. searchsorted(ts, end_ts, 'right'); an empty one raises ValueError (np.min of nothing)
  level range   int(round(x / tick)) of min(lows), max(highs) of ALL bars of the range, once
  accumulation  bars one after another, per level `np.float32 +=`; after every bar total = buy + sell in float32
  no bins       comp_poc_hva_lva on the dense range, unrounded totals, no trim
  bins          np.round(total, 8) in float32 = rint(v * 1e8f) / 1e8f; entries == 0 dropped from both ends (NaN and negative entries
                stop the trim); a profile trimmed to nothing raises ValueError naming the bar; one level left comes back as its only
                bin; else bucket_price_levels on the trimmed levels; then comp_poc_hva_lva
  position      row t - start of the outputs
Reads nothing outside the repository."""
import functools
import math

import numpy as np

from tests import _vp_ref as H

ALL_ZERO_MESSAGE = "every total volume rounds to 0"
LEVEL_MESSAGE = "footprint level outside its range"
EMPTY_MESSAGE = "zero-size array to reduction operation minimum which has no identity"
CHUNKS = (0, 1, 2, 7, 64)                    # chunk_bars every case runs under on the device: automatic and forced
E8 = np.float32(1e8)


# ====================================================================================================== the restatement
def round8(v):
    """np.round(v, 8) of a float32 array, spelled out: multiply, rint, divide, each rounded to float32 (1e8 is a float32)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.rint(v * E8) / E8).astype(np.float32)


def trim_trailing_zeros(levels, volumes):
    v = round8(volumes)
    left, right = 0, len(levels) - 1
    while left <= right and v[left] == 0:
        left += 1
    while right >= left and v[right] == 0:
        right -= 1
    return levels[left:right + 1], v[left:right + 1]


def bar_range(ts, start_ts, end_ts):
    return int(np.searchsorted(ts, start_ts, side="left")), int(np.searchsorted(ts, end_ts, side="right"))


def developing_range(highs, lows, off, levels, buy, sell, s, e, n_bins, tick, va, info=None, which=0, trace=None):
    """-> (poc, hva, lva int32) of the bars [s, e).  `info`: receives L, the number of levels of the range; `trace`: a list that
    receives (cum, threshold) at every test of every walk's condition."""
    if s >= e:
        raise ValueError(EMPTY_MESSAGE)
    if not tick > 0:
        raise ValueError("price_tick must be > 0")
    if n_bins is not None and int(n_bins) == 0:
        raise ZeroDivisionError("integer division or modulo by zero")
    minl, maxl = H.level_of(np.min(lows[s:e]), tick), H.level_of(np.max(highs[s:e]), tick)   # NaN: ValueError
    n = maxl - minl + 1
    if n < 1:
        raise H.LevelError("its highest high is below its lowest low")
    if info is not None:
        info.setdefault("L", []).append(n)
    window = np.arange(minl, maxl + 1, dtype=np.int32)
    ab, as_ = np.zeros(n, np.float32), np.zeros(n, np.float32)
    poc, hva, lva = (np.zeros(e - s, np.int32) for _ in range(3))
    for t in range(s, e):
        r0, r1 = int(off[t]), int(off[t + 1])
        if r1 > r0:
            idx = levels[r0:r1].astype(np.int64) - minl
            if idx.min() < 0 or idx.max() >= n:
                raise H.LevelError(LEVEL_MESSAGE)
            ab[idx] += buy[r0:r1]
            as_[idx] += sell[r0:r1]
        tot = ab + as_
        lv = window
        if n_bins is not None:
            lv, tot = trim_trailing_zeros(window, tot)
            if len(lv) == 0:
                raise ValueError(f"range {which}, bar {t - s} of the range: {ALL_ZERO_MESSAGE}")
            if len(lv) > 1:
                lv, tot = H.bucket_price_levels(lv, tot, n_bins)
        poc[t - s], hva[t - s], lva[t - s] = H.comp_poc_hva_lva(lv, tot, va, trace=trace)
    return poc, hva, lva


def volume_profile_developing(ts, highs, lows, off, levels, buy, sell, start_ts, end_ts, n_bins=None, price_tick=None, va_pct=68.34,
                              info=None):
    nb = len(ts)
    if not (nb == len(highs) == len(lows) == len(off) - 1) or nb == 0:
        raise AssertionError("Input arrays should have the same length and be non-empty.")
    s, e = bar_range(ts, start_ts, end_ts)
    return (ts[s:e],) + developing_range(highs, lows, off, levels, buy, sell, s, e, n_bins, price_tick, va_pct, info)


def capacity_class(max_levels):
    return H.capacity_class(max_levels)


# ====================================================================================================== builders
def random_bars(n, kind, seed, lo=1, hi=6):
    return H.bars_from_counts(seed + 1, np.random.default_rng(seed).integers(lo, hi, n), kind)


def empties(kind, seed, first):
    """30 bars; empty ones at the first, an interior and the last place of the chunks of 2 and 7 bars (and bar 0 when `first`)."""
    counts = np.random.default_rng(seed).integers(1, 5, 30)
    counts[[3, 6, 7, 13, 14, 17, 20, 21, 29]] = 0
    if first:
        counts[0] = 0
    return H.bars_from_counts(seed + 1, counts, kind)


def explicit(bars, lo=100, hi=139):
    """bars: [(levels, buy, sell)]; every bar's low / high is lo / hi, so the range's levels are lo .. hi whatever the bars hold."""
    n = len(bars)
    return H.csr(H.regular_ts(n), [lo] * n, [hi] * n, [np.asarray(b[0], np.int64) for b in bars], [b[1] for b in bars], [b[2] for b in bars])


def trim(which):
    one = lambda l, v=1.5: ([l], [v], [0.25])
    if which == "lowest":
        return explicit([one(100, 1 + k / 4) for k in range(5)])
    if which == "highest":
        return explicit([one(139, 1 + k / 4) for k in range(5)])
    if which == "middle":
        return explicit([one(120, 1 + k / 4) for k in range(5)])
    if which == "down":
        return explicit([one(120 - 2 * k) for k in range(9)])
    if which == "up":
        return explicit([one(120 + 2 * k) for k in range(9)])
    if which == "by_one":
        return explicit([one(120 + (k + 1) // 2 * (1 if k % 2 else -1), 2.0 - k / 8) for k in range(12)])
    if which == "round_to_zero":             # 3e-9 rounds to 0, 5e-9 * 1e8 is a tie and rounds to even (0), 1.5e-8 rounds to 2e-8
        return explicit([([100, 110, 120, 139], [3e-9, 2.0, 1.0, 5e-9], [0, 0, 0, 0]), ([101, 138], [1.5e-8, 0], [0, 1.5e-8]),
                         ([100, 139], [3e-9, 5e-9], [0, 0])])
    if which == "tiny_only":                 # totals that all round to 0 but one of 1.5e-8
        return explicit([([105, 120, 130], [3e-9, 1.5e-8, 5e-9], [0, 0, 0]), ([105, 130], [3e-9, 0], [0, 5e-9])])
    if which == "negative_ends":             # negative entries at both ends stop the trim
        return explicit([([100, 120, 139], [-1.0, 3.0, -0.5], [0, 1.0, 0]), ([110, 125], [2.0, 1.0], [0.5, 0.5])])
    if which == "nan_ends":                  # NaN at the lowest level, later at the highest
        return explicit([([100, 120], [math.nan, 3.0], [0, 1.0]), ([110, 125], [2.0, 1.0], [0.5, 0.5]), ([139], [math.nan], [1.0])])
    raise KeyError(which)


def one_level(which):
    one = lambda l, v=1.5: ([l], [v], [0.25])
    many = ([104, 110, 120, 121, 133], [1, 2, 3.5, 1, 2], [0.5, 0, 1, 1, 0])
    if which == "first":
        return explicit([one(120), many, one(110), many])
    if which == "several":
        return explicit([one(120), one(120, 2.0), one(120, 0.5), many, many])
    raise KeyError(which)


def profile_last(total, split=True):
    """Three bars whose third profile is `total` exactly: the first bar brings the buy part, the second the sell part of
    _vp_ref.profile, the third is empty."""
    ts, hi, lo, off, lv, b, s = H.profile(total, split=split)
    z = np.zeros(len(lv), np.float32)
    return H.csr(H.regular_ts(3), [int(lv[0])] * 3, [int(lv[-1])] * 3, [lv, lv, lv[:0]], [b, z, z[:0]], [z, s, z[:0]])


def planted(where, value, seed):
    d = H.bars_from_counts(seed, [3] * 9, 2)
    return H.plant(d, int(d[3][{"first": 0, "middle": 4, "last": 8}[where]]) + 1, value, sell=(where == "middle"))


BUILDERS = dict(random_bars=random_bars, empties=empties, trim=trim, one_level=one_level, profile_last=profile_last,
                planted=planted, feeder=H.feeder, bar_widths=H.bar_widths, three_bars=H.three_bars, half_ticks=H.half_ticks,
                near_half_cent=H.near_half_cent, placement=H.placement)


# ====================================================================================================== the case table
# name -> dict(build=(builder, kwargs), spans=[(a, b)]: bar ranges [a, b) (b None: to the end), or stamps=(start_ts offset in ns from
# ts[a], end_ts offset from ts[b]) for a range given by time stamps between bars, n_bins, tick, va, kind (1 exact volumes, 2 lognormal,
# 3 NaN / inf))
CASES = {}


def _case(name, builder, kwargs, spans=((0, None),), n_bins=None, tick=1.0, va=68.34, kind=1, stamps=None):
    assert name not in CASES, name
    CASES[name] = dict(build=(builder, dict(kwargs)), spans=tuple(spans), n_bins=n_bins, tick=tick, va=va, kind=kind, stamps=stamps)


def _table():
    # ---- bars per range against the chunk length
    for n in sorted({m for k in (1, 2, 7, 64) for m in (k - 1, k, k + 1, 2 * k + 1) if m >= 1}):
        kind = 1 + n % 2
        _case(f"chunk.n{n}", "random_bars", dict(n=n, kind=kind, seed=500 + n), n_bins=None if n % 3 else 5, kind=kind)
    _case("chunk.auto200.raw", "random_bars", dict(n=200, kind=2, seed=77), kind=2)
    _case("chunk.auto200.b27", "random_bars", dict(n=200, kind=1, seed=78), n_bins=27)
    # ---- order of the float32 adds
    _case("feeder.raw", "feeder", dict(kind=2, seed=3), kind=2)
    _case("feeder.b3", "feeder", dict(kind=2, seed=4), n_bins=3, kind=2)
    # ---- levels per bar, empty bars
    for kind in (1, 2):
        _case(f"bar_widths.raw.k{kind}", "bar_widths", dict(kind=kind, seed=9), kind=kind)
        _case(f"bar_widths.b27.k{kind}", "bar_widths", dict(kind=kind, seed=10), n_bins=27, kind=kind)
        _case(f"empties.raw.k{kind}", "empties", dict(kind=kind, seed=7, first=True), kind=kind)
        _case(f"empties.b5.k{kind}", "empties", dict(kind=kind, seed=8, first=False), n_bins=5, kind=kind)
    # ---- levels per range, sparsely filled
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 20_000):
        _case(f"levels.{n}.raw", "three_bars", dict(n_levels=n, kind=1, seed=n))
        _case(f"levels.{n}.b27", "three_bars", dict(n_levels=n, kind=1, seed=n + 1), n_bins=27)
    for n in (65, 1025, 4097, 8193):
        _case(f"levels.{n}.b27.k2", "three_bars", dict(n_levels=n, kind=2, seed=n + 2, lone=40), n_bins=27, kind=2)
    # ---- trim
    for which in ("lowest", "highest", "middle", "down", "up", "by_one", "round_to_zero", "tiny_only", "negative_ends", "nan_ends"):
        kind = 3 if which == "nan_ends" else 1
        for nb in (None, 2, 5):
            _case(f"trim.{which}.{nb}", "trim", dict(which=which), n_bins=nb, kind=kind)
    # ---- one trimmed level under bucketing
    for which in ("first", "several"):
        for nb in (1, 3, 27):
            _case(f"one_level.{which}.b{nb}", "one_level", dict(which=which), n_bins=nb)
    # ---- bins: the layouts of the rolling table on a developing range
    for name, c in H.CASES.items():
        if name.split(".")[0] in ("bins", "bincount") and c["n_bins"] is not None:
            _case(name, c["build"][0], c["build"][1], n_bins=c["n_bins"], kind=c["kind"])
    # ---- the walk: profiles of the rolling table reached as the last bar of a 3-bar range
    for pname in ("poc_first", "poc_last", "two_levels", "max_10_74", "max_63_64", "max_three", "all_zero", "sym_long", "zeros_both",
                  "zeros_unequal", "up_short", "down_odd", "exact8", "exact64", "top_heavy", "ramp_up"):
        tot = H.CASES[f"walk.{pname}.va68.34"]["build"][1]["total"]
        for va in (0.0, 50.0, 68.34, 100.0, 150.0):
            _case(f"walk.{pname}.va{va}", "profile_last", dict(total=tot), va=va)
    for pname in ("max_63_64", "sym_long", "ramp_up", "exact64"):
        tot = H.CASES[f"walk.{pname}.va68.34"]["build"][1]["total"]
        _case(f"walk.{pname}.b3", "profile_last", dict(total=tot), n_bins=3)
    # ---- NaN / +inf volumes
    for where in ("first", "middle", "last"):
        for vname, value in (("nan", math.nan), ("inf", math.inf)):
            for nb in (None, 2):
                _case(f"special.{vname}.{where}.{nb}", "planted", dict(where=where, value=value, seed=600 + len(where)), n_bins=nb, kind=3)
    # ---- ranges
    base = dict(n=60, kind=1, seed=41)
    _case("ranges.start5", "random_bars", base, spans=[(5, 20)], n_bins=5)
    _case("ranges.start5.raw", "random_bars", base, spans=[(5, 20)])
    _case("ranges.single_bar", "random_bars", base, spans=[(7, 8)], n_bins=3)
    _case("ranges.touching", "random_bars", base, spans=[(0, 10), (10, 25)], n_bins=5)
    _case("ranges.overlapping", "random_bars", base, spans=[(0, 15), (10, 30), (12, 14)])
    _case("ranges.overlapping.k2", "random_bars", dict(n=60, kind=2, seed=42), spans=[(0, 15), (10, 30), (12, 14)], n_bins=5, kind=2)
    _case("ranges.between_bars", "random_bars", base, spans=[(3, 20)], stamps=(500_000_000, 500_000_000), n_bins=5)
    _case("ranges.duplicate_stamps", "placement", dict(which="dup", kind=1, seed=43), spans=[(4, 10)], stamps=(0, 0))
    rng = np.random.default_rng(50)
    at = np.concatenate([[0], np.cumsum(rng.integers(1, 10, 50))])
    _case("ranges.fifty", "random_bars", dict(n=int(at[-1]), kind=1, seed=44), spans=list(zip(at[:-1].tolist(), at[1:].tolist())), n_bins=5)
    # ---- tick rounding
    for tick in (1.0, 0.5, 0.25):
        _case(f"half_tick.{tick}.raw", "half_ticks", dict(tick=tick, kind=1, seed=5), tick=tick)
        _case(f"half_tick.{tick}.b3", "half_ticks", dict(tick=tick, kind=1, seed=5), n_bins=3, tick=tick)
    _case("near_half_cent.raw", "near_half_cent", dict(kind=1, seed=6), tick=0.01)
    _case("near_half_cent.b2", "near_half_cent", dict(kind=1, seed=6), n_bins=2, tick=0.01)


_table()
GROUPS = ("chunk", "feeder", "bar_widths", "empties", "levels", "trim", "one_level", "bins", "bincount", "walk", "special", "ranges",
          "half_tick", "near_half_cent")


def group(g):
    return [n for n in CASES if n.split(".")[0] == g]


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASES[name]
    d = BUILDERS[c["build"][0]](**c["build"][1])
    for a in d:
        a.setflags(write=False)
    return d


def stamps(name):
    """[(start_ts, end_ts)] of the case's ranges."""
    c = CASES[name]
    ts = inputs(name)[0]
    a0, b0 = c["stamps"] or (0, 0)
    return [(int(ts[a]) + a0, int(ts[(len(ts) if b is None else b) - 1]) + b0) for a, b in c["spans"]]


def bar_ranges(name):
    ts = inputs(name)[0]
    return [bar_range(ts, a, b) for a, b in stamps(name)]


def params(name):
    c = CASES[name]
    return c["n_bins"], c["tick"], c["va"]


def input_hash(name):
    c = CASES[name]
    return H.sha256(*inputs(name), np.array(stamps(name), np.int64), np.array([-1.0 if c["n_bins"] is None else c["n_bins"], c["tick"], c["va"]]))


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> ([(ts, poc, hva, lva)] per range, info): the restatement's outputs (computed once, shared, read-only)."""
    info = {}
    outs = []
    for a, b in stamps(name):
        o = volume_profile_developing(*inputs(name), a, b, *params(name), info=info)
        for x in o:
            x.setflags(write=False)
        outs.append(o)
    return outs, info


def names(kind=None):
    return [n for n, c in CASES.items() if kind is None or c["kind"] == kind]


# ====================================================================================================== refused calls
# name -> dict(inputs, span (bar range), n_bins, tick, va, error, code, message); "returns": calls that must NOT be refused
REFUSALS, RETURNS = {}, {}


def _nan_at(which, bar):
    d = [a.copy() for a in H.bars_from_counts(77, [3] * 10, 1)]
    d[2 if which == "low" else 1][bar] = math.nan
    return tuple(d)


def _empty_first():
    """Five bars; bars 0 and 3 are empty."""
    return H.bars_from_counts(88, [0, 3, 2, 0, 4], 1)


def _refusals():
    def add(name, data, span, n_bins, tick, error, code, message, va=68.34):
        REFUSALS[name] = dict(inputs=data, span=span, n_bins=n_bins, tick=tick, va=va, error=error, code=code, message=message)
    ok = H.three_bars(40, 1, 1)
    add("empty_range", ok, (2, 2), None, 1.0, ValueError, "E_ARG", "zero-size array")
    for where, pos in (("first64", 10), ("rest", 100)):
        add(f"level_below.{where}", H._bad_level(pos, 999), (0, 3), None, 1.0, ValueError, "E_LEVEL", "level outside")
        add(f"level_above.{where}", H._bad_level(pos, 1132), (0, 3), 5, 1.0, ValueError, "E_LEVEL", "level outside")
    add("nan_low", _nan_at("low", 5), (2, 8), None, 1.0, ValueError, "E_ARG", "NaN")
    add("nan_high", _nan_at("high", 5), (2, 8), 3, 1.0, ValueError, "E_ARG", "NaN")
    add("n_bins_0", ok, (0, 3), 0, 1.0, ZeroDivisionError, "E_ZERODIV", "division")
    add("tick_0", ok, (0, 3), None, 0.0, ValueError, "E_ARG", "price_tick")
    add("tick_negative", ok, (0, 3), None, -1.0, ValueError, "E_ARG", "price_tick")
    add("tick_nan", ok, (0, 3), None, math.nan, ValueError, "E_ARG", "price_tick")
    add("all_zero_first_bar.bins", _empty_first(), (0, 5), 5, 1.0, ValueError, "E_LEVEL", "bar 0 of the range")
    add("all_zero_later_start.bins", _empty_first(), (3, 5), 5, 1.0, ValueError, "E_LEVEL", "bar 0 of the range")
    wide = [a.copy() for a in ok]
    wide[1][1] = float((1 << 24) + 100)
    add("above_16m_levels", tuple(wide), (0, 3), None, 1.0, ValueError, "E_CAPACITY", "price levels")
    RETURNS["nan_low.outside"] = dict(inputs=_nan_at("low", 5), span=(6, 10), n_bins=None, tick=1.0, va=68.34)
    RETURNS["nan_high.outside"] = dict(inputs=_nan_at("high", 1), span=(2, 10), n_bins=3, tick=1.0, va=68.34)
    RETURNS["all_zero_first_bar.raw"] = dict(inputs=_empty_first(), span=(0, 5), n_bins=None, tick=1.0, va=68.34)


_refusals()


def refusal_stamps(c):
    ts = c["inputs"][0]
    a, b = c["span"]
    if a >= b:                                                   # an empty range: end stamp in front of the start stamp
        return int(ts[a]), int(ts[a]) - 1
    return int(ts[a]), int(ts[b - 1])


# ====================================================================================================== np.round(x, 8) in float32
def round_probe():
    """A fixed float32 array for the rounding emulation: lognormal over 12 decades, dyadic values, and the special values."""
    rng = np.random.default_rng(123)
    a = np.exp(rng.uniform(math.log(1e-10), math.log(1e2), 20000)).astype(np.float32)
    d = (rng.integers(0, 1 << 20, 5000) / np.float32(1 << 12)).astype(np.float32)
    sp = np.array([0.0, -0.0, math.inf, -math.inf, math.nan, -1.0, -3e-9, 3.3e38, 5e-9, 3e-9, 1.5e-8, 2.5e-8, 1e-8, 0.5, 1e30, 16777216.0,
                   1.00000001, 123456.789], np.float32)
    return np.concatenate([a, -a[:2000], d, sp])


# profiles for trim_trailing_zeros on its own (levels 100, 101, ...): zeros and tiny values at both ends, nothing left, a NaN and a
# negative entry at an end, float64 volumes
TRIM_PROFILES = (np.array([0, 0, 3e-9, 1, 0, 2, 5e-9, 0], np.float32), np.zeros(5, np.float32), np.array([math.nan, 0, 1, 0], np.float32),
                 np.array([0, -1, 0, 1.5e-8, 0], np.float32), np.array([1.5e-8, 0.25, 0, 7], np.float32),
                 np.array([0.0, 1e-9, 2.0, 0.0], np.float64))
