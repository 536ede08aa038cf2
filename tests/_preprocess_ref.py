"""Plain sequential restatements of the two loops of TradesData(preprocess=True) -- merge_split_trades (finmlkit/bar/utils.py:263-329)
and comp_trade_side_vector (:26-46) --, of TimeBarReader._resample (finmlkit/bar/io.py:890-950) per group, and the hand-built cases that the host tests (tests/test_preprocess_host.py) and the GPU tests
(tests/test_gpu_preprocess_edges.py) share.  The cases are placed round the geometry of csrc/fmk_preprocess.hip: tiles of 2048 ticks,
the 1024-tile trips of the one-block scans (k_side_scan_tiles, k_scan_tile_scan), the rows (256 ticks) and waves (64) of
k_merge_emit, and the two thresholds (1e-12 strict, 1e-8 strict, head-relative); and of csrc/fmk_resample.hip: the grid-stride loop
past 128 * n_cu groups, the 64-row chunks, the three paths of the weighted median and the Kahan recurrence.

Every generator is integer arithmetic on a counter hash (splitmix64) followed by at most one IEEE multiplication per element, so every
machine regenerates the same bits; tools/gen_preprocess_edges_golden.py records the untouched reference on every case and the
sha256 of every generated input (tests/golden/preprocess_edges.{json,npz})."""
import functools
import hashlib

import numpy as np

SV_TILE = MG_TILE = 2048
TRIP = 1024                                   # tile aggregates scanned per trip of the one-block scans
TRIP_N = TRIP * SV_TILE                       # 2 097 152: the second trip starts past this many ticks
T0 = 1_700_000_000_000_000_000
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
NAN, INF = float("nan"), float("inf")
HASH_ABOVE = 2100                             # outputs longer than this are recorded as a sha256


# ---------------------------------------------------------------------------------------------- the restatements
def comp_trade_side_vector(prices):
    """side[0] = 0; side[i] = sign(p[i] - p[i-1]) if |p[i] - p[i-1]| > 1e-12 else side[i-1] (a NaN difference is not a move)."""
    p = np.ascontiguousarray(prices, dtype=np.float64).tolist()
    n = len(p)
    if n == 0:
        raise IndexError("empty prices")                          # the reference reads prices[0]
    out = [0] * n
    side, prev = 0, p[0]
    for i in range(1, n):
        x = p[i]
        dp = x - prev
        if abs(dp) > 1e-12:
            side = 1 if dp > 0 else -1
        out[i] = side
        prev = x
    return np.array(out, dtype=np.int8)


def merge_split_trades(timestamps, prices, amounts, is_buyer_maker):
    """A trade joins the merged trade in front of it iff its timestamp and flag equal the HEAD's and |price - head price| < 1e-8;
    the head's float32 amount takes `+=` in trade order.  -> (ts, price, amount float32, side int8 | empty)."""
    t = np.ascontiguousarray(timestamps, dtype=np.int64).tolist()
    p = np.ascontiguousarray(prices, dtype=np.float64).tolist()
    a = list(np.ascontiguousarray(amounts, dtype=np.float32))     # numpy float32 scalars: every `+` rounds to float32
    f = None if is_buyer_maker is None else np.ascontiguousarray(is_buyer_maker).astype(bool).tolist()
    n = len(t)
    if n == 0:
        raise IndexError("empty trades")                          # the reference reads element 0
    o_t, o_p, o_a, o_f = [t[0]], [p[0]], [a[0]], [f[0] if f else False]
    with np.errstate(all="ignore"):
        for i in range(1, n):
            same = t[i] == o_t[-1] and abs(p[i] - o_p[-1]) < 1e-8
            if f is not None:
                same = same and f[i] == o_f[-1]
            if same:
                o_a[-1] = o_a[-1] + a[i]
            else:
                o_t.append(t[i])
                o_p.append(p[i])
                o_a.append(a[i])
                o_f.append(f[i] if f else False)
    side = np.where(np.array(o_f, dtype=bool), -1, 1).astype(np.int8) if f is not None else np.empty(0, dtype=np.int8)
    return np.array(o_t, dtype=np.int64), np.array(o_p, dtype=np.float64), np.array(o_a, dtype=np.float32), side


# ---------------------------------------------------------------------------------------------- comparison, hashing
MERGE_KEYS = ("ts", "px", "am", "side")


def same(got, want, what):
    """dtype, shape and value of every element (NaN at the same places); no tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if not np.array_equal(got, want, equal_nan=got.dtype.kind == "f"):
        bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))))
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, first at {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}")
    return got.size


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- generators
def mix(seed, n):
    """splitmix64 of the counters 1 .. n under `seed` -> uint64[n]."""
    with np.errstate(over="ignore"):
        z = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def cents(steps, base=2_700_000):
    """A price series from integer steps: (base + cumsum(steps)) cents."""
    return (base + np.cumsum(np.asarray(steps, dtype=np.int64))) * 0.01


def walk_steps(seed, n):
    return ((mix(seed, n) >> np.uint64(11)) % np.uint64(3)).astype(np.int64) - 1          # -1, 0, +1


def mantissa_amounts(seed, n):
    """float32 sizes in [8, 16) with all 24 mantissa bits in use: the order of a float32 sum shows."""
    return (((mix(seed, n) >> np.uint64(20)) & np.uint64(0x7FFFFF)) | np.uint64(0x800000)).astype(np.float32) * np.float32(2.0 ** -20)


# ---- tick rule
STRETCH = (1020 * SV_TILE, 1028 * SV_TILE)    # the flat stretch: tiles 1020 .. 1027 (cut at n)
PLACE_N = 3 * SV_TILE + 9
PLACE_AT = (1, 7, 8, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, PLACE_N - 1)
EPS_N = SV_TILE + 8


def _tick_trip(variant, m):
    n = TRIP_N + m
    s = walk_steps(11, n)
    a, b = STRETCH[0], min(STRETCH[1], n)
    s[a:b] = 0
    if variant == "flat":
        s[:b] = 0                                                 # flat from tick 0: zeros carried across the trip
    else:
        s[a - 1] = 1 if variant == "up" else -1                   # the last move in front of the stretch
    return cents(s)


def _tick_single(idx):
    p = np.full(PLACE_N, 100.0)
    p[idx:] = 100.01 if idx % 2 else 99.99
    return p


def _tick_mirror(idx):
    s = np.zeros(PLACE_N, dtype=np.int64)
    if idx - 1 >= 1:
        s[idx - 1] = 1
    if idx + 1 <= PLACE_N - 1:
        s[idx + 1] = -1
    return cents(s)


def _tick_eps(sign, moved):
    """price[0] sets the side to -sign at tick 1; the first element of tile 1 then differs from 0.0 by exactly 1e-12 (no move) or by
    the next double above it (a move to sign)."""
    p = np.zeros(EPS_N)
    p[0] = sign * 1.0
    p[SV_TILE:] = sign * (np.nextafter(1e-12, 1.0) if moved else 1e-12)
    return p


def _alternating(n):
    return cents(1 - 2 * (np.arange(n) % 2))                      # a move at every tick, up and down in turn


def _tick_odd(kind):
    p = _alternating(EPS_N)
    if kind in ("nan_last", "nan_both"):
        p[SV_TILE - 1] = NAN
    if kind in ("nan_first", "nan_both"):
        p[SV_TILE] = NAN
    if kind in ("pinf", "ninf"):
        p[SV_TILE - 1] = p[SV_TILE] = INF if kind == "pinf" else -INF
    return p


TICK_CASES = {}
for _v in ("up", "down", "flat"):
    for _m in (-1, 0, 1, 2049):
        TICK_CASES[f"tick.trip.{_v}.m{_m}"] = functools.partial(_tick_trip, _v, _m)
TICK_CASES["tick.trip.up.m12297"] = functools.partial(_tick_trip, "up", 6 * SV_TILE + 9)    # moves again behind the stretch
for _i in PLACE_AT:
    TICK_CASES[f"tick.single.{_i}"] = functools.partial(_tick_single, _i)
    TICK_CASES[f"tick.mirror.{_i}"] = functools.partial(_tick_mirror, _i)
for _s, _sn in ((1.0, "pos"), (-1.0, "neg")):
    TICK_CASES[f"tick.eps.{_sn}.exact"] = functools.partial(_tick_eps, _s, False)
    TICK_CASES[f"tick.eps.{_sn}.above"] = functools.partial(_tick_eps, _s, True)
for _k in ("nan_last", "nan_first", "nan_both", "pinf", "ninf"):
    TICK_CASES[f"tick.odd.{_k}"] = functools.partial(_tick_odd, _k)
TICK_CASES["tick.odd.negzero"] = lambda: np.array([1.0, 0.0, -0.0, 0.0, -0.0, -0.0, 1.0, -0.0])
TICK_CASES["tick.n1"] = lambda: np.array([5.0])
TICK_CASES["tick.n2.up"] = lambda: np.array([5.0, 5.5])
TICK_CASES["tick.n2.down"] = lambda: np.array([5.0, 4.5])
TICK_CASES["tick.n2.flat"] = lambda: np.array([5.0, 5.0])


# ---- merge
RUN_LEN, RUN_PIECE = 5000, 7
EMIT_HEADS = (0, 63, 64, 255, 256, 257, 2047)
NOHEAD = (2000, 6200)                         # first and last tick of the one-trade stretch
CHAIN_AT, CHAIN_LEN, CHAIN_STEP = SV_TILE - 2, 12, 6e-9
MG_TRIP_N = TRIP_N + 2049


def _background(n, seed):
    """Strictly increasing timestamps (every trade a head), a cent walk, full-mantissa sizes, one flag in eight set."""
    h = mix(seed, n)
    ts = T0 + np.arange(n, dtype=np.int64) * 1000
    return ts, cents(walk_steps(seed + 1, n)), mantissa_amounts(seed + 2, n), ((h >> np.uint64(50)) & np.uint64(7)) == 0


def _put_run(ts, px, ibm, start, length=RUN_LEN):
    """One coarse run: `length` trades of one timestamp and flag, the price changing every RUN_PIECE trades."""
    end = min(start + length, len(ts))
    ts[start:end] = ts[start]
    px[start:end] = 100.0 + (np.arange(end - start) // RUN_PIECE) * 0.01
    ibm[start:end] = False
    return end


def _mg_trip():
    n = MG_TRIP_N
    h = mix(21, n)
    new_ts = (h & np.uint64(1)) == 1                              # bursts of geometric length (p = 1/2)
    new_ts[0] = True
    ts = T0 + np.cumsum(new_ts.astype(np.int64)) * 1000
    k = (h >> np.uint64(3)) % np.uint64(5)
    px = cents(np.where(k == 0, -1, np.where(k == 1, 1, 0)))
    ibm = ((h >> np.uint64(40)) & np.uint64(3)) == 0
    _put_run(ts, px, ibm, TRIP_N - 3)                             # the run crosses the trip edge and the tile edge behind it
    return ts, px, mantissa_amounts(22, n), ibm


def _mg_run_edges():
    ts, px, am, ibm = _background(4 * MG_TILE + 5, 31)
    _put_run(ts, px, ibm, MG_TILE - 3)
    return ts, px, am, ibm


def _mg_nohead():
    ts, px, am, ibm = _background(4 * MG_TILE + 5, 41)
    a, b = NOHEAD[0], NOHEAD[1] + 1
    ts[a:b], px[a:b], ibm[a:b] = ts[a], 123.45, False
    return ts, px, am, ibm


def _mg_all_heads():
    return _background(2 * MG_TILE + 1, 51)


def _mg_one_trade():
    n = 2 * MG_TILE + 1
    return np.full(n, T0, dtype=np.int64), np.full(n, 27000.01), mantissa_amounts(61, n), np.zeros(n, dtype=bool)


def _mg_emit_edges():
    ts, px, am, ibm = _background(3 * MG_TILE, 71)
    t = slice(MG_TILE, 2 * MG_TILE)
    piece = np.zeros(MG_TILE, dtype=np.int64)
    piece[list(EMIT_HEADS[1:])] = 1
    ts[t], px[t], ibm[t] = ts[MG_TILE], 50.0 + np.cumsum(piece) * 0.01, False
    return ts, px, am, ibm


def _mg_drift(b):
    ts, px, am, ibm = _background(MG_TILE + 64, 81)
    c = slice(CHAIN_AT, CHAIN_AT + CHAIN_LEN)
    ts[c], px[c], ibm[c] = ts[CHAIN_AT], b + np.arange(CHAIN_LEN) * CHAIN_STEP, False
    return ts, px, am, ibm


def _small(prices, amounts=None, flags=None, ts=None):
    n = len(prices)
    return (np.full(n, T0, dtype=np.int64) if ts is None else np.array(ts, dtype=np.int64), np.array(prices, dtype=np.float64),
            np.ones(n, dtype=np.float32) * np.float32(1.25) if amounts is None else np.array(amounts, dtype=np.float32),
            np.zeros(n, dtype=bool) if flags is None else np.array(flags, dtype=bool))


def _mg_all_true():
    ts, px, am, ibm = _background(MG_TILE + 300, 91)
    ts[10:40] = ts[10]
    px[10:40] = px[10]
    ts[2040:2060] = ts[2040]                                       # a merged trade across the tile edge, flags true
    px[2040:2060] = px[2040]
    return ts, px, am, np.ones(len(ts), dtype=bool)


MERGE_CASES = {
    "merge.trip": _mg_trip,
    "merge.run_edges": _mg_run_edges,
    "merge.nohead": _mg_nohead,
    "merge.all_heads": _mg_all_heads,
    "merge.one_trade": _mg_one_trade,
    "merge.emit_edges": _mg_emit_edges,
    "merge.drift.b1": functools.partial(_mg_drift, 1.0),
    "merge.drift.b27000": functools.partial(_mg_drift, 27000.0),
    "merge.1e-8.exact": lambda: _small([0.0, 1e-8]),
    "merge.1e-8.below": lambda: _small([0.0, np.nextafter(1e-8, 0.0)]),
    "merge.price.nan": lambda: _small([1.0, NAN, NAN, 1.0, 1.0]),
    "merge.price.inf": lambda: _small([INF, INF, 2.0, -INF, -INF]),
    "merge.price.negzero": lambda: _small([0.0, -0.0, 0.0, 1.0, -0.0, 0.0]),
    "merge.price.aba": lambda: _small([5.0, 6.0, 5.0]),
    "merge.amount.absorbed": lambda: _small([9.5] * 301, amounts=[2.0 ** 24] + [1.0] * 300),
    "merge.amount.reversed": lambda: _small([9.5] * 301, amounts=[1.0] * 300 + [2.0 ** 24]),
    "merge.amount.nan": lambda: _small([9.5, 9.5, 9.5, 8.5, 8.5], amounts=[1.5, NAN, 2.0, 3.0, 4.0]),
    "merge.amount.inf": lambda: _small([9.5, 9.5, 9.5, 8.5, 8.5, 8.5], amounts=[1.5, INF, 2.0, 3.0, INF, -INF]),
    "merge.amount.negzero": lambda: _small([9.5, 8.5, 8.5, 7.5], amounts=[-0.0, -0.0, -0.0, 1.0], ts=[T0, T0 + 1, T0 + 1, T0 + 2]),
    "merge.flag.flip": lambda: _small([9.5] * 6, flags=[False, True, True, False, False, True]),
    "merge.flag.all_true": _mg_all_true,
    "merge.ts.ends": lambda: _small([9.5] * 9, ts=[I64_MIN, I64_MIN, I64_MIN + 1, -5, -5, -1, 0, I64_MAX, I64_MAX]),
    "merge.ts.nonadjacent": lambda: _small([9.5] * 5, ts=[7, 9, 7, 7, 9]),
}
REFUSED_CASES = {
    "refused.tick.empty": ("tick", lambda: np.empty(0)),
    "refused.merge.empty": ("merge", lambda: (np.empty(0, np.int64), np.empty(0), np.empty(0, np.float32), np.empty(0, bool))),
}
LARGE = tuple(n for n in list(TICK_CASES) + list(MERGE_CASES) if n.startswith("tick.trip.") or n == "merge.trip")
SMALL_TICK = tuple(n for n in TICK_CASES if n not in LARGE)
SMALL_MERGE = tuple(n for n in MERGE_CASES if n not in LARGE)


@functools.lru_cache(maxsize=3)
def inputs(name):
    """The case's input arrays (read-only): a price array for a tick-rule case, (ts, px, am, flags) for a merge case."""
    v = TICK_CASES[name]() if name in TICK_CASES else MERGE_CASES[name]()
    for a in (v if isinstance(v, tuple) else (v,)):
        a.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _expected_small(name, with_flag):
    return expected_uncached(name, with_flag)


def expected_uncached(name, with_flag=True):
    if name in TICK_CASES:
        return comp_trade_side_vector(inputs(name))
    ts, px, am, ibm = inputs(name)
    return merge_split_trades(ts, px, am, ibm if with_flag else None)


def expected(name, with_flag=True):
    """The restatement's output, computed once per small case and left unchanged (the large cases are not kept)."""
    if name in LARGE:
        return expected_uncached(name, with_flag)
    out = _expected_small(name, bool(with_flag))
    for a in (out if isinstance(out, tuple) else (out,)):
        a.setflags(write=False)
    return out


def head_flags(ts, px, ibm):
    """Which trades open a merged trade, by the decomposition the kernel uses: timestamp and flag against the trade in front (all
    members of a merged trade share them), the price against the head's inside such a run."""
    n = len(ts)
    coarse = np.ones(n, dtype=bool)
    coarse[1:] = ts[1:] != ts[:-1]
    if ibm is not None:
        coarse[1:] |= ibm[1:] != ibm[:-1]
    heads = coarse.copy()
    p, c = px.tolist(), coarse.tolist()
    head = p[0]
    for i in range(1, n):
        if c[i]:
            head = p[i]
        elif not abs(p[i] - head) < 1e-8:
            heads[i] = True
            head = p[i]
    return heads


# ---------------------------------------------------------------------------------------------- structural assertions
def check_structure(name, want, want_noflag=None):
    """What the case claims to reach, asserted on its inputs and on the expectation `want` (from the restatement, the recording or
    the C oracle -- the three agree).  -> a dict of the figures, for the counts."""
    info = {}
    if name.startswith("tick.trip."):
        p = inputs(name)
        n = len(p)
        m = n - TRIP_N
        tiles = -(-n // SV_TILE)
        a, b = STRETCH[0], min(STRETCH[1], n)
        variant = name.split(".")[2]
        carried = {"up": 1, "down": -1, "flat": 0}[variant]
        assert (tiles > TRIP) == (m > 0) and tiles >= TRIP          # m <= 0 stops at the end of the first trip: the edge from below
        assert a // SV_TILE == 1020 and (np.diff(p[a - 1:b]) == 0).all()      # whole tiles of zero aggregate from tile 1020 on
        if m > 0:
            assert a // SV_TILE < TRIP <= (b - 1) // SV_TILE        # ... on both sides of the trip edge
            assert (want[TRIP_N:b] == carried).all()
        assert (want[a:b] == carried).all() and (variant == "flat" or want[a - 1] == carried)
        if variant == "flat":
            assert not want[:b].any()
        if b < n:
            assert len(np.unique(want[b:])) == 2 and (np.diff(p[b - 1:]) != 0).any()     # both signs behind the stretch
        info.update(tiles=tiles, stretch_tiles=(b - a + SV_TILE - 1) // SV_TILE)
    elif name.startswith("tick.single."):
        i = int(name.split(".")[2])
        s = 1 if i % 2 else -1
        assert len(want) == PLACE_N and not want[:i].any() and (want[i:] == s).all()
        if i == 1:
            assert (want[2 * SV_TILE:3 * SV_TILE] == s).all()       # carried across two whole tiles of zero aggregate
    elif name.startswith("tick.mirror."):
        i = int(name.split(".")[2])
        assert want[i] == want[i - 1] and (i + 1 >= PLACE_N or want[i + 1] == -1) and (i - 1 < 1 or want[i - 1] == 1)
    elif name.startswith("tick.eps."):
        _, _, sn, kind = name.split(".")
        s = 1 if sn == "pos" else -1
        p = inputs(name)
        d = abs(p[SV_TILE] - p[SV_TILE - 1])
        assert (d == 1e-12 and not d > 1e-12) if kind == "exact" else (d > 1e-12 and d == np.nextafter(1e-12, 1.0))
        assert (want[1:SV_TILE] == -s).all() and (want[SV_TILE:] == (-s if kind == "exact" else s)).all()
    elif name.startswith("tick.odd.nan"):
        clean = comp_trade_side_vector(_alternating(EPS_N))
        killed = np.flatnonzero(want != clean)
        k = name.split(".")[2]
        # an alternating walk moves at every tick: a NaN at i takes the moves of i and i + 1, and the side of i - 1 stays for both
        first = {"nan_last": SV_TILE - 1, "nan_first": SV_TILE, "nan_both": SV_TILE - 1}[k]
        assert want[first] == want[first - 1] == want[first + 1] and len(killed) >= 1 and killed.min() >= first
        if k == "nan_both":
            assert want[first + 2] == want[first - 1] and len(set(want[first - 1:first + 3])) == 1
    elif name in ("tick.odd.pinf", "tick.odd.ninf"):
        s = 1 if name.endswith("pinf") else -1
        assert list(want[SV_TILE - 1:SV_TILE + 2]) == [s, s, -s]
    elif name == "tick.odd.negzero":
        assert list(want) == [0, -1, -1, -1, -1, -1, 1, -1]
    elif name == "merge.trip":
        ts, px, am, ibm = inputs(name)
        heads = head_flags(ts, px, ibm)
        assert heads.sum() == len(want[0])
        per_tile = np.add.reduceat(heads.astype(np.int64), np.arange(0, len(ts), MG_TILE))
        assert len(per_tile) > TRIP and per_tile[TRIP - 1] > 0 and per_tile[TRIP] > 0
        assert len(want[0]) > per_tile[:TRIP].sum() > 0             # more merged trades than one trip counts
        run = slice(TRIP_N - 3, len(ts))
        assert (ts[run] == ts[TRIP_N - 3]).all() and heads[run].sum() == -(-(len(ts) - TRIP_N + 3) // RUN_PIECE)
        info.update(tiles=len(per_tile), heads_first_trip=per_tile[:TRIP].sum(), heads_behind=per_tile[TRIP:].sum())
    elif name == "merge.run_edges":
        ts, px, am, ibm = inputs(name)
        heads = head_flags(ts, px, ibm)
        assert heads.sum() == len(want[0])
        s = MG_TILE - 3
        assert (ts[s:s + RUN_LEN] == ts[s]).all() and s + RUN_LEN > 3 * MG_TILE          # crosses the edges at 2048, 4096 and 6144
        assert heads[MG_TILE:2 * MG_TILE].sum() == heads[2 * MG_TILE:3 * MG_TILE].sum() - 1 == MG_TILE // RUN_PIECE
        assert len(want[0]) == len(ts) - RUN_LEN + -(-RUN_LEN // RUN_PIECE)
    elif name == "merge.nohead":
        ts, px, am, ibm = inputs(name)
        heads = head_flags(ts, px, ibm)
        assert heads.sum() == len(want[0])
        assert not heads[MG_TILE:3 * MG_TILE].any() and heads[NOHEAD[0]] and heads[NOHEAD[1] + 1]
        tot = np.float32(0)
        for x in am[NOHEAD[0]:NOHEAD[1] + 1]:
            tot = tot + x
        assert want[2][NOHEAD[0]] == tot != np.float32(am[NOHEAD[0]:NOHEAD[1] + 1][::-1].cumsum(dtype=np.float32)[-1])   # the order shows
    elif name == "merge.all_heads":
        assert len(want[0]) == 2 * MG_TILE + 1 == len(want_noflag[0])
    elif name == "merge.one_trade":
        assert len(want[0]) == 1 == len(want_noflag[0])
    elif name == "merge.emit_edges":
        ts, px, am, ibm = inputs(name)
        slots = np.flatnonzero(want[0] == ts[MG_TILE])
        assert list(slots) == [MG_TILE + r for r in range(len(EMIT_HEADS))]             # tile 0 holds 2048 heads, tile 1 these seven
        assert list(want[1][slots]) == [px[MG_TILE + h] for h in EMIT_HEADS]
        lens = np.diff(EMIT_HEADS + (MG_TILE,))
        assert len(want[0]) == 2 * MG_TILE + len(EMIT_HEADS)
        info.update(followers=int(lens.sum() - len(EMIT_HEADS)))
    elif name.startswith("merge.drift."):
        ts, px, am, ibm = inputs(name)
        x = px[CHAIN_AT:CHAIN_AT + CHAIN_LEN]
        assert (np.abs(np.diff(x)) < 1e-8).all()                    # a previous-relative rule would merge the whole chain
        assert [bool(abs(v - x[0]) < 1e-8) for v in x[:3]] == [True, True, False]
        in_chain = int((want[0] == ts[CHAIN_AT]).sum())
        assert 3 * in_chain > CHAIN_LEN and in_chain == CHAIN_LEN // 2 and CHAIN_AT < MG_TILE < CHAIN_AT + CHAIN_LEN
        info.update(chain_heads=in_chain)
    elif name == "merge.1e-8.exact":
        assert len(want[0]) == 2 and not 1e-8 < 1e-8
    elif name == "merge.1e-8.below":
        assert len(want[0]) == 1
    elif name == "merge.price.nan":
        assert len(want[0]) == 4 and np.isnan(want[1][1:3]).all()  # 1 | NaN | NaN | 1 1
    elif name == "merge.price.inf":
        assert len(want[0]) == 5
    elif name == "merge.price.negzero":
        assert len(want[0]) == 3 and list(want[2]) == [3.75, 1.25, 2.5]
    elif name == "merge.price.aba":
        assert len(want[0]) == 3
    elif name == "merge.amount.absorbed":
        assert list(want[2]) == [2.0 ** 24]
    elif name == "merge.amount.reversed":
        assert list(want[2]) == [2.0 ** 24 + 300]
    elif name == "merge.amount.nan":
        assert np.isnan(want[2][0]) and want[2][1] == 7.0
    elif name == "merge.amount.inf":
        assert want[2][0] == INF and np.isnan(want[2][1])
    elif name == "merge.amount.negzero":
        assert list(want[2]) == [0.0, 0.0, 1.0] and np.signbit(want[2][:2]).all()
    elif name == "merge.flag.flip":
        assert len(want[0]) == 4 and list(want[3]) == [1, -1, 1, -1] and len(want_noflag[0]) == 1
    elif name == "merge.flag.all_true":
        assert (want[3] == -1).all() and len(want[0]) == len(want_noflag[0]) == MG_TILE + 300 - 29 - 19
    elif name == "merge.ts.ends":
        assert list(want[0]) == [I64_MIN, I64_MIN + 1, -5, -1, 0, I64_MAX]
    elif name == "merge.ts.nonadjacent":
        assert list(want[0]) == [7, 9, 7, 9]
    return info


# ================================================================================================ resampling
RS_COLS = ("open", "high", "low", "close", "volume", "trades", "vwap", "median_trade_size")
RS_OUT = RS_COLS + ("valid",)


def _kahan(values):
    """pandas' group_sum: Kahan's recurrence in the column's own dtype, NaN rows skipped, the compensation reset when it is NaN."""
    T = values.dtype.type
    s = c = T(0)
    for v in values:
        if v != v:
            continue
        y = v - c
        t = s + y
        c = (t - s) - y
        if c != c:
            c = T(0)
        s = t
    return s


def resample_groups(seg, open_, high, low, close, volume, trades, vwap, median):
    """Rows [seg[g], seg[g+1]) are group g -> (open, high, low, close, volume, trades, vwap float32, median float32, valid uint8)."""
    G = len(seg) - 1
    out = [np.empty(G, np.float64) for _ in range(4)] + [np.empty(G, volume.dtype), np.empty(G, np.int64), np.empty(G, np.float32),
                                                         np.empty(G, np.float32), np.empty(G, np.uint8)]
    with np.errstate(all="ignore"):
        pv = vwap * volume                                        # float32 only when both columns are
        for g in range(G):
            s, e = int(seg[g]), int(seg[g + 1])
            first = last = hi = lo = NAN
            have = False
            for i in range(s, e):
                if not have and open_[i] == open_[i]:
                    first, have = open_[i], True
                if close[i] == close[i]:
                    last = close[i]
                if high[i] == high[i] and not hi >= high[i]:
                    hi = high[i]
                if low[i] == low[i] and not lo <= low[i]:
                    lo = low[i]
            vs, ps = _kahan(volume[s:e]), _kahan(pv[s:e])
            sizes = median[s:e]
            order = np.argsort(sizes, kind="stable")             # NaN last
            cum = np.cumsum(trades[s:e][order].astype(np.float64))
            out[0][g], out[1][g], out[2][g], out[3][g] = first, hi, lo, last
            out[4][g] = vs
            out[5][g] = int(trades[s:e].sum())
            out[6][g] = np.float32(ps / vs) if pv.dtype == np.float32 else np.float32(np.float64(ps) / np.float64(vs))
            out[7][g] = np.float32(sizes[order][np.searchsorted(cum, cum[-1] * 0.5, side="left")])
            out[8][g] = have
    return tuple(out)


def _rows(seed, R):
    """Seeded columns for R rows: a cent walk, full-mantissa float32 volumes, 0 .. 4 trades, medians on a grid of eighths (ties)."""
    h = mix(seed, R)
    px = cents(walk_steps(seed + 1, R))
    return {"open": px.copy(), "high": px + ((h >> np.uint64(5)) % np.uint64(4)).astype(np.float64) * 0.01,
            "low": px - ((h >> np.uint64(8)) % np.uint64(4)).astype(np.float64) * 0.01, "close": px + 0.0,
            "volume": mantissa_amounts(seed + 2, R), "trades": ((h >> np.uint64(30)) % np.uint64(5)).astype(np.int64),
            "vwap": px + 0.005, "median_trade_size": ((h >> np.uint64(40)) % np.uint64(64)).astype(np.float64) * 0.125}


def _sprinkle_nan(d, seed, one_in=16):
    h = mix(seed, len(d["open"]))
    for k, c in enumerate(("open", "high", "low", "close", "volume", "vwap", "median_trade_size")):
        d[c][((h >> np.uint64(6 * k)) % np.uint64(one_in)) == 0] = NAN
    return d


def _cast(d, combo):
    """combo "v32w64" ...: the dtypes of the volume and vwap columns (the four instantiations of k_resample)."""
    d["volume"] = d["volume"].astype(np.float32 if combo[:3] == "v32" else np.float64)
    d["vwap"] = d["vwap"].astype(np.float32 if combo[3:] == "w32" else np.float64)
    return d


COMBOS = ("v32w32", "v32w64", "v64w32", "v64w64")
GRID_GROUPS = 70_000
SIZES = (1, 63, 64, 65, 128, 129, 4097)


def _seg(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _rs_grid():
    lens = 1 + (mix(101, GRID_GROUPS) % np.uint64(3)).astype(np.int64)
    seg = _seg(lens)
    return seg, _cast(_sprinkle_nan(_rows(102, int(seg[-1])), 105), "v32w64")


def _rs_sizes(combo):
    seg = _seg(SIZES)
    d = _sprinkle_nan(_rows(111, int(seg[-1])), 115, one_in=32)
    d["volume"] = d["volume"].astype(np.float64) * 1.000001 if combo[:3] == "v64" else d["volume"]      # rounding in every float64 step
    return seg, _cast(d, combo)


# -- weighted median: every pattern once in a group of at most 64 rows and once in a longer one
MEDIAN_PATTERNS = ("zero_trades", "exact_cutoff", "equal_run", "nan_majority", "all_nan", "neg_inf", "pos_inf", "neg_zero")
MEDIAN_LENS = (64, 65, 40, 130)


def _median_group(pattern, L, seed):
    """-> (sizes, weights) of one group of L rows, in a seeded order."""
    order = np.argsort(mix(seed, L), kind="stable")
    sizes = np.arange(1, L + 1, dtype=np.float64) * 0.25
    w = np.ones(L, dtype=np.int64)
    if pattern == "zero_trades":
        w[:] = 0
        sizes[3] = NAN                                            # the smallest size answers, not the NaN and not row 0
    elif pattern == "exact_cutoff":
        if L % 2:
            w[L - 1] = 2                                          # total L + 1: the cumulative weight of element (L + 1) / 2 - 1 is the cutoff
    elif pattern == "equal_run":
        sizes[L // 4:3 * L // 4] = 7.5                            # the cutoff falls inside the run
        w[:] = 1 + np.arange(L) % 3
    elif pattern == "nan_majority":
        sizes[L // 2 - 1:] = NAN
        w[L // 2 - 1:] = 3
    elif pattern == "all_nan":
        sizes[:] = NAN
    elif pattern == "neg_inf":
        sizes[0], w[0] = -INF, L
        sizes[1] = INF
    elif pattern == "pos_inf":
        sizes[L - 1], w[L - 1] = INF, L
        sizes[0] = -INF
    elif pattern == "neg_zero":
        sizes[:] = np.arange(L) - 1.0
        sizes[1], w[1] = -0.0, L                                  # -1 | -0.0 (the majority) | 1 2 ...
        sizes[2] = 0.0
    return sizes[order], w[order]


def _rs_median():
    groups = [(p, L) for p in MEDIAN_PATTERNS for L in MEDIAN_LENS]
    seg = _seg([L for _, L in groups])
    d = _rows(121, int(seg[-1]))
    for g, (p, L) in enumerate(groups):
        d["median_trade_size"][seg[g]:seg[g + 1]], d["trades"][seg[g]:seg[g + 1]] = _median_group(p, L, 130 + g)
    return seg, _cast(d, "v32w64")


def _rs_firstlast():
    lens = (3, 130, 2, 5, 2, 70, 4)
    seg = _seg(lens)
    d = _rows(141, int(seg[-1]))
    a = int(seg[1])
    d["open"][a:a + 65] = NAN                                     # the first open is row 65: the second 64-row chunk's second row
    d["close"][a + 65:a + 130] = NAN                              # the last close is row 64: the second chunk's first row
    d["open"][seg[3]:seg[4]] = NAN                                # no open at all between two valid groups: the row is dropped
    d["high"][seg[5]:seg[6]] = NAN                                # no high at all: NaN comes out, the row stays
    d["low"][seg[5]:seg[6] - 1] = NAN                             # the only low is the group's last row, in its second chunk
    return seg, _cast(d, "v32w64")


SUM_GROUPS = ("absorbed", "inf_then_numbers", "neg_inf_then_inf", "nan_volume", "nan_vwap", "zero_sum_inf", "zero_sum_nan", "all_nan_volume")


def _rs_sums(combo):
    big = 1e8 if combo[:3] == "v32" else 2.0 ** 53               # what one more 1.0 does not change in the column's dtype
    vols = {"absorbed": [big] + [1.0] * 200,
            "inf_then_numbers": [2.0, INF] + [3.0] * 70,          # the compensation turns NaN and is reset; the sum stays inf
            "neg_inf_then_inf": [1.0, -INF, 5.0, INF, 2.0],       # the sum itself is NaN from the fourth row on
            "nan_volume": [1.5, NAN, 2.5, NAN, 4.0],
            "nan_vwap": [1.5, 2.0, 2.5, 3.0, 4.0],
            "zero_sum_inf": [1.0, -1.0],
            "zero_sum_nan": [0.0, 0.0, 0.0],
            "all_nan_volume": [NAN, NAN]}
    seg = _seg([len(vols[k]) for k in SUM_GROUPS])
    d = _rows(151, int(seg[-1]))
    d["volume"] = np.concatenate([np.array(vols[k], dtype=np.float64) for k in SUM_GROUPS])
    g = SUM_GROUPS.index
    d["vwap"][seg[g("nan_vwap")]:seg[g("nan_vwap") + 1]] = [10.0, NAN, 20.0, NAN, 30.0]
    d["vwap"][seg[g("zero_sum_inf")]:seg[g("zero_sum_inf") + 1]] = [2.0, 1.0]
    return seg, _cast(d, combo)


RESAMPLE_CASES = {"resample.grid": _rs_grid, "resample.median": _rs_median, "resample.firstlast": _rs_firstlast}
for _c in COMBOS:
    RESAMPLE_CASES[f"resample.sizes.{_c}"] = functools.partial(_rs_sizes, _c)
    RESAMPLE_CASES[f"resample.sums.{_c}"] = functools.partial(_rs_sums, _c)


@functools.lru_cache(maxsize=None)
def rs_inputs(name):
    """-> (seg, (open, high, low, close, volume, trades, vwap, median)), read-only."""
    seg, d = RESAMPLE_CASES[name]()
    cols = tuple(np.ascontiguousarray(d[c]) for c in RS_COLS)
    for a in (seg,) + cols:
        a.setflags(write=False)
    return seg, cols


@functools.lru_cache(maxsize=None)
def rs_expected(name):
    seg, cols = rs_inputs(name)
    out = resample_groups(seg, *cols)
    for a in out:
        a.setflags(write=False)
    return out


def rs_frame(name):
    """The case as a bar frame that `index.floor("1D")` splits into the same groups: group g is day g, its rows a second apart."""
    import pandas as pd
    seg, cols = rs_inputs(name)
    lens = np.diff(seg)
    day = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    sec = np.arange(int(seg[-1]), dtype=np.int64) - np.repeat(seg[:-1], lens)
    assert lens.max() < 86_400
    idx = pd.DatetimeIndex((day * 86_400 + sec) * 1_000_000_000, name="timestamp")
    return pd.DataFrame(dict(zip(RS_COLS, cols)), index=idx), "1D"


def rs_check_structure(name, want):
    """The resampling cases' claims, on the inputs and the expectation."""
    seg, cols = rs_inputs(name)
    lens = np.diff(seg)
    info = {"groups": len(lens), "rows": int(seg[-1])}
    o, h, l, c, vol, tr, vw, med = cols
    if name == "resample.grid":
        assert len(lens) == GRID_GROUPS and set(lens) == {1, 2, 3}
        assert 0 < want[8].sum() < GRID_GROUPS and 0 < np.isnan(want[7]).sum() < GRID_GROUPS
        info.update(dropped=int((want[8] == 0).sum()))
    elif name.startswith("resample.sizes."):
        assert tuple(lens) == SIZES and vol.dtype == (np.float32 if "v32" in name else np.float64)
        assert vw.dtype == (np.float32 if "w32" in name else np.float64) and want[4].dtype == vol.dtype
    elif name == "resample.median":
        groups = [(p, L) for p in MEDIAN_PATTERNS for L in MEDIAN_LENS]
        assert min(MEDIAN_LENS) < 64 in MEDIAN_LENS and 65 in MEDIAN_LENS and tuple(lens) == tuple(L for _, L in groups)
        for g, (p, L) in enumerate(groups):
            sizes, w, got = med[seg[g]:seg[g + 1]], tr[seg[g]:seg[g + 1]], want[7][g]
            order = np.argsort(sizes, kind="stable")
            cum = np.cumsum(w[order])
            if p == "zero_trades":
                assert not w.any() and np.isnan(sizes).sum() == 1 and got == np.nanmin(sizes) == 0.25 and sizes[0] != got
            elif p == "exact_cutoff":
                k = int(np.searchsorted(cum, cum[-1] * 0.5, side="left"))
                assert cum[k] * 2 == cum[-1] and got == sizes[order][k] < sizes[order][k + 1]      # `>` would take the next one
            elif p == "equal_run":
                k = int(np.searchsorted(cum, cum[-1] * 0.5, side="left"))
                assert got == 7.5 and sizes[order][k - 1] == sizes[order][k + 1] == 7.5
            elif p == "nan_majority":
                assert w[np.isnan(sizes)].sum() * 2 > w.sum() and 0 < (~np.isnan(sizes)).sum() and np.isnan(got)
            elif p == "all_nan":
                assert np.isnan(sizes).all() and np.isnan(got)
            elif p == "neg_inf":
                assert got == -INF and (sizes == INF).any()
            elif p == "pos_inf":
                assert got == INF and (sizes == -INF).any()
            elif p == "neg_zero":
                assert got == 0.0 and (sizes < 0).any()
    elif name == "resample.firstlast":
        a = int(seg[1])
        assert want[0][1] == o[a + 65] and np.isnan(o[a:a + 65]).all() and want[3][1] == c[a + 64] and np.isnan(c[a + 65:a + 130]).all()
        assert list(want[8]) == [1, 1, 1, 0, 1, 1, 1] and np.isnan(want[0][3])
        assert np.isnan(want[1][5]) and want[8][5] == 1 and want[2][5] == l[seg[6] - 1] and lens[5] > 64
    elif name.startswith("resample.sums."):
        g = SUM_GROUPS.index
        T = vol.dtype.type
        with np.errstate(all="ignore"):
            a = vol[seg[g("absorbed")]:seg[g("absorbed") + 1]]
            plain = T(0)
            for v in a:
                plain = plain + v
            assert plain == a[0] and want[4][g("absorbed")] == T(float(a[0]) + 200.0) != plain       # Kahan recovers what `+` absorbs
        assert want[4][g("inf_then_numbers")] == INF and np.isnan(want[4][g("neg_inf_then_inf")])
        assert want[4][g("nan_volume")] == 8.0 and want[4][g("nan_vwap")] == 13.0 and np.isfinite(want[6][g("nan_vwap")])
        assert want[4][g("zero_sum_inf")] == 0.0 and want[6][g("zero_sum_inf")] == INF and np.isnan(want[6][g("zero_sum_nan")])
        assert want[4][g("all_nan_volume")] == 0.0 and np.isnan(want[6][g("all_nan_volume")])
    return info
