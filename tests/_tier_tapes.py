"""Tapes that put a volume / dollar bar call on ONE rung of its ladder (tests/test_gpu_threshold_tiers.py), the rung each was built
for, and a host model of the ladders as csrc/fmk_volume.hip (fmk_volume_bar_indexer_dev) and csrc/fmk_dollar.hip climb them.

Nothing here touches the GPU: the tapes come from seeded generators and integer arithmetic, the expected tier and tried mask are
LITERALS of the case tables (written from DESIGN.md section 6 and the comments of the ladder, not from a run), and
tests/test_threshold_tier_tapes.py checks on the host that every tape regenerates bit for bit, that its two estimates sit inside
the band of its rung and that the model of the ladder lands where the table says."""
import ctypes
import math
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np

# enum fmk_vol_tier of include/fmk_diag.h
E1024, E1536, E2048, LDS, LDS_TOTAL, GLOBAL, CHAIN, SERIAL, CACHED, P_SAMPLE, P_TOTAL = range(11)
N_TIERS = 11
TIER_NAMES = ("exact_1024", "exact_1536", "exact_2048", "lds_2048", "lds_2048_after_total", "global_tables", "chain_walk",
              "serial_walk", "cached", "sample_pass", "total_pass")
CLASSES = {E1024: (3072, 1024), E1536: (2560, 1536), E2048: (4096, 2048)}        # (S, W)
SAMPLE = 1 << 19
# the project's band limits (fmk_volume_bar_indexer_dev)
EST_E1024, EST_E1536, EST_EXACT, EST_LDS, MEAN_MISLED, MEAN_GLOBAL = 640.0, 1150.0, 1500.0, 1800.0, 1400.0, 65536.0
NEXT, BAD, REPLAY, NOCERT = 1, 2, 3, 4                                           # return codes of a tier that declines

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def read_volume_diag(lib):
    """fmk_diag_volume_last of include/fmk_diag.h (host bookkeeping of the library: reading it touches no device)"""
    tier, tried, listed = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    code = (ctypes.c_int64 * N_TIERS)()
    est, mean = ctypes.c_double(), ctypes.c_double()
    assert lib.fmk_diag_volume_last(ctypes.byref(tier), ctypes.byref(tried), code, ctypes.byref(est), ctypes.byref(mean),
                                    ctypes.byref(listed)) == 0
    return dict(tier=tier.value, tried=tried.value, codes=list(code), est_len=est.value, mean_len=mean.value, listed=listed.value)


def read_dollar_diag(lib):
    """fmk_diag_dollar_last + fmk_diag_dollar_source"""
    path, form, cached = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.fmk_diag_dollar_last(ctypes.byref(path)) == 0
    assert lib.fmk_diag_dollar_source(ctypes.byref(form), ctypes.byref(cached)) == 0
    return dict(path=path.value, closed_form=form.value, cached=cached.value)


def reached(d, tier) -> bool:
    """the ladder got as far as `tier`: it answered, or it was tried and declined"""
    return d["tier"] == tier or bool(d["tried"] >> tier & 1)


def mask(tried: Dict[int, int]) -> int:
    m = 0
    for t in tried:
        m |= 1 << t
    return m


def codes(tried: Dict[int, int]):
    return [tried.get(t, 0) for t in range(N_TIERS)]


def estimates(a, thr) -> Tuple[float, float]:
    """(est_len, mean_len) as the ladder defines them, from correctly rounded sums (math.fsum)."""
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    ns = min(n, SAMPLE)
    s, t = math.fsum(a[:ns]), math.fsum(a)
    return (ns * thr / s if s > 0.0 else 1e300), (n * thr / t if t > 0.0 else 1e300)


def bar_lengths_from_every_tick(a, thr):
    """L[i]: ticks of the bar that starts right behind tick i (the smallest k >= 1 with a[i+1] + .. + a[i+k] >= thr; n + 1 where it
    never closes) -- what the table kernels compute for EVERY tick, on or off the chain.  Exact for dyadic amounts; for others the
    float64 prefix differences are good to ~1e-12, far inside the room the tapes leave."""
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    P = np.concatenate(([0.0], np.cumsum(a)))                # P[k] = a[0] + .. + a[k-1]
    m = np.searchsorted(P, P[1:] + thr, side="left")          # tick i: smallest m with P[m] >= P[i+1] + thr; close tick m - 1
    L = (m - 1 - np.arange(n)).astype(np.int64)
    L[m > n] = n + 1
    return L


def overflows(a, thr, W, L=None) -> bool:
    """Does a table tier of span W decline this tape (return code 1)?  k_vx_level0 / k_vol_level0: some tick's bar does not close within
    W ticks although W ticks of data remain behind it; or the first bar (which counts tick 0: logic.py:107) is longer than W."""
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    if L is None:
        L = bar_lengths_from_every_tick(a, thr)
    i = np.arange(n)
    if np.any((L > W) & (i + 1 + W <= n)):
        return True
    return n >= W and float(np.sum(a[:W])) < thr


def longest_closed_bar_from_any_tick(L, n) -> int:
    ok = L <= n
    return int(L[ok].max()) if ok.any() else 0


def model(a, thr, certifies: bool, bad_in_sample: Optional[str] = None, bad_anywhere: bool = False, serial: bool = False):
    """The ladder of fmk_volume_bar_indexer_dev on the host: (tier, tried).  Replays are taken to agree (code 3 is a table literal
    only); `certifies`: every window passes the exact-sum certificate; bad_in_sample: None, 'neg' or 'nan'."""
    tried: Dict[int, int] = {}
    if serial or not (thr > 0.0):
        return SERIAL, tried
    a = np.asarray(a, dtype=np.float64)
    n = len(a)
    if bad_in_sample:
        tried[P_SAMPLE] = BAD
    est, mean = estimates(np.nan_to_num(a, nan=0.0), thr)
    if bad_in_sample == "nan":
        est = 1e300                                            # the sample's total is NaN
    L = None if bad_anywhere else bar_lengths_from_every_tick(a, thr)
    rc = NEXT

    def vx(t):
        if bad_anywhere:
            return BAD
        if not certifies:
            return NOCERT
        return NEXT if overflows(a, thr, CLASSES[t][1], L) else 0

    if est < EST_EXACT:
        if est < EST_E1024:
            rc = vx(E1024)
            if rc:
                tried[E1024] = rc
            else:
                return E1024, tried
        if rc == NEXT and est < EST_E1536:
            rc = vx(E1536)
            if rc:
                tried[E1536] = rc
            else:
                return E1536, tried
        if rc == NEXT:
            rc = vx(E2048)
            if rc:
                tried[E2048] = rc
            else:
                return E2048, tried
        if rc == NOCERT:
            rc = NEXT
    if rc == NEXT and est < EST_LDS:
        rc = BAD if bad_anywhere else (NEXT if overflows(a, thr, 2048, L) else 0)
        if rc:
            tried[LDS] = rc
        else:
            return LDS, tried
    if rc == NEXT:
        if bad_anywhere:
            tried[P_TOTAL] = BAD
            return SERIAL, tried
        if est >= EST_LDS and mean < MEAN_MISLED:
            if overflows(a, thr, 2048, L):
                tried[LDS_TOTAL] = NEXT
            else:
                return LDS_TOTAL, tried
        if mean < MEAN_GLOBAL:
            ls = 12
            while (1 << ls) < longest_closed_bar_from_any_tick(L, n):
                ls += 1
            if float(1 << ls) > 32.0 * mean or ls > 22:
                tried[GLOBAL] = NEXT
            else:
                return GLOBAL, tried
        return CHAIN, tried
    return SERIAL, tried


@dataclass
class VolCase:
    name: str
    make: Callable[[], Tuple[np.ndarray, float]]        # -> (amounts, threshold)
    tier: int                                           # the tier the tape was built for
    tried: Dict[int, int] = field(default_factory=dict)  # tier -> return code of every tier that declines on the way
    also: Tuple[int, ...] = ()                          # at the limit W itself: the tier is this one or one of these (recorded)
    certifies: bool = True
    bad_in_sample: Optional[str] = None
    bad_anywhere: bool = False
    serial: bool = False                                # taken out of the ladder (thr, FMK_THRESHOLD_SERIAL)
    env: Optional[Tuple[str, str]] = None
    model_skips: bool = False                           # the host model does not cover the code (a replay that disagrees)
    est_band: Optional[Tuple[float, float]] = None
    mean_band: Optional[Tuple[float, float]] = None
    listed: Optional[Tuple[int, int]] = None            # decisions listed before the replay, default mode: lo <= listed <= hi
    fast_reports: bool = False                          # the parallel mode must report an uncertified decision

    @property
    def id(self):
        return self.name


# ------------------------------------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------------------------------------
def dyadic_lots(seed, n, f64):
    """integers 1 .. 7 x 0.25 (mean exactly 1.0 in expectation), the first lot 1.0: est_len of a one-tick tape is thr itself"""
    a = np.random.default_rng(seed).integers(1, 8, n) * 0.25
    a[0] = 1.0
    return a.astype(np.float64 if f64 else np.float32)


def class_ns(t):
    S, W = CLASSES[t]
    return (1, W - 1, W, W + 1, S - 1, S, S + 1, 2 * S + 1, 16 * S + 1, 256 * S + 1)


CLASS_MEAN = {E1024: 100, E1536: 900, E2048: 1300}
CLASS_BAND = {E1024: (0.0, EST_E1024), E1536: (EST_E1024, EST_E1536), E2048: (EST_E1536, EST_EXACT)}


def class_alone_cases():
    """Each exact-sum class answers alone: est_len inside the class's own band, no bar near W."""
    out = []
    for t in (E1024, E1536, E2048):
        for f64 in (False, True):
            for n in class_ns(t):
                def make(t=t, f64=f64, n=n):
                    return dyadic_lots(100 + t, 256 * CLASSES[t][0] + 1, f64)[:n].copy(), float(CLASS_MEAN[t])
                out.append(VolCase(f"class_{TIER_NAMES[t]}_{'f64' if f64 else 'f32'}_n{n}", make, t, {}, est_band=CLASS_BAND[t]))
    return out


LOT = 4.0                      # the "unit" lot: 2^-4 lots are 1/64 of it, so one bar can hold up to 64 x bar quiet ticks


def quiet_tape(n, bar, start, stretch, f64=False):
    """`bar`-tick bars of unit lots (one lot = 4.0, thr = 4 bar) with ONE quiet stretch of `stretch` lots of 2^-4 from tick `start`.
    The chain bar that starts with the stretch is stretch + ceil(bar - stretch / 64) ticks long."""
    a = np.full(n, LOT, np.float64 if f64 else np.float32)
    a[start:start + stretch] = 0.0625
    return a, float(bar) * LOT


def stretch_for(bar, longest):
    """the stretch that makes the bar which starts with it exactly `longest` ticks long"""
    for q in range(longest, 0, -1):
        if q < 64 * bar and q + math.ceil(bar - q / 64.0) == longest:
            return q
    raise ValueError(longest)


HANDOFF_N = 150_000
BLOCK_EDGE = 61_440            # a multiple of 3072, 2560, 4096 and 2048: an edge of every tier's level-0 blocks


def handoff_cases():
    """One quiet stretch hands the call from class to class.  64-tick bars: mean_len ~ 64, so 32 x mean_len = 2048 < 4096 and a
    2 500-tick bar is left to the chain walk; 256-tick bars: 32 x 256 = 8192 >= 4096, the global tables keep it."""
    way = {1300: (E1536, {E1024: NEXT}),
           1800: (E2048, {E1024: NEXT, E1536: NEXT}),
           2500: (None, {E1024: NEXT, E1536: NEXT, E2048: NEXT, LDS: NEXT})}
    out = []
    for longest, (tier, tried) in way.items():
        for bar in ((64,) if tier is not None else (64, 256)):
            q = stretch_for(bar, longest)
            for where, start in (("first", 0), ("last", ((HANDOFF_N - longest - 2 * bar) // bar) * bar),
                                 ("edge", ((BLOCK_EDGE - q // 2) // bar) * bar)):
                tr = dict(tried)
                tt = tier
                if tt is None:
                    tt = GLOBAL if bar == 256 else CHAIN
                    if tt == CHAIN:
                        tr[GLOBAL] = NEXT
                out.append(VolCase(f"handoff_{longest}_bar{bar}_{where}", lambda bar=bar, start=start, q=q: quiet_tape(HANDOFF_N, bar, start, q),
                                   tt, tr, est_band=(0.0, EST_E1024)))
    return out


def limit_cases():
    """Longest bars of exactly W/2, W - 1, W and W + 1 ticks per class (64-tick bars, so class 1 is always the first tried).  Strict
    at <= W/2 (this class) and >= W + 1 (not this class); at W - 1 and W: this class or the next, recorded."""
    out = []
    before = {E1024: {}, E1536: {E1024: NEXT}, E2048: {E1024: NEXT, E1536: NEXT}}
    after = {E1024: (E1536, {E1024: NEXT}), E1536: (E2048, {E1024: NEXT, E1536: NEXT}),
             E2048: (CHAIN, {E1024: NEXT, E1536: NEXT, E2048: NEXT, LDS: NEXT, GLOBAL: NEXT})}
    next_rung = {E1024: E1536, E1536: E2048, E2048: LDS}
    start = ((BLOCK_EDGE + 5000) // 64) * 64
    # longest bar <= W/2, this class strictly.  Class 1: 64-tick bars.  Class 2: 700-tick bars put est_len in its own band (640 .. 1150)
    # and the longest is 768.  Class 3 has no such tape -- est_len >= 1150 means bars beyond W/2 = 1024, and below 1150 class 2 is
    # tried first and serves every bar up to 1536 -- so its strict case is a bar that class 2 refuses: 1600 ticks.
    out.append(VolCase("limit_exact_1024_inside_512", lambda: quiet_tape(HANDOFF_N, 64, start, stretch_for(64, 512)), E1024, {},
                       est_band=(0.0, EST_E1024)))
    out.append(VolCase("limit_exact_1536_inside_768", lambda: quiet_tape(HANDOFF_N, 700, 700 * 90, stretch_for(700, 768)), E1536, {},
                       est_band=(EST_E1024, EST_E1536)))
    out.append(VolCase("limit_exact_2048_inside_1600", lambda: quiet_tape(HANDOFF_N, 64, start, stretch_for(64, 1600)), E2048,
                       before[E2048], est_band=(0.0, EST_E1024)))
    for t in (E1024, E1536, E2048):
        W = CLASSES[t][1]
        for longest, kind in ((W - 1, "below"), (W, "at"), (W + 1, "beyond")):
            q = stretch_for(64, longest)
            if kind == "beyond":
                tier, tried, also = after[t][0], after[t][1], ()
            else:
                tier, tried, also = t, before[t], (next_rung[t],)
            out.append(VolCase(f"limit_{TIER_NAMES[t]}_{kind}_{longest}", lambda q=q: quiet_tape(HANDOFF_N, 64, start, q),
                               tier, tried, also=also, est_band=(0.0, EST_E1024)))
    return out


def refused_cases():
    """The exact-sum certificate is refused (code 4) by ONE class, the 2048-tick LDS tables answer; est_len ~ 300."""
    n = 50_000
    out = []

    def lognormal():
        a = np.random.default_rng(41).lognormal(0.0, 0.5, n)
        return a, float(np.mean(a)) * 300.0
    out.append(VolCase("refused_lognormal_f64", lognormal, LDS, {E1024: NOCERT}, certifies=False, est_band=(200.0, 450.0)))

    def mixed():
        rng = np.random.default_rng(42)
        a = rng.integers(1, 8, n) * 0.25
        k = rng.integers(0, n, 40)
        a[k[:20]] = 2.0 ** -20
        a[k[20:]] = 2.0 ** 12
        a = a.astype(np.float32)
        return a, float(np.mean(a, dtype=np.float64)) * 300.0
    out.append(VolCase("refused_f32_span_2^32", mixed, LDS, {E1024: NOCERT}, certifies=False, est_band=(200.0, 450.0)))
    for where, k in (("first", 5), ("middle", n // 2), ("last", n - 3)):
        def one64(k=k):
            a = dyadic_lots(43, n, True)
            a[k] = 1.0 + 2.0 ** -52                            # one full mantissa: quantum 2^-52, no float64 window of it certifies
            return a, 300.0
        out.append(VolCase(f"refused_one_f64_mantissa_{where}", one64, LDS, {E1024: NOCERT}, certifies=False, est_band=(200.0, 450.0)))

        def one32(k=k):
            a = dyadic_lots(44, n, False)
            a[k] = np.float32(2.0 ** -20)                      # quantum 2^-43: a window total of ~3000 is beyond 2^53 quanta
            return a, 300.0
        out.append(VolCase(f"refused_one_f32_tiny_{where}", one32, LDS, {E1024: NOCERT}, certifies=False, est_band=(200.0, 450.0)))
    return out


LDS_S = 2048                   # ticks per level-0 block of the LDS tables (vol_run)


def lds_tree_cases():
    """The tape of refused_lognormal_f64 at the edges of the LDS tier's table tree (csrc/fmk_voltree.h, radix 16): one block with and
    without a tail (no level above level 0), two and three blocks (one level), 17 blocks (two levels), 257 blocks (three)."""
    out = []
    for n in (LDS_S - 1, LDS_S, LDS_S + 1, 2 * LDS_S + 1, 16 * LDS_S + 1, 256 * LDS_S + 1):
        def make(n=n):
            a = np.random.default_rng(41).lognormal(0.0, 0.5, n)
            return a, float(np.mean(a)) * 300.0
        out.append(VolCase(f"lds_lognormal_n{n}", make, LDS, {E1024: NOCERT}, certifies=False, est_band=(200.0, 450.0)))
    return out


def global_cases():
    out = []
    # 3000-tick bars give tables of 4096 rows: n = 4097 is two blocks (one level above level 0), 16 * 4096 + 1 is 17 (two levels)
    for L, ns in ((3000, (4097, 16 * 4096 + 1, 70_001, 1_200_000)), (20_000, (70_001, 1_200_000)), (60_000, (70_001, 1_200_000))):
        for n in ns:
            def make(L=L, n=n):
                a = np.random.default_rng(50 + L // 1000).lognormal(0.0, 0.5, n)
                return a, L * (math.fsum(a) / n)
            out.append(VolCase(f"global_{L}_n{n}", make, GLOBAL, {}, certifies=False, est_band=(EST_LDS, 1e299),
                               mean_band=(MEAN_MISLED, MEAN_GLOBAL)))
    return out


def golden_case():
    """tests/golden/volume_total_tie_case.npz: threshold = the correctly rounded total, which the reference's running sum stays below.
    est_len = mean_len = n = 36 689: the global tables.  In the default mode vol_global_tables settles every fragile tick with the
    reference's own sum BEFORE the tables are built (k_vg_replay), so the one decision on the knife edge is decided there, nothing is
    left to list and the tables answer: no bar."""
    def golden():
        d = np.load(os.path.join(GOLDEN_DIR, "volume_total_tie_case.npz"))
        return d["a"], float(d["thr"])
    return [VolCase("global_golden_total_tie", golden, GLOBAL, {}, certifies=False, est_band=(EST_LDS, MEAN_GLOBAL),
                    mean_band=(MEAN_MISLED, MEAN_GLOBAL))]


def knife_tape(n, L, sigma, sign, seed0):
    """Lognormal float64 amounts and thr = the reference's own running sum at tick L: decision 1 is an exact tie for the reference,
    which closes at L.  sign -1 / +1: the first seed from seed0 whose EXACT sum of a[0 .. L] (math.fsum) lies at least 8 ulp below /
    above that float64 sum -- a tier that decides on near-exact sums then closes at L + 1 / at L; 0: any seed."""
    for seed in range(seed0, seed0 + 64):
        a = np.random.default_rng(seed).lognormal(0.0, sigma, n)
        thr = float(np.cumsum(a[:L + 1])[L])
        ulps = (math.fsum(a[:L + 1]) - thr) / float(np.spacing(thr))
        if sign == 0 or ulps * sign >= 8.0:
            return a, thr
    raise ValueError("no seed")


def knife_cases():
    """The first decision on a knife edge, per replaying tier.  The table tiers settle a fragile tick with the reference's own sum
    BEFORE the tables are built in the default mode (k_vol_level0 inline, k_vg_replay), clear its flag and so list nothing: no
    disagreement can reach vol_certify from them; the parallel mode lists the decision.  The chain walk decides on double-double
    block totals, lists the decision and k_vol_verify replays it: where the exact sum lies below the reference's, the walk closes one
    tick late, the replay disagrees (code 3) and the serial walk answers; where it lies above, the replay confirms."""
    return [VolCase("knife_lds_900", lambda: knife_tape(50_000, 900, 0.5, 0, 900), LDS, {E1536: NOCERT}, certifies=False,
                    est_band=(EST_E1024, EST_E1536), listed=(0, 0), fast_reports=True),
            VolCase("knife_global_9000", lambda: knife_tape(200_000, 9000, 0.5, 0, 910), GLOBAL, {}, certifies=False,
                    est_band=(EST_LDS, 1e299), mean_band=(MEAN_MISLED, MEAN_GLOBAL), listed=(0, 0), fast_reports=True),
            VolCase("knife_chain_replay_disagrees", lambda: knife_tape(400_000, 100_000, 0.5, -1, 920), SERIAL, {CHAIN: REPLAY},
                    certifies=False, model_skips=True, est_band=(EST_LDS, 1e299), mean_band=(MEAN_GLOBAL, 1e299), listed=(1, 8),
                    fast_reports=True),
            VolCase("knife_chain_replay_confirms", lambda: knife_tape(400_000, 100_000, 0.5, +1, 930), CHAIN, {}, certifies=False,
                    est_band=(EST_LDS, 1e299), mean_band=(MEAN_GLOBAL, 1e299), listed=(1, 8), fast_reports=True)]


def chain_cases():
    def long_bars():
        a = np.random.default_rng(61).lognormal(0.0, 0.5, 400_000)
        return a, 100_000 * (math.fsum(a) / len(a))

    def no_close():
        a = dyadic_lots(62, 50_000, False)
        return a, 2.0 * math.fsum(a.astype(np.float64))

    def last_tick_only():
        a = dyadic_lots(63, 100_000, False)                    # dyadic: the total is exact, the reference's sum reaches it on the last tick
        return a, math.fsum(a.astype(np.float64))
    band = dict(est_band=(EST_LDS, 1e299), mean_band=(MEAN_GLOBAL, 1e299))
    return [VolCase("chain_100000_n400000", long_bars, CHAIN, {}, certifies=False, **band),
            VolCase("chain_no_close", no_close, CHAIN, {}, **band),
            VolCase("chain_only_close_is_the_last_tick", last_tick_only, CHAIN, {}, **band)]


def misled_cases():
    n = 1 << 21

    def short_after_all():
        a = np.full(n, 4.0, np.float32)
        a[:SAMPLE] = 1.0
        return a, 2000.0

    def mirror():
        a = np.ones(n, np.float32)
        a[:SAMPLE] = 50.0
        return a, 5000.0
    return [VolCase("misled_head_2000_mean_615", short_after_all, LDS_TOTAL, {}, est_band=(EST_LDS, 1e299), mean_band=(0.0, MEAN_MISLED)),
            VolCase("misled_mirror_head_100_tail_5000", mirror, GLOBAL, {E1024: NEXT, E1536: NEXT, E2048: NEXT, LDS: NEXT},
                    est_band=(0.0, EST_E1024), mean_band=(0.0, MEAN_MISLED))]


def serial_cases():
    out = []
    for name, thr in (("zero", 0.0), ("negative", -5.0), ("nan", float("nan"))):
        out.append(VolCase(f"serial_thr_{name}", lambda thr=thr: (dyadic_lots(70, 30_000, False), thr), SERIAL, {}, serial=True))
    out.append(VolCase("serial_env", lambda: (dyadic_lots(71, 30_000, False), 100.0), SERIAL, {}, serial=True,
                       env=("FMK_THRESHOLD_SERIAL", "1")))
    n = SAMPLE + 5000
    for f64 in (False, True):
        d = "f64" if f64 else "f32"

        def neg_in(f64=f64):
            a = dyadic_lots(72, n, f64)
            a[1000] = -0.5
            return a, 100.0
        out.append(VolCase(f"serial_negative_in_sample_{d}", neg_in, SERIAL, {P_SAMPLE: BAD, E1024: BAD}, bad_in_sample="neg",
                           bad_anywhere=True, est_band=(0.0, EST_E1024)))

        def nan_in(f64=f64):
            a = dyadic_lots(73, n, f64)
            a[1000] = np.nan
            return a, 100.0
        out.append(VolCase(f"serial_nan_in_sample_{d}", nan_in, SERIAL, {P_SAMPLE: BAD, P_TOTAL: BAD}, bad_in_sample="nan", bad_anywhere=True))

        def neg_last(f64=f64):
            a = dyadic_lots(74, n, f64)
            a[-1] = -0.5
            return a, 100.0
        out.append(VolCase(f"serial_negative_last_tick_{d}", neg_last, SERIAL, {E1024: BAD}, bad_anywhere=True, est_band=(0.0, EST_E1024)))

        def nan_last(f64=f64):
            a = dyadic_lots(75, n, f64)
            a[-1] = np.nan
            return a, 100.0
        out.append(VolCase(f"serial_nan_last_tick_{d}", nan_last, SERIAL, {E1024: BAD}, bad_anywhere=True, est_band=(0.0, EST_E1024)))

    def nan_last_long():
        a = np.random.default_rng(76).lognormal(0.0, 0.5, n)
        thr = 5000 * (math.fsum(a) / n)
        a[-1] = np.nan
        return a, thr
    out.append(VolCase("serial_nan_last_tick_met_by_the_total_pass", nan_last_long, SERIAL, {P_TOTAL: BAD}, bad_anywhere=True,
                       certifies=False, est_band=(EST_LDS, 1e299)))

    def tenths():
        return np.full(400_000, 0.1), 6000.0
    # lots of 0.1 with a round threshold: EVERY tick starts a bar that hits 6000 exactly in exact arithmetic and misses it by an ulp or two
    # in float64, k_vg_nxt marks every one fragile, and vol_global_tables prices their replay (fragile ticks x mean_len additions)
    # above the serial walk (24 000 additions' worth per tick): code 3 without a replay having run
    out.append(VolCase("serial_replay_dearer_than_the_walk", tenths, SERIAL, {GLOBAL: REPLAY}, certifies=False, model_skips=True,
                       est_band=(EST_LDS, MEAN_GLOBAL), mean_band=(MEAN_MISLED, MEAN_GLOBAL)))
    return out


def volume_cases():
    return (class_alone_cases() + handoff_cases() + limit_cases() + refused_cases() + lds_tree_cases() + global_cases() + golden_case() + knife_cases() + chain_cases() + misled_cases()
            + serial_cases())


# ------------------------------------------------------------------------------------------------------------------------------
# dollar bars
# ------------------------------------------------------------------------------------------------------------------------------
ONEPASS, TWOPASS, NEITHER = 1, 2, 0
DL_TILE = 512 * 16


@dataclass
class DolCase:
    name: str
    make: Callable[[], Tuple[np.ndarray, np.ndarray, float]]   # -> (prices, amounts, threshold)
    path: int                                                   # fmk_diag_dollar_last
    closed_form: int                                            # fmk_diag_dollar_source
    fast_reports: bool = False                                  # the parallel mode must report an uncertified decision
    certain: bool = False                                       # integer tape: no decision within the drift bound (checked on the host)
    env: Optional[Tuple[str, str]] = None

    @property
    def id(self):
        return self.name


def integer_tape(seed, n):
    """integer lots 1 .. 3 at integer prices 4 .. 12 (a reflected +-1 walk): every product and every running sum is an integer"""
    rng = np.random.default_rng(seed)
    w = np.cumsum(rng.integers(-1, 2, n))
    px = 4.0 + np.abs((w + 4) % 16 - 8)                        # triangle wave of the walk: 4 .. 12
    am = rng.integers(1, 4, n).astype(np.float32)
    return px.astype(np.float64), am


CERTAIN_N = 130 * DL_TILE + 1
CERTAIN_FRAC = 2.0 ** -8


def certain_threshold():
    """K + 2^-8 with at most ~200 closes on the longest tape: m x thr is 2^-8 or more away from every integer for m < 256, hundreds of
    times the drift bound (1e-11 + 2.3e-16 per tick) x thr"""
    px, am = integer_tape(80, CERTAIN_N)
    return float(int(np.sum(px * am)) // 200) + CERTAIN_FRAC


def margin_of_certain_tape(px, am, thr, extra_ticks=0.0):
    """min over ticks of (distance of the exact running sum from the nearest multiple of thr) / (the drift bound at that tick)"""
    D = np.cumsum((px * am.astype(np.float64)).astype(np.int64))          # exact
    Tq = int(round(thr * 256))
    assert Tq == thr * 256
    r = (D * 256) % Tq
    dist = np.minimum(r, Tq - r) / 256.0
    bound = (1e-11 + 2.31e-16 * (np.arange(len(D)) + 1.0 + extra_ticks)) * thr
    return float(np.min(dist / bound))


def tenth_tape(seed, n):
    """tenth lots at prices 1 .. 4: products on a 0.1 grid, so with thr = 25 the exact sums hit multiples of thr every few hundred ticks
    while the float64 sums of the reference miss them by an ulp either way"""
    rng = np.random.default_rng(seed)
    w = np.cumsum(rng.integers(-1, 2, n))
    px = 1.0 + np.abs((w + 3) % 6 - 3)
    am = rng.integers(1, 10, n) / 10.0
    return px.astype(np.float64), am


def ticks_whose_bar_hits_the_threshold_exactly(a, thr):
    """tenth lots: ticks j for which some later prefix sum is EXACTLY thr above the prefix at j (in tenths)"""
    P = np.cumsum(np.rint(np.asarray(a) * 10).astype(np.int64))
    return int(np.count_nonzero(np.isin(P + int(round(thr * 10)), P)))


def exact_decimal_ties(px, am, thr):
    """ticks whose EXACT running sum (in tenths) is a multiple of thr"""
    D = np.cumsum(np.rint(px).astype(np.int64) * np.rint(am * 10).astype(np.int64))
    return int(np.count_nonzero(D % int(round(thr * 10)) == 0))


def dollar_cases():
    out = []
    thr0 = certain_threshold()
    for n in (2, DL_TILE - 1, DL_TILE, DL_TILE + 1, 64 * DL_TILE + 1, 65 * DL_TILE + 1, 130 * DL_TILE + 1):
        def make(n=n):
            px, am = integer_tape(80, CERTAIN_N)
            return px[:n].copy(), am[:n].copy(), thr0
        out.append(DolCase(f"path0_onepass_n{n}", make, 0, ONEPASS, certain=True))

    def one_tick():
        px, am = integer_tape(80, CERTAIN_N)
        return px[:1].copy(), am[:1].copy(), thr0
    out.append(DolCase("path0_twopass_n1", one_tick, 0, TWOPASS, certain=True))

    def one_block_trade():
        px, am = integer_tape(80, 200_000)
        px[77_777] = 8.0
        am[77_777] = np.float32(int(1.5 * thr0) // 8)          # one increment of ~1.5 thresholds: the one-pass form declines
        return px, am, thr0
    out.append(DolCase("path0_twopass_one_increment_above_thr", one_block_trade, 0, TWOPASS, certain=True))

    for n in (30_000, 400_000):
        def lognormal(n=n):
            rng = np.random.default_rng(90)
            px = 100.0 + 0.25 * np.abs(np.cumsum(rng.integers(-1, 2, n)))
            am = rng.lognormal(-1.0, 1.0, n)
            return px, am, float(np.cumsum(px * am)[1000])      # the reference's own running sum at tick 1000: decision 1 is an exact tie
        out.append(DolCase(f"path1_lognormal_n{n}", lognormal, 1, ONEPASS, fast_reports=True))
        out.append(DolCase(f"path1_tenths_n{n}", lambda n=n: tenth_tape(91, n) + (25.0,), 1, ONEPASS, fast_reports=True))

    out.append(DolCase("path2_block_trades_n200000", None, 2, TWOPASS, env=("FMK_DL_FORCE_EXACT_TIER", "1")))   # make: needs the oracle's synth

    def negative():
        px, am = tenth_tape(92, 30_000)
        am[12_345] = -0.3
        return px, am, 25.0
    out.append(DolCase("path3_negative_amount", negative, 3, NEITHER))

    def nan_price():
        px, am = tenth_tape(93, 30_000)
        px[12_345] = np.nan
        return px, am, 25.0
    out.append(DolCase("path3_nan_price", nan_price, 3, NEITHER))
    out.append(DolCase("path3_thr_zero", lambda: tenth_tape(94, 30_000) + (0.0,), 3, NEITHER))
    out.append(DolCase("path3_thr_negative", lambda: tenth_tape(94, 30_000) + (-25.0,), 3, NEITHER))
    out.append(DolCase("path3_env_serial", lambda: tenth_tape(96, 30_000) + (25.0,), 3, NEITHER, env=("FMK_THRESHOLD_SERIAL", "1")))

    def whale():
        px, am = tenth_tape(95, 30_000)
        px[10_000] = 1.0
        am[10_000] = 600 * 25.0                                # 600 thresholds: beyond the exact tier's backlog limit of 500
        return px, am, 25.0
    out.append(DolCase("path3_whale_of_600_thresholds", whale, 3, TWOPASS, fast_reports=True))
    return out


def block_trade_tape(orc, n=200_000):
    """The construction of test_dollar_bars_with_block_trades_stay_on_the_parallel_path at a size that runs in seconds: the synthetic
    tape with 0.1 % of the ticks turned into block trades of 1.2 .. 9 thresholds."""
    ts, px, am, sd = orc.synth(42, 0, n)
    am = am.copy()
    rng = np.random.default_rng(5)
    idx = rng.integers(0, n, n // 1000)
    thr = float((am.astype(np.float64) * px).mean()) * 865.0
    k = 1.2 + (9.0 - 1.2) * rng.integers(0, 1025, len(idx)) / 1024.0
    am[idx] = (k * thr / px[idx]).astype(np.float32)
    return px, am, thr
