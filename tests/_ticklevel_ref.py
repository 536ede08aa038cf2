"""Plain sequential restatement of the reference's tick-level features -- comp_lagged_returns (feature/core/utils.py:12-64), ewms,
ewmst_mean0, ewmst and realized_vol (feature/core/volatility.py:9-219, 256-286) -- as loops over Python floats (IEEE float64, one
rounded operation each), operation for operation as the reference writes them (ewms: its `x ** 2` as the compiled reference has
it, x * x).  `exp` and `log` are libm's (math.exp, math.log, extended to the arguments on which Python raises): the reference
compiled by Numba calls libm, and that is the project's contract.

realized_vol is the one function whose restatement is not the reference's order of operations: the reference's sum over a window
is NumPy's pairwise sum when interpreted and a plain loop when compiled, so the restatement is the correctly rounded value,
sqrt(fsum(r * r over the non-NaN elements) / divisor), each square rounded to float64 as every implementation rounds it.

The module also holds the seeded tapes, in integer arithmetic so that every machine regenerates the same bits, and the table of
fixture cases (fixture_cases) that tools/gen_ticklevel_edges_golden.py records and the tests replay.  Reads nothing outside the
repository."""
import math
import sys

import numpy as np

from tests._label_ref import host_log
from tests._recur_ref import grid_walk, nan_canonical, sha256  # noqa: F401 -- part of this module's interface

WINDOW_MESSAGE = "The return window must be greater than zero."
RV_WINDOW_MESSAGE = "window must be at least 1"
NAN, INF = math.nan, math.inf

# the kernels' geometry (csrc/fmk_ticklevel.hip): what the lengths and windows of the cases are cut at
LR_TILE, LR_CAP = 1024, 3072          # ticks per workgroup of k_lagged_returns; timestamps its LDS stage holds
EW_ITEMS, EW_TILE = 8, 2048           # consecutive ticks per lane; ticks per workgroup of the scan
EW_GROUP = 256                        # tile maps per group of the hierarchical scan
RV_SMALL_W, RV_MAX_W = 640, 2048      # realized_vol: the two LDS kernels, the segment scans beyond
RV_REGION = {True: 256 * 9, False: 256 * 25}     # region elements per workgroup (window <= RV_SMALL_W: True)

BASE_NS = 1_700_000_000_000_000_000   # float64 spacing here: 256 ns
SMALL_BASE_NS = 1_000_000_000_000_000  # below 2^53: every timestamp exact in float64
DAY3_NS = 3 * 86_400 * 1_000_000_000
GAPS_NS = (0, 1, 1_000_000, 1_000_000_000)
LONG_RUN = 3100                       # equal timestamps in the long run of burst_tape: more than LR_CAP
LONG_TAPE = 6 * 1024                  # the shortest burst_tape that holds the long run


def host_exp(x):
    """math.exp extended the way glibc defines it: overflow -> +inf (Python raises there)."""
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def _div(a, b):
    """a / b as IEEE gives it (Python raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0 or b != b:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def input_hash(a):
    """sha256 over the bytes of a float64 or int64 column."""
    a = np.ascontiguousarray(a)
    return sha256(a.view(np.float64)) if a.dtype == np.int64 else sha256(a)


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN


# ------------------------------------------------------------------------------------------------ the five functions
def comp_lagged_returns(timestamps, close, return_window_sec, is_log):
    if return_window_sec <= 0:
        raise ValueError(WINDOW_MESSAGE)
    c = np.asarray(close, np.float64).tolist()
    n = len(c)
    out = np.full(n, np.nan)
    if n == 0:
        return out                     # (the reference raises IndexError here)
    ts = np.asarray(timestamps, np.int64).astype(np.float64)       # searchsorted(int64 array, float64 key) compares in float64
    w_ns = return_window_sec * 1e9
    start = int(np.searchsorted(ts, ts[0] + w_ns, side="left"))
    for i in range(start, n):
        lag = int(np.searchsorted(ts, ts[i] - w_ns, side="right")) - 1
        if 0 <= lag < i:
            if c[lag] != 0.0:
                q = _div(c[i], c[lag])
                out[i] = host_log(q) if is_log else q - 1.0
            else:
                out[i] = INF
    return out


def lag_index(timestamps, return_window_sec):
    """The lag index of every tick as comp_lagged_returns finds it, -1 where there is none (what the tests assert their
    constructions with)."""
    ts = np.asarray(timestamps, np.int64).astype(np.float64)
    w_ns = return_window_sec * 1e9
    lag = np.searchsorted(ts, ts - w_ns, side="right") - 1
    start = int(np.searchsorted(ts, ts[0] + w_ns, side="left"))
    idx = np.arange(len(ts))
    return np.where((idx >= start) & (lag >= 0) & (lag < idx), lag, -1)


def alpha_of(dt_ns, half_life):
    """volatility.py:178-182: dt = (t - t_prev) / 1e9; alpha = 1 - exp(-dt / half_life)."""
    dt = dt_ns / 1e9
    return 1.0 - host_exp(_div(-dt, half_life))


def ewmst(timestamps, y, half_life, sigma_floor=1e-12, state=None, final=None):
    """`state`: (V, V2, Sy, Syy) in front of tick 1 instead of zeros, `final`: a list that receives the state after the last tick --
    what a shard of a longer series enters with and leaves behind (the reference has neither)."""
    ts = np.asarray(timestamps, np.int64).tolist()
    ys = np.asarray(y, np.float64).tolist()
    n = len(ys)
    out = np.empty(n, np.float64)
    if n == 0:
        return out
    V, V2, Sy, Syy = state or (0.0, 0.0, 0.0, 0.0)
    last = ts[0]
    out[0] = NAN
    for i in range(1, n):
        alpha = alpha_of(ts[i] - last, half_life)
        last = ts[i]
        om = 1.0 - alpha
        yi = ys[i]
        V = alpha + om * V
        V2 = alpha * alpha + (om * om) * V2
        if yi != yi:
            Sy = om * Sy
            Syy = om * Syy
        else:
            Sy = alpha * yi + om * Sy
            Syy = alpha * yi * yi + om * Syy
        if V > 0.0:
            mean = Sy / V
            e2 = Syy / V
            var_raw = e2 - mean * mean
            denom = V - (V2 / V)
            var = var_raw * (V / denom) if (denom > 0.0 and var_raw > 0.0) else 0.0
            sigma = _sqrt(var)
            if sigma < sigma_floor:
                sigma = sigma_floor
            out[i] = sigma
        else:
            out[i] = NAN
    if final is not None:
        final[:] = [V, V2, Sy, Syy]
    return out


def ewmst_mean0(timestamps, y, half_life, sigma_floor=1e-12):
    ts = np.asarray(timestamps, np.int64).tolist()
    ys = np.asarray(y, np.float64).tolist()
    n = len(ys)
    out = np.empty(n, np.float64)
    if n == 0:
        return out
    U = V = 0.0
    last = ts[0]
    out[0] = NAN
    for i in range(1, n):
        alpha = alpha_of(ts[i] - last, half_life)
        last = ts[i]
        yt = ys[i]
        if yt != yt:
            U = (1.0 - alpha) * U
            V = (1.0 - alpha) * V
        else:
            U = alpha * (yt * yt) + (1.0 - alpha) * U
            V = alpha + (1.0 - alpha) * V
        var = U / V if V > 0.0 else NAN
        if var < 0.0:
            var = 0.0
        sigma = _sqrt(var)
        if sigma < sigma_floor:
            sigma = sigma_floor
        out[i] = sigma
    return out


def libm_square(x):
    """x ** 2 as the interpreted reference evaluates it: libm's pow(x, 2.0), which is not always the correctly rounded x * x."""
    return x ** 2


def ewms(y, span, square=None):
    """`square`: how the reference's three `** 2` are evaluated.  Compiled by Numba a power with a constant integer exponent is a
    multiplication, which is the contract and the default; the generator's gate passes libm_square, what the interpreted run does."""
    square = square or (lambda x: x * x)
    ys = np.asarray(y, np.float64).tolist()
    n = len(ys)
    out = np.full(n, np.nan)
    if span <= 1:
        return out
    alpha = 2.0 / (span + 1.0)
    om = 1.0 - alpha
    om2 = square(om)
    Sw = Sw2 = Sy = Sy2 = 0.0
    for t in range(n):
        yt = ys[t]
        nan = yt != yt
        Sw = om * Sw + (0.0 if nan else 1.0)
        Sw2 = om2 * Sw2 + (0.0 if nan else 1.0)
        if not nan:
            Sy = om * Sy + yt
            Sy2 = om * Sy2 + square(yt)
        else:
            Sy = om * Sy
            Sy2 = om * Sy2
        if Sw > 0.0:
            mean = Sy / Sw
            den = Sw - (Sw2 / Sw)
            if den > 0.0:
                var = (Sy2 / Sw - square(mean)) * Sw / den
                var = max(var, 0.0)                  # Python's max: a NaN that comes first stays
                out[t] = _sqrt(var)
    return out


def realized_vol(r, window, is_sample):
    """The correctly rounded value per window (see the module's text).  window 0: every window is empty, all NaN; a negative window
    is refused, as the product refuses it."""
    window = int(window)
    if window < 0:
        raise ValueError(RV_WINDOW_MESSAGE)
    r = np.asarray(r, np.float64)
    n = len(r)
    out = np.full(n, np.nan)
    if window == 0 or window > n:
        return out
    ok = ~np.isnan(r)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = np.where(ok, r * r, 0.0).tolist()       # zeros add nothing to an exact sum
    cnt = np.concatenate(([0], np.cumsum(ok))).tolist()
    for i in range(window - 1, n):
        valid = cnt[i + 1] - cnt[i + 1 - window]
        if valid > 1:
            out[i] = _sqrt(math.fsum(sq[i + 1 - window:i + 1]) / (valid - 1 if is_sample else valid))
    return out


def rv_outputs_per_workgroup(window):
    """T of k_realized_vol: the region a workgroup stages, less the window's halo."""
    return RV_REGION[window <= RV_SMALL_W] - (window - 1)


FUNCTIONS = {"lr": "comp_lagged_returns", "ewmst": "ewmst", "ewmst0": "ewmst_mean0", "ewms": "ewms", "rv": "realized_vol"}
GATED = ("lr", "ewmst", "ewmst0", "ewms")            # bit for bit against the reference; rv is bounded


def call(fn, inputs, args, mod=None):
    """One case on this module, or on `mod`, which has the reference's names."""
    mod = mod or sys.modules[__name__]
    return getattr(mod, FUNCTIONS[fn])(*inputs, *args)


# ------------------------------------------------------------------------------------------------ tapes, prices, returns
def _from_gaps(base, gaps):
    gaps = np.asarray(gaps, np.int64)
    gaps[0] = 0
    return base + np.cumsum(gaps)


def _burst_gaps(n, rng):
    """Runs of 1..40 equal timestamps; between two runs a gap drawn from GAPS_NS (0 joins them)."""
    lens = rng.integers(1, 41, n)
    kind = rng.integers(0, len(GAPS_NS), n)
    starts = np.cumsum(lens) - lens
    keep = starts < n
    gaps = np.zeros(n, np.int64)
    gaps[starts[keep]] = np.array(GAPS_NS, np.int64)[kind[keep]]
    return gaps


def burst_tape(n, seed, zero=(), day3=None, back=()):
    """n int64 timestamps from BASE_NS: runs of 1..40 equal timestamps, gaps from {0, 1 ns, 1 ms, 1 s}, two gaps of 3 days and,
    from LONG_TAPE ticks on, one run of LONG_RUN equal timestamps (placed by the seed).
    zero: (lo, hi) pairs, the ticks lo..hi inclusive get dt == 0; day3: the ticks that follow a 3-day gap instead of the seed's
    two; back: ticks whose timestamp steps back 1 ms."""
    rng = np.random.default_rng(seed)
    gaps = _burst_gaps(n, rng)
    p = int(rng.integers(8, 900))                     # drawn whatever n is
    if n >= LONG_TAPE:
        gaps[p + 1:p + LONG_RUN] = 0
        d = p + LONG_RUN + rng.integers(0, n - p - LONG_RUN, 2)      # behind the long run: it stays whole
    else:
        d = rng.integers(1, max(n, 2), 2)
    for i in d.tolist() if day3 is None else ():      # the seed's two gaps give way to what a case places
        if 0 < i < n:
            gaps[i] = DAY3_NS
    for lo, hi in zero:
        gaps[lo:hi + 1] = 0
    for i in day3 or ():
        gaps[i] = DAY3_NS
    for i in back:
        gaps[i] = -1_000_000
    return _from_gaps(BASE_NS, gaps)


def gap_tape(n, fill_ns, placed, base=BASE_NS):
    """n timestamps whose gaps are `fill_ns` except where `placed` says otherwise: (lo, hi, gap_ns) triples, the ticks lo..hi
    inclusive follow a gap of gap_ns; later triples overwrite earlier ones."""
    gaps = np.full(n, int(fill_ns), np.int64)
    for lo, hi, g in placed:
        gaps[lo:hi + 1] = g
    return _from_gaps(base, gaps)


def even_tape(n, gap_ns):
    return BASE_NS + np.arange(n, dtype=np.int64) * int(gap_ns)


def small_tape(n, seed):
    """burst_tape's runs and gaps from SMALL_BASE_NS, without the long run and the 3-day gaps: every timestamp below 2^53."""
    ts = _from_gaps(SMALL_BASE_NS, _burst_gaps(n, np.random.default_rng(seed)))
    assert n == 0 or ts[-1] < 1 << 53
    return ts


def tape(kind, n, arg, zero=(), day3=None, back=()):
    if kind == "burst":
        return burst_tape(n, arg, zero, day3, back)
    if kind == "small":
        return small_tape(n, arg)
    assert kind == "even"
    return even_tape(n, arg)


def equal_run_lengths(ts):
    """The length of the run of equal timestamps each tick belongs to."""
    ts = np.asarray(ts)
    edges = np.flatnonzero(np.concatenate(([True], ts[1:] != ts[:-1], [True])))
    return np.repeat(np.diff(edges), np.diff(edges))


def prices(n, seed, zero_at=(), nan_at=()):
    """The 0.01-grid walk with a zero price and a NaN price planted where a case asks for them."""
    px = grid_walk(max(n, 1), seed)[:n].copy()
    for i in zero_at:
        px[i] = 0.0
    for i in nan_at:
        px[i] = np.nan
    return px


def returns(n, seed, step=35, nan=(), inf_at=()):
    """One-step simple returns of the grid walk (two correctly rounded operations per element); NaN over the (lo, hi) ranges
    lo..hi-1, +inf at `inf_at`."""
    w = grid_walk(n + 1, seed, step)
    y = w[1:] / w[:-1] - 1.0
    for lo, hi in nan:
        y[lo:hi] = np.nan
    for i in inf_at:
        y[i] = np.inf
    return y


def quiet_returns(n, seed, nan=(), outlier_at=(), inf_at=()):
    """Returns of size 1e-5 (an integer of at most 3000 over 1e8) with the 25.0 outlier, NaN runs and inf a case asks for."""
    r = np.random.default_rng(seed).integers(-3000, 3001, n) / 1e8
    for lo, hi in nan:
        r[max(lo, 0):max(hi, 0)] = np.nan
    for i in outlier_at:
        r[i] = 25.0
    for i in inf_at:
        r[i] = np.inf
    return r


def lr_inputs(kind, n, arg, pseed, zero_at=(), nan_at=(), zero=(), day3=None):
    return tape(kind, n, arg, zero, day3), prices(n, pseed, zero_at, nan_at)


def ew_inputs(kind, n, arg, yseed, step=35, nan=(), inf_at=(), zero=(), day3=None, back=()):
    return tape(kind, n, arg, zero, day3, back), returns(n, yseed, step, nan, inf_at)


def ewms_inputs(n, yseed, nan=(), step=35):
    return (returns(n, yseed, step, nan),)


def rv_inputs(n, seed, nan=(), outlier_at=(), inf_at=()):
    return (quiet_returns(n, seed, nan, outlier_at, inf_at),)


BUILDERS = {"lr": lr_inputs, "ew": ew_inputs, "ewms": ewms_inputs, "rv": rv_inputs}


def build(source):
    """The inputs of a case from its recipe {"gen": name of BUILDERS, "args": [...], "kw": {...}}."""
    return BUILDERS[source["gen"]](*source["args"], **source.get("kw", {}))


# ------------------------------------------------------------------------------------------------ the table of cases
HALF_LIVES = (0.05, 5.0, 600.0, math.nextafter(2.0, 0.0), 1e-301, 1e301, INF)
ODD_HALF_LIVES = (0.0, -1.0)          # recorded only if the reference returns without raising
FLOORS = (1e-12, 0.0, 1e-3)
LR_LENGTHS = (1, 2, 1023, 1024, 1025, 2049, 3 * 1024 + 5)
LR_WINDOWS = (1e-7, 2.56e-7, 1e-3, 1.0, 60.0, 1e7)     # 1e7 s: longer than every tape
EW_LENGTHS = (1, 2, 7, 8, 9, 2047, 2048, 2049, 4097)
EWMS_SPANS = (2, 3, 20, 100_000)
RV_WINDOWS = (1, 2, 639, 640, 641, 2047, 2048, 2049, 4097)
N_EW = 4097
Y_NAN = {"lead": [(0, 40)], "at7": [(7, 8)], "at8": [(8, 9)], "at2047": [(2047, 2048)], "at2048": [(2048, 2049)],
         "across2048": [(2040, 2061)], "all": [(0, 1 << 30)]}
TAPE_PLACED = {"zero2040_2060": dict(zero=[(2040, 2060)]), "zero_tile": dict(zero=[(2048, 4095)]),
               "gap2047": dict(day3=[2047, 3000]), "gap2048": dict(day3=[2048, 3000]), "back2050": dict(back=[2050])}
RECORD_MAX = 9000                     # the interpreted reference runs cases up to this many ticks ...
RV_RECORD_WORK = 10_000_000           # ... and realized_vol, whose interpreted run walks every window, up to this many window elements


def _case(fn, gen, gen_args, args, **kw):
    return dict(fn=fn, source={"gen": gen, "args": list(gen_args), "kw": kw}, args=list(args))


def rv_lengths(window):
    if window <= RV_MAX_W:
        t = rv_outputs_per_workgroup(window)
        return sorted({window, window + 1, t - 1, t, t + 1, 2 * t + 1, window + t - 1, window + t})
    return [window, window + 1, 2 * window - 1, 2 * window, 2 * window + 1, 3 * window + 20]     # (the last: room for a long NaN run)


def rv_recorded(window, n):
    return n <= RECORD_MAX and (n - window + 1) * window <= RV_RECORD_WORK


def rv_plan(window, n):
    """Where a case of realized_vol holds its outlier, its NaN runs and its inf: a run of window + 3 NaN across the edge between
    the first two workgroups (windows above RV_MAX_W: across the first segment edge) where the series is long enough for it --
    the windows that follow it hold exactly 1 and exactly 2 valid elements -- and a short run there otherwise."""
    edge = rv_outputs_per_workgroup(window) if window <= RV_MAX_W else (2 * window if n >= 3 * window + 20 else window)
    kw = dict(nan=[], outlier_at=[], inf_at=[])
    if n >= 16:
        kw["outlier_at"] = [n // 3]
        kw["inf_at"] = [n - 3]
    if n > edge + window + 8:
        lo = edge - window // 2 - 1
        kw["nan"].append((lo, lo + window + 3))
    elif n > edge + 2:
        kw["nan"].append((edge - 1, edge + 1))
    if kw["nan"] and kw["outlier_at"] and kw["nan"][0][0] <= kw["outlier_at"][0] < kw["nan"][0][1]:
        kw["outlier_at"] = [kw["nan"][0][0] - 5]       # beside the run, not inside it
    return kw


def odd_prices_at(n=2100, seed=906, w=1e-3):
    """Where the odd-price case holds its two zero and its two NaN prices: ticks that other ticks lag onto (the last tick of a run
    of equal timestamps), near ticks 300 and 700 and on both sides of the tile edge at 1024."""
    lag = lag_index(burst_tape(n, seed), w)
    onto = np.unique(lag[lag >= 0])
    near = lambda x: int(onto[np.abs(onto - x).argmin()])
    before, after = int(onto[onto < LR_TILE].max()), int(onto[onto >= LR_TILE].min())
    return dict(zero_at=[near(300), before], nan_at=[near(700), after])


def fixture_cases():
    """name -> case, every one at most RECORD_MAX ticks: what the generator records and the GPU test replays."""
    out = {}
    # comp_lagged_returns: every length with the windows 1 ms and 1 s, every window at 1025 and 3077 ticks, on both tapes
    for kind, seed in (("burst", 901), ("small", 902)):
        for n in LR_LENGTHS:
            for w in LR_WINDOWS:
                if w in (1e-3, 1.0) or n in (1025, 3 * 1024 + 5):
                    for lg in (False, True):
                        out[f"lr.{kind}.n{n}.w{w!r}.{'log' if lg else 'simple'}"] = _case("lr", "lr", [kind, n, seed, 903], [w, lg])
    n = 6 * 1024 + 5                                  # the long run: staged and unstaged tiles in one call
    for lg in (False, True):
        out[f"lr.mixed.{'log' if lg else 'simple'}"] = _case("lr", "lr", ["burst", n, 904, 905], [1.0, lg])
        out[f"lr.odd_prices.{'log' if lg else 'simple'}"] = _case("lr", "lr", ["burst", 2100, 906, 907], [1e-3, lg], **odd_prices_at())
    for look in (2047, 2048, 2049):                   # the LDS stage's capacity, on the fourth tile
        out[f"lr.stage.look{look}"] = _case("lr", "lr", ["even", 4 * 1024 + 5, 1_000_000, 908], [(look - 0.5) * 1e-3, False])
    # ewmst / ewmst_mean0
    for fn in ("ewmst", "ewmst0"):
        for n in EW_LENGTHS:
            out[f"{fn}.length.n{n}"] = _case(fn, "ew", ["burst", n, 910, 911], [5.0, 1e-12], nan=[(0, min(n, 3))])
        for hl in HALF_LIVES + ODD_HALF_LIVES:
            out[f"{fn}.half_life.{hl!r}"] = _case(fn, "ew", ["burst", N_EW, 912, 913], [hl, 1e-12], nan=[(0, 40)])
        for fl in FLOORS:
            out[f"{fn}.floor.{fl!r}"] = _case(fn, "ew", ["burst", N_EW, 914, 915, 5], [5.0, fl])
        for tag, kw in TAPE_PLACED.items():
            out[f"{fn}.tape.{tag}"] = _case(fn, "ew", ["burst", N_EW, 916, 917], [5.0, 1e-12], **kw)
        for tag, runs in Y_NAN.items():
            out[f"{fn}.nan.{tag}"] = _case(fn, "ew", ["burst", N_EW, 918, 919], [5.0, 1e-12], nan=runs)
        out[f"{fn}.inf.even"] = _case(fn, "ew", ["even", N_EW, 1_000_000, 920], [5.0, 1e-12], inf_at=[100])
    # ewms
    for n in EW_LENGTHS:
        out[f"ewms.length.n{n}"] = _case("ewms", "ewms", [n, 930], [20], nan=[(0, min(n, 3))])
    for span in EWMS_SPANS + (0, 1):
        out[f"ewms.span.{span}"] = _case("ewms", "ewms", [N_EW, 931], [span], nan=[(0, 3)])
    for tag, runs in Y_NAN.items():
        out[f"ewms.nan.{tag}"] = _case("ewms", "ewms", [N_EW, 932], [20], nan=runs)
    # realized_vol
    for w in RV_WINDOWS:
        for n in rv_lengths(w):
            if rv_recorded(w, n):
                out[f"rv.w{w}.n{n}"] = _case("rv", "rv", [n, 940 + w % 50], [w, True], **rv_plan(w, n))
        out[f"rv.w{w}.short"] = _case("rv", "rv", [max(w - 1, 1), 941], [w, True])           # a window larger than n
    for w in (2, 640, 2048, 2049):
        n = rv_lengths(w)[-2]
        out[f"rv.w{w}.n{n}.population"] = _case("rv", "rv", [n, 942], [w, False], **rv_plan(w, n))
    out["rv.w0"] = _case("rv", "rv", [50, 943], [0, True])
    return out


def refused_cases():
    """Arguments the product refuses with ValueError."""
    return {"refused.lr_w0": _case("lr", "lr", ["small", 50, 950, 951], [0.0, False]),
            "refused.lr_w-1": _case("lr", "lr", ["small", 50, 950, 951], [-1.0, True]),
            "refused.rv_w-1": _case("rv", "rv", [50, 952], [-1, True])}
