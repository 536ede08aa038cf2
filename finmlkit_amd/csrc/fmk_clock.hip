// fmk_clock.hip -- the bar-clock, run-length and opening-range features of the reference on resident series: BarDuration,
// BarDurationEWMA, BarRate, DirRunLen and ORBBreak (finmlkit/feature/transforms.py:1511-1548, :1460-1508, :1210-1270, :1605-1664,
// :1122-1207; there pandas' diff, ewm, a time-window rolling sum, a sequential loop and a Python loop per day).  DESIGN.md section 7i.
//
//   bar_duration       elementwise, one launch: (double)(ts[i] - ts[i - periods]) / 1e9, the division pandas does.
//                      Traffic: 8 + 8 (the lagged stamp, a cache hit for small lags) read, 8 written per row.
//   bar_duration_ewma  a specification for fmk_recur_core.h (K = 2, seed at element 1): the durations are formed from the stamps while
//                      loading and never stored.  Traffic: ts 8 read twice, 8 written per row.
//   bar_rate           lb(i), the first row inside the closed window [ts[i] - w, ts[i]], is monotone in i: the schedule of
//                      k_lagged_returns (fmk_ticklevel.hip) on int64 -- the lag of each tile's first row in a launch of its own, the
//                      slice [lb(first row), last row] staged once in LDS and bisected there, four consecutive rows per thread (the
//                      first bisects, the others gallop on from their predecessor); a slice longer than the stage takes the same
//                      per-row gallop and bisection on global memory, the first row of a thread starting from the tile's lag.
//                      Traffic: ts 8 (+ the window's overlap) read, 8 written.
//   dir_run_len        the last-head scan (fmk_lasthead.h) with the flag "this row starts a run"; int8 out.
//                      Traffic: x 8 read twice, 1 written per row.
//   orb_break          the last-head scan with the flag "this row's day differs from the row before"; the four opening rows of a day
//                      are gathers that the whole day shares (a thread keeps them while its rows stay in one day); two uint8 out.
//                      Traffic: ts 8 read twice, close 8 read, 2 written per row (+ 72 bytes of gathers per day and thread).
// Every output but bar_duration_ewma's is the reference's bits; that one is a recurrence scan (1e-9 relative, its NaN exact).
#include <math.h>

#include "fmk_common.h"
#include "fmk_lasthead.h"
#include "fmk_recur_core.h"

#define BR_TILE 1024                 // rows per workgroup of bar_rate (4 per thread)
#define BR_CAP 3072                  // int64 stamps staged in LDS (24 KB): the tile and its look-back
#define CK_DAY_NS 86400000000000LL
#define CK_MINUTE_NS 60000000000LL

namespace {

typedef long long ck_l2 __attribute__((ext_vector_type(2), aligned(8)));       // 16-byte accesses on an 8-byte alignment promise

// the thread's 8 consecutive stamps and the one in front of them (0 for what is not there)
__device__ __forceinline__ void ck_load_ts(const int64_t *__restrict__ ts, int64_t i0, int64_t n, bool whole, int64_t (&t)[8], int64_t *tp)
{
    if (whole) {
        const ck_l2 *q = (const ck_l2 *)(ts + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) { const ck_l2 v = q[k]; t[2 * k] = v.x; t[2 * k + 1] = v.y; }
        *tp = ts[i0 - 1];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = i0 + k < n ? ts[i0 + k] : 0;
        *tp = (i0 >= 1 && i0 - 1 < n) ? ts[i0 - 1] : 0;
    }
}

// pandas' total_seconds: asi8 / 10**9, a division
__device__ __forceinline__ double ck_seconds(int64_t ns) { return (double)ns / 1e9; }

// ---------------------------------------------------------------------------------------------------------------- bar_duration
__global__ __launch_bounds__(256) void k_bar_duration(const int64_t *__restrict__ ts, int64_t n, int64_t periods, double *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        // 0 <= i - periods <= n - 1 without forming i - periods first (any int64 is a valid periods)
        const bool there = periods <= i && periods >= i - (n - 1);
        out[i] = there ? ck_seconds(ts[i] - ts[i - periods]) : NAN;
    }
}

// ---------------------------------------------------------------------------------------------------------------- bar_duration_ewma
// ewma (fmk_recur.hip: RcEwma) over d[t] = seconds(ts[t] - ts[t-1]), seeded (d[1], 1) at element 1; element 0 is before the seed
struct RcDurEwma {
    static constexpr int K = 2;
    const int64_t *ts;
    double a;                        // 1.0 - alpha
    int64_t seed;                    // 1
    struct In { int64_t t[RC_ITEMS]; int64_t tp; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const { ck_load_ts(ts, i0, n, whole, in.t, &in.tp); }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const
    {
        const int p = j ? j - 1 : 0;
        x[0] = ck_seconds(in.t[j] - (j ? in.t[p] : in.tp));
        x[1] = 1.0;
    }
    __device__ __forceinline__ double lin(double x) const { return x; }
    __device__ __forceinline__ double step(double s, double x) const { return x + a * s; }
    __device__ __forceinline__ double emit(const double (&s)[K], const In &, int) const { return s[0] / s[1]; }
    __device__ __forceinline__ double before() const { return NAN; }
    __device__ __forceinline__ int64_t seed_lo() const { return 1; }
    __device__ __forceinline__ int64_t seed_hi() const { return 1; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { t[0] = ck_seconds(ts[i] - ts[i - 1]); t[1] = 1.0; }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &, const double (&t)[K]) const { s[0] = t[0]; s[1] = t[1]; }
    __device__ __forceinline__ void fin(double (&)[K], int64_t) const {}
};

// ---------------------------------------------------------------------------------------------------------------- bar_rate
// the first j in [0, i] with ts[j] >= target (ts[i] >= target), by backward gallop + bisection on global memory
__device__ __forceinline__ int64_t br_search_global(const int64_t *__restrict__ ts, int64_t i, int64_t target)
{
    int64_t hi = i;                          // f(hi) true
    int64_t step = 1, lo = i - 1;
    while (lo >= 0 && ts[lo] >= target) {
        hi = lo;
        step <<= 1;
        lo = i - step;
    }
    if (lo < 0) lo = -1;                     // f(-1) "false" sentinel
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ts[mid] >= target) hi = mid; else lo = mid;
    }
    return hi;
}

// the same j by forward gallop + bisection from `from` <= j: the caller knows that no row before `from` qualifies
__device__ __forceinline__ int64_t br_search_from(const int64_t *__restrict__ ts, int64_t from, int64_t i, int64_t target)
{
    int64_t lo = from - 1, hi = i;           // f(lo) false (or the sentinel), f(hi) true
    int64_t step = 1;
    while (lo + step < hi && ts[lo + step] < target) { lo += step; step <<= 1; }
    hi = lo + step < hi ? lo + step : hi;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ts[mid] >= target) hi = mid; else lo = mid;
    }
    return hi;
}

// lb of the first row of every tile (one thread per tile, all tiles in parallel): where the tile's LDS stage starts
__global__ __launch_bounds__(256) void k_br_tile_start(const int64_t *__restrict__ ts, int64_t w_ns, int64_t tiles, int64_t *__restrict__ tile_start)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tiles) return;
    const int64_t i = t * BR_TILE;
    tile_start[t] = br_search_global(ts, i, ts[i] - w_ns);
}

__global__ __launch_bounds__(256) void k_bar_rate(const int64_t *__restrict__ ts, int64_t n, double window_sec, int64_t w_ns,
                                                  const int64_t *__restrict__ tile_start, double *__restrict__ out)
{
    __shared__ int64_t s_ts[BR_CAP];
    const int64_t i_first = (int64_t)blockIdx.x * BR_TILE;
    const int64_t i_last = (i_first + BR_TILE < n ? i_first + BR_TILE : n) - 1;
    const int64_t r0 = tile_start[blockIdx.x];           // lb(first row of the tile): lb of every row of the tile is >= r0
    const int64_t len = i_last - r0 + 1;
    const bool staged = len <= BR_CAP;                   // uniform over the workgroup
    if (staged)
        for (int64_t k = threadIdx.x; k < len; k += 256) s_ts[k] = ts[r0 + k];
    __syncthreads();
    constexpr int PER = BR_TILE / 256;
    const int64_t i0 = i_first + (int64_t)threadIdx.x * PER;
    int prev = -1;                                       // staged offset of the previous row's lb (-1: none yet)
    int64_t far = -1;                                    // the previous row's lb on the global-memory path
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int64_t i = i0 + k;
        if (i > i_last) break;
        int64_t lb;
        if (staged) {
            const int64_t target = s_ts[i - r0] - w_ns;
            int lo = -1, hi = (int)(i - r0);             // staged offsets: f(lo) false (or the sentinel), f(hi) true
            if (prev >= 0) {
                // the target does not decrease along the rows: the answer is >= the previous row's, whose left neighbour is false
                lo = prev - 1;
                int step = 1;
                while (lo + step < hi && s_ts[lo + step] < target) { lo += step; step <<= 1; }
                hi = lo + step < hi ? lo + step : hi;
            }
            while (hi - lo > 1) {
                const int mid = lo + ((hi - lo) >> 1);
                if (s_ts[mid] >= target) hi = mid; else lo = mid;
            }
            prev = hi;
            lb = r0 + hi;
        } else {
            // from the tile's start, then from the previous row's answer: lb does not decrease along the rows
            lb = br_search_from(ts, far >= 0 ? far : r0, i, ts[i] - w_ns);
            far = lb;
        }
        out[i] = (double)(i - lb + 1) / window_sec * 3600.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- dir_run_len
// np.sign as a code: -1, 0, +1, and 2 for NaN (unequal to everything, itself included)
__device__ __forceinline__ int ck_sign(double x) { return x > 0.0 ? 1 : x < 0.0 ? -1 : x == 0.0 ? 0 : 2; }

struct LhRunLen {
    const double *x;
    int8_t *out;
    struct In { double x[LH_ITEMS]; double xp; int8_t r[LH_ITEMS]; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        rc_load8(x, i0, n, whole, in.x);
        in.xp = rc_prev(x, i0, n);
    }
    // a run starts at row 1, where the sign differs from the row before, and at every NaN; row 0 is outside every run
    __device__ __forceinline__ bool flag(const In &in, int j, int64_t i) const
    {
        if (i == 0) return false;
        const int p = j ? j - 1 : 0;
        const int s = ck_sign(in.x[j]), sp = ck_sign(j ? in.x[p] : in.xp);
        return i == 1 || s == 2 || s != sp;
    }
    __device__ __forceinline__ void emit(In &in, int j, int64_t i, int h) const
    {
        const bool counts = i >= 1 && ck_sign(in.x[j]) != 0;
        in.r[j] = counts ? (int8_t)(uint8_t)((uint32_t)((int)i - h + 1) & 0xFFu) : (int8_t)0;      // the low 8 bits, as the compiled store
    }
    __device__ __forceinline__ void finish(const In &in, int64_t i0, int64_t n, bool whole) const
    {
        if (whole && ((uintptr_t)(out + i0) & 7) == 0) {
            uint64_t w = 0;
#pragma unroll
            for (int j = 0; j < LH_ITEMS; ++j) w |= (uint64_t)(uint8_t)in.r[j] << (8 * j);
            *(uint64_t *)(out + i0) = w;
        } else {
#pragma unroll
            for (int j = 0; j < LH_ITEMS; ++j)
                if (i0 + j < n) out[i0 + j] = in.r[j];
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------- orb_break
// floor(ts / 86 400e9), also before 1970
__device__ __forceinline__ int64_t ck_day(int64_t t)
{
    const int64_t q = t / CK_DAY_NS;
    return q - ((t % CK_DAY_NS) < 0 ? 1 : 0);
}

struct LhOrb {
    const int64_t *ts;
    const double *high, *low, *close;
    uint8_t *o_long, *o_short;
    struct In {
        int64_t t[LH_ITEMS];
        int64_t tp;
        uint8_t lg[LH_ITEMS], sh[LH_ITEMS];
        int s;                       // the day start the opening range below belongs to (LH_NONE: none loaded)
        bool open;                   // that day starts in its first minute
        double hi, lo;               // the NaN-skipping max of high and min of low over rows s .. s+3 (NaN: all four are)
    };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        ck_load_ts(ts, i0, n, whole, in.t, &in.tp);
        in.s = LH_NONE;
    }
    __device__ __forceinline__ bool flag(const In &in, int j, int64_t i) const
    {
        const int p = j ? j - 1 : 0;
        return i == 0 || ck_day(in.t[j]) != ck_day(j ? in.t[p] : in.tp);
    }
    // row 0 is flagged: h is never LH_NONE here.  Rows s .. s+3 are read only where i - s >= 4: they exist.
    __device__ __forceinline__ void emit(In &in, int j, int64_t i, int h) const
    {
        uint8_t lg = 0, sh = 0;
        if ((int)i - h >= 4) {
            if (in.s != h) {
                const int64_t t0 = ts[h];
                in.s = h;
                in.open = t0 - ck_day(t0) * CK_DAY_NS < CK_MINUTE_NS;
                double hi = NAN, lo = NAN;
                if (in.open) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double a = high[h + k], b = low[h + k];
                        if (a == a && !(hi >= a)) hi = a;            // NaN skipped; the first number replaces the NaN
                        if (b == b && !(lo <= b)) lo = b;
                    }
                }
                in.hi = hi;
                in.lo = lo;
            }
            if (in.open) {
                const double c = close[i];
                lg = c > in.hi ? 1 : 0;                              // false for a NaN on either side
                sh = c < in.lo ? 1 : 0;
            }
        }
        in.lg[j] = lg;
        in.sh[j] = sh;
    }
    __device__ __forceinline__ void finish(const In &in, int64_t i0, int64_t n, bool whole) const
    {
        if (whole && (((uintptr_t)(o_long + i0) | (uintptr_t)(o_short + i0)) & 7) == 0) {
            uint64_t a = 0, b = 0;
#pragma unroll
            for (int j = 0; j < LH_ITEMS; ++j) {
                a |= (uint64_t)in.lg[j] << (8 * j);
                b |= (uint64_t)in.sh[j] << (8 * j);
            }
            *(uint64_t *)(o_long + i0) = a;
            *(uint64_t *)(o_short + i0) = b;
        } else {
#pragma unroll
            for (int j = 0; j < LH_ITEMS; ++j)
                if (i0 + j < n) { o_long[i0 + j] = in.lg[j]; o_short[i0 + j] = in.sh[j]; }
        }
    }
};

}  // namespace

extern "C" int fmk_bar_duration_dev(fmk_ctx *ctx, const int64_t *d_ts, int64_t n, int64_t periods, double *d_out)
{
    FMK_TRY(fmk_series_check(ctx, "bar_duration", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    k_bar_duration<<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>(d_ts, n, periods, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_bar_duration_ewma_dev(fmk_ctx *ctx, const int64_t *d_ts, int64_t n, double span, double *d_out)
{
    FMK_TRY(fmk_rule_ewma(ctx, span));
    FMK_TRY(fmk_series_check(ctx, "bar_duration_ewma", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    RcDurEwma sp;
    sp.ts = d_ts;
    sp.a = 1.0 - 2.0 / (span + 1.0);
    sp.seed = 1;
    return rc_scan(ctx, sp, n, d_out, NAN);
}

extern "C" int fmk_bar_rate_dev(fmk_ctx *ctx, const int64_t *d_ts, int64_t n, double window_sec, int64_t window_ns, double *d_out)
{
    FMK_TRY(fmk_rule_bar_rate(ctx, window_ns));
    FMK_TRY(fmk_series_check(ctx, "bar_rate", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    const int64_t tiles = fmk_ceil_div(n, BR_TILE);
    void *scr;
    FMK_TRY(fmk_scratch(ctx, (size_t)tiles * sizeof(int64_t), &scr));
    int64_t *tile_start = (int64_t *)scr;
    k_br_tile_start<<<(unsigned)fmk_ceil_div(tiles, 256), 256, 0, ctx->stream>>>(d_ts, window_ns, tiles, tile_start);
    FMK_LAUNCH_CHECK(ctx);
    k_bar_rate<<<(unsigned)tiles, 256, 0, ctx->stream>>>(d_ts, n, window_sec, window_ns, tile_start, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_dir_run_len_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int8_t *d_out)
{
    FMK_TRY(fmk_series_check(ctx, "dir_run_len", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    LhRunLen f;
    f.x = d_x;
    f.out = d_out;
    return lh_scan(ctx, f, n);
}

extern "C" int fmk_orb_break_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_high, const double *d_low, const double *d_close,
                                 int64_t n, uint8_t *d_orb_long, uint8_t *d_orb_short)
{
    FMK_TRY(fmk_series_check(ctx, "orb_break", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    LhOrb f;
    f.ts = d_ts;
    f.high = d_high; f.low = d_low; f.close = d_close;
    f.o_long = d_orb_long; f.o_short = d_orb_short;
    return lh_scan(ctx, f, n);
}

// Tile sizes of the kernels above, for tests that place their cases at tile edges: [0] the scans' tile (fmk_lasthead.h and
// fmk_recur_core.h agree), [1] their tiles per trip of the aggregate scan, [2] bar_rate's tile, [3] bar_rate's LDS stage in stamps.
extern "C" int fmk_clock_geometry(int64_t *out4)
{
    static_assert(LH_TILE == RC_TILE && LH_AGG_UNIT == RC_AGG_UNIT, "one tile for the scans of this file");
    out4[0] = LH_TILE;
    out4[1] = LH_AGG_UNIT;
    out4[2] = BR_TILE;
    out4[3] = BR_CAP;
    return FMK_OK;
}
