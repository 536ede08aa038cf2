// fmk_order.hip -- the windowed order statistics of the reference on a resident float64 series: comp_burst_ratio and pct_change
// (feature/core/utils.py), roc and stoch_k (feature/core/momentum.py).  A median, a minimum and a maximum are selections, not sums:
// they have no evaluation order, so every output is the reference's bits on any schedule.  The arithmetic after the selection is
// one or two IEEE operations in the reference's order, nothing contracted (the build's -ffp-contract=off).  DESIGN.md section 7d.
//
//   burst ratio  W = x[i - window + 1 .. i]: NaN when W holds a NaN (np.median); med = the middle element of sorted W (odd window) or
//                (a + b) / 2.0 over the two middle ones (even); out = x[i] / med when med > 0, NaN otherwise
//   %K           lo = min(low[W]), hi = max(high[W]); out = (100.0 * (close[t] - lo)) / (hi - lo) when hi > lo, NaN otherwise and
//                when low or high holds a NaN in W
//   roc          ((p[i] - p[i - period]) / p[i - period]) * 100.0 for i >= period
//   pct_change   base = x[t - periods]: (x[t] - base) / base when base > 0, NaN otherwise
//
// Rolling median, windows up to ORD_SORT_WINDOW_MAX (k_burst_sorted): a workgroup owns ORD_TILE consecutive outputs and stages the
// span [t0 - window + 1, t1) they read in LDS as order-preserving 64-bit keys (MedKey<true>; every NaN becomes key 0, below -inf)
// with their positions in the span, and sorts the span once (bitonic, by key).  Every lane then walks the sorted POSITIONS from the
// smallest key upwards, all lanes at the same entry (one LDS word per four entries, a broadcast), and counts per output the entries
// whose position lies in that output's window; the step at which the count passes rank window / 2 (and (window - 1) / 2 for an
// even window) is the index of the median's key.  A wave leaves the walk when all its outputs have their ranks.  The NaN entries
// sort first, so a window holds a NaN iff one of the first entries (those with key 0) lies in it.
// Longer windows (k_burst_walk, correct for every window <= n): a workgroup owns ORD_WALK_TILE outputs, one per lane; the key of
// rank window / 2 is built bit by bit from the top, each bit by one count of the window's keys below the candidate; the counts walk
// the window by the lockstep walk of fmk_window.h, one output per lane.  One more walk gives the largest key below it (even windows).
// Rolling minimum / maximum (k_stoch): the same walk, over `low` and then over `high`.
#include <limits.h>

#include "fmk_common.h"
#include "fmk_median.h"
#include "fmk_window.h"

#define ORD_BLOCK 256                                    // lanes per workgroup
#define ORD_OPL 4                                        // sorted path: outputs per lane
#define ORD_TILE (ORD_BLOCK * ORD_OPL)                   // sorted path: outputs per workgroup
#define ORD_SPAN_MAX 4096                                // sorted path: entries in LDS (8 B key + 2 B position: 40 KiB, four workgroups per CU)
#define ORD_SORT_WINDOW_MAX (ORD_SPAN_MAX - ORD_TILE + 1)   // the longest window whose full tile fits
#define ORD_WALK_TILE ORD_BLOCK                          // walk kernels: outputs per workgroup, one per lane

namespace {

typedef MedKey<true> OK64;
typedef uint64_t okey_t;

// the key of a float64: order-preserving over the numbers, 0 for every NaN (below the key of -inf)
__device__ __forceinline__ okey_t ord_key(double v)
{
    const okey_t k = OK64::tokey((okey_t)__double_as_longlong(v));
    return v == v ? k : 0;
}

// ---------------------------------------------------------------------------------------------- rolling median, sorted span
struct BurstArgs {
    const double *x;
    double *out;
    int64_t n, window;
    int P;                                               // sorted path: entries sorted, a power of two >= the longest span
    int slab;                                            // walk path: LDS elements per staging
};

template <bool EVEN>
__device__ __forceinline__ void burst_step(unsigned p, const unsigned (&base)[ORD_OPL], unsigned w, unsigned k1, unsigned k2,
                                           unsigned (&cnt)[ORD_OPL], unsigned (&j1)[ORD_OPL], unsigned (&j2)[ORD_OPL])
{
#pragma unroll
    for (int r = 0; r < ORD_OPL; ++r) {
        cnt[r] += (p - base[r]) < w ? 1u : 0u;           // the entry lies in output r's window
        j2[r] += cnt[r] <= k2 ? 1u : 0u;                 // the steps before the count passes the rank: the index of that rank's entry
        if constexpr (EVEN) j1[r] += cnt[r] <= k1 ? 1u : 0u;
    }
}

template <bool EVEN>
__global__ __launch_bounds__(ORD_BLOCK) void k_burst_sorted(BurstArgs a)
{
    extern __shared__ okey_t ord_lds[];
    okey_t *key = ord_lds;
    uint16_t *pos = (uint16_t *)(ord_lds + a.P);
    const int tid = threadIdx.x, P = a.P;
    const int64_t t0 = a.window - 1 + (int64_t)blockIdx.x * ORD_TILE;
    const int64_t t1 = t0 + ORD_TILE < a.n ? t0 + ORD_TILE : a.n;
    const int64_t lo = t0 - (a.window - 1);              // the tile reads x[lo .. t1 - 1]
    const int len = (int)(t1 - lo);                      // <= P; the entries beyond are padding: the largest key, a position in no window
    for (int i = tid; i < P; i += ORD_BLOCK) {
        okey_t k = OK64::MAXK;
        unsigned p = 0xFFFFu;
        if (i < len) { k = ord_key(a.x[lo + i]); p = (unsigned)i; }
        key[i] = k;
        pos[i] = (uint16_t)p;
    }
    __syncthreads();
    // ascending bitonic sort by key; entries with equal keys may come in any order (only the key of a rank is read)
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = tid; q < (P >> 1); q += ORD_BLOCK) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                const okey_t ki = key[i], kl = key[l];
                const bool up = (i & k) == 0;
                if (up ? ki > kl : ki < kl) {
                    const uint16_t pi = pos[i], pl = pos[l];
                    key[i] = kl; key[l] = ki;
                    pos[i] = pl; pos[l] = pi;
                }
            }
            __syncthreads();
        }
    }
    // nn: the entries with key 0 (NaN), which come first
    int nn = 0;
    for (int step = P >> 1; step > 0; step >>= 1)
        if (nn + step <= len && key[nn + step - 1] == 0) nn += step;
    if (nn < len && key[nn] == 0) ++nn;

    const unsigned w = (unsigned)a.window, k2 = w >> 1, k1 = (w - 1) >> 1;
    unsigned base[ORD_OPL], cnt[ORD_OPL], j1[ORD_OPL], j2[ORD_OPL];
    bool nan[ORD_OPL];
#pragma unroll
    for (int r = 0; r < ORD_OPL; ++r) {
        base[r] = (unsigned)(r * ORD_BLOCK + tid);       // output r's window: span positions base .. base + w - 1
        nan[r] = false;
    }
    for (int j = 0; j < nn; ++j) {
        const unsigned p = pos[j];
#pragma unroll
        for (int r = 0; r < ORD_OPL; ++r) nan[r] = nan[r] || (p - base[r]) < w;
    }
    const int jstart = nn & ~3;                          // (the NaN entries walked again lie in windows that give NaN anyway)
    const int jend = (len + 3) & ~3;                     // <= P: P is a multiple of four
#pragma unroll
    for (int r = 0; r < ORD_OPL; ++r) {
        const bool live = t0 + base[r] < t1 && !nan[r];
        cnt[r] = live ? 0u : k2 + 1u;                    // nothing to find
        j1[r] = j2[r] = (unsigned)jstart;
    }
    for (int j = jstart; j < jend; j += 4) {
        if (((j - jstart) & 31) == 0) {
            bool done = true;
#pragma unroll
            for (int r = 0; r < ORD_OPL; ++r) done = done && cnt[r] > k2;
            if (__all(done)) break;
        }
        const uint64_t four = *(const uint64_t *)(pos + j);
        burst_step<EVEN>((unsigned)(four & 0xFFFFu), base, w, k1, k2, cnt, j1, j2);
        burst_step<EVEN>((unsigned)((four >> 16) & 0xFFFFu), base, w, k1, k2, cnt, j1, j2);
        burst_step<EVEN>((unsigned)((four >> 32) & 0xFFFFu), base, w, k1, k2, cnt, j1, j2);
        burst_step<EVEN>((unsigned)(four >> 48), base, w, k1, k2, cnt, j1, j2);
    }
#pragma unroll
    for (int r = 0; r < ORD_OPL; ++r) {
        const int64_t t = t0 + base[r];
        if (t >= t1) continue;
        double o = NAN;
        if (!nan[r] && j2[r] < (unsigned)len) {          // (a window without a NaN always finds its ranks among the len entries)
            double med = OK64::value(key[j2[r]]);
            if constexpr (EVEN) med = (OK64::value(key[j1[r]]) + med) / 2.0;
            if (med > 0.0) o = a.x[t] / med;
        }
        a.out[t] = o;
    }
}

// ---------------------------------------------------------------------------------------------- rolling median, any window
__global__ __launch_bounds__(ORD_BLOCK) void k_burst_walk(BurstArgs a)
{
    extern __shared__ okey_t ord_lds[];
    const int64_t t0 = a.window - 1 + (int64_t)blockIdx.x * ORD_WALK_TILE;
    const int64_t t1 = t0 + ORD_WALK_TILE < a.n ? t0 + ORD_WALK_TILE : a.n;
    const int64_t lo = t0 - (a.window - 1), span = t1 - lo;
    const bool restage = span > (int64_t)a.slab;         // more than one slab: every walk stages again
    const double *x = a.x;
    auto load = [x, lo](int64_t i) { return ord_key(x[lo + i]); };
    const int64_t k2 = a.window >> 1, k1 = (a.window - 1) >> 1;

    okey_t mn = OK64::MAXK;                              // the smallest key: 0 iff the window holds a NaN
    fmk_window_walk<ORD_BLOCK, 1>(ord_lds, span, a.window, a.slab, true, load, [&](int, okey_t k) { mn = k < mn ? k : mn; });
    // v2: the key of rank k2 = the largest v with count(key < v) <= k2, built from the top bit down
    okey_t v2 = 0;
    for (int b = 63; b >= 0; --b) {
        const okey_t cand = v2 | ((okey_t)1 << b);
        int64_t c = 0;
        fmk_window_walk<ORD_BLOCK, 1>(ord_lds, span, a.window, a.slab, restage, load, [&](int, okey_t k) { c += k < cand ? 1 : 0; });
        v2 = c <= k2 ? cand : v2;
    }
    okey_t v1 = v2;
    if (k1 != k2) {                                      // even window: rank k2 - 1 is v2 again when more than k1 keys lie below...
        int64_t c = 0;
        okey_t below = 0;                                // the largest key < v2
        fmk_window_walk<ORD_BLOCK, 1>(ord_lds, span, a.window, a.slab, restage, load, [&](int, okey_t k) {
            const bool lt = k < v2;
            c += lt ? 1 : 0;
            below = lt && k > below ? k : below;
        });
        v1 = c > k1 ? below : v2;                        // c keys below v2: ranks 0 .. c - 1; rank k1 is among them iff k1 < c
    }
    const int64_t t = t0 + threadIdx.x;
    if (t >= t1) return;
    double o = NAN;
    if (mn != 0) {
        double med = OK64::value(v2);
        if (k1 != k2) med = (OK64::value(v1) + med) / 2.0;
        if (med > 0.0) o = x[t] / med;
    }
    a.out[t] = o;
}

// ---------------------------------------------------------------------------------------------- %K: rolling minimum and maximum
struct StochArgs {
    const double *close, *low, *high;
    double *out;
    int64_t n, length;
    int slab;
};

__global__ __launch_bounds__(ORD_BLOCK) void k_stoch(StochArgs a)
{
    extern __shared__ double ord_f64[];
    const int64_t t0 = a.length - 1 + (int64_t)blockIdx.x * ORD_WALK_TILE;
    const int64_t t1 = t0 + ORD_WALK_TILE < a.n ? t0 + ORD_WALK_TILE : a.n;
    const int64_t lo0 = t0 - (a.length - 1), span = t1 - lo0;
    const double *low = a.low, *high = a.high;
    double lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    fmk_window_walk<ORD_BLOCK, 1>(ord_f64, span, a.length, a.slab, true, [low, lo0](int64_t i) { return low[lo0 + i]; },
                                  [&](int, double v) { nan = nan || v != v; lo = v < lo ? v : lo; });
    fmk_window_walk<ORD_BLOCK, 1>(ord_f64, span, a.length, a.slab, true, [high, lo0](int64_t i) { return high[lo0 + i]; },
                                  [&](int, double v) { nan = nan || v != v; hi = v > hi ? v : hi; });
    const int64_t t = t0 + threadIdx.x;
    if (t >= t1) return;
    double o = NAN;
    if (!nan && hi > lo) o = (100.0 * (a.close[t] - lo)) / (hi - lo);
    a.out[t] = o;
}

// ---------------------------------------------------------------------------------------------- roc, pct_change
template <bool ROC>
__global__ __launch_bounds__(256) void k_ord_lag(const double *__restrict__ x, int64_t n, int64_t lag, double *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double r = NAN;
        if (i >= lag) {
            const double c = x[i], b = x[i - lag];
            if constexpr (ROC) r = ((c - b) / b) * 100.0;
            else if (b > 0.0) r = (c - b) / b;
        }
        out[i] = r;
    }
}

}  // namespace

extern "C" int fmk_burst_ratio_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out)
{
    FMK_TRY(fmk_rule_window(ctx, nullptr, window));
    FMK_TRY(fmk_series_check(ctx, "comp_burst_ratio", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    if (window > n) return FMK_OK;
    const int64_t outputs = n - (window - 1);
    BurstArgs a;
    a.x = d_x; a.out = d_out; a.n = n; a.window = window; a.P = 0; a.slab = 0;
    if (window <= ORD_SORT_WINDOW_MAX) {
        const int64_t span = window - 1 + (outputs < ORD_TILE ? outputs : ORD_TILE);     // the longest span of a tile
        int P = 4;
        while (P < span) P <<= 1;
        a.P = P;
        const size_t lds = (size_t)P * (sizeof(okey_t) + sizeof(uint16_t));
        const unsigned tiles = (unsigned)fmk_ceil_div(outputs, ORD_TILE);
        if (window & 1) k_burst_sorted<false><<<tiles, ORD_BLOCK, lds, ctx->stream>>>(a);
        else k_burst_sorted<true><<<tiles, ORD_BLOCK, lds, ctx->stream>>>(a);
    } else {
        a.slab = fmk_slab(window, ORD_WALK_TILE);
        k_burst_walk<<<(unsigned)fmk_ceil_div(outputs, ORD_WALK_TILE), ORD_BLOCK, (size_t)a.slab * sizeof(okey_t), ctx->stream>>>(a);
    }
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_stoch_k_dev(fmk_ctx *ctx, const double *d_close, const double *d_low, const double *d_high, int64_t n, int64_t length,
                               double *d_out)
{
    FMK_TRY(fmk_rule_stoch_k(ctx, length));
    FMK_TRY(fmk_series_check(ctx, "stoch_k", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    FMK_TRY(fmk_nan_head(ctx, d_out, n, length));
    if (length > n) return FMK_OK;
    const int64_t outputs = n - (length - 1);
    StochArgs a;
    a.close = d_close; a.low = d_low; a.high = d_high; a.out = d_out; a.n = n; a.length = length;
    a.slab = fmk_slab(length, ORD_WALK_TILE);
    k_stoch<<<(unsigned)fmk_ceil_div(outputs, ORD_WALK_TILE), ORD_BLOCK, (size_t)a.slab * sizeof(double), ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_roc_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t period, double *d_out)
{
    FMK_TRY(fmk_rule_roc(ctx, period));
    FMK_TRY(fmk_series_check(ctx, "roc", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    k_ord_lag<true><<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>(d_x, n, period, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_pct_change_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t periods, double *d_out)
{
    FMK_TRY(fmk_rule_pct_change(ctx, periods));
    FMK_TRY(fmk_series_check(ctx, "pct_change", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    k_ord_lag<false><<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>(d_x, n, periods, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}
