// fmk_shape.hip -- four window statistics of the reference's transforms.py on a resident float64 series, each recomputed per window:
// KurtosisTransform (:900-933), TrendSlope (:936-988), HurstExponent (:1341-1397) and BiPowerVariation (:1551-1602).  O(n x window).
// The reference computes them with pandas' rolling.apply around scipy / numpy calls; the contract is its values within the measured
// tolerances of tests/golden/shape.json and its NaN positions exactly.  DESIGN.md section 7c3.
//
// A window that reads a NaN or an infinity gives NaN (pandas' rolling turns +-inf into NaN and wants a full window).  With w the window:
//   kurtosis  t >= w - 1 over x[t-w+1 .. t]: m = sum / w, m2 = sum((x-m)^2) / w, m4 = sum(((x-m)^2)^2) / w, out = m4 / (m2 * m2) - 3;
//             NaN where the w elements all compare equal (whatever fl(sum / w) is: a held price has no kurtosis), and 0 / 0 = NaN
//   slope     t >= w - 1 over y = ln x (x finite and > 0, NaN otherwise): out = atan(sum((p - (w-1)/2) * (y_p - mean y)) /
//             (w (w^2 - 1) / 12)) * (180 / pi), p = 0 .. w-1 (0 / 0 = NaN at w = 1)
//   hurst     t >= w - 1, w >= 9: for k in 1, 2, 4, 8 the population variance v_k of the w - k sums of k consecutive elements of
//             x[t-w+2 .. t]; tau_k = sqrt(v_k); all four > 0: (-1.5 ln tau_1 - 0.5 ln tau_2 + 0.5 ln tau_4 + 1.5 ln tau_8) / (5 ln 2),
//             NaN otherwise, and NaN where for some k the w - k staged sums D_k all compare equal (tau_k is 0 for the numbers held
//             here, whatever the rounded mean leaves).  x[t-w+1] enters no sum and still has to be finite.
//   bipower   t >= w over x[t-w .. t]: out = sqrt(pi / 2) * sum_{j = t-w+1 .. t} |x[j]| * |x[j-1]|
// Schedule: the lockstep window walk of fmk_window.h.  The loader makes every non-finite element NaN while it stages, so plain NaN
// propagation through the sums gives the NaN outputs.  Kurtosis, slope and hurst walk twice (sums, then sums about the lane's own
// means) and stage twice only when the span takes more than one slab; bipower walks once over products formed at staging.  A lane
// counts the elements it has taken for an output: the walk delivers a window's elements in ascending order, so the count is the
// position in the window (the slope's weight, and which of hurst's sums are whole yet).  Kurtosis and hurst compare, in the first
// walk, every word they take with the window's last one, which the lane reads for itself: the words themselves, never deviations.
#include <limits.h>

#include "fmk_common.h"
#include "fmk_log.h"
#include "fmk_window.h"

#define SHAPE_BLOCK 256              // lanes per workgroup
#ifndef SHAPE_OPL
#define SHAPE_OPL 4                  // outputs per lane of the 8-byte walks (kurtosis, slope, bipower)
#endif
#ifndef HURST_OPL
#define HURST_OPL 2                  // outputs per lane of the 32-byte walk: eight accumulators per output
#endif
#define SHAPE_TILE (SHAPE_BLOCK * SHAPE_OPL)
#define HURST_TILE (SHAPE_BLOCK * HURST_OPL)
#define HURST_MIN_WINDOW 9           // lag 8 needs one difference

namespace {

struct ShapeArgs {
    const double *x;
    double *out;
    int64_t n, window;
    int slab;                        // LDS words per staging
};

// hurst's staged word: the sums of the last 1, 2, 4 and 8 elements ending at an index
struct __attribute__((aligned(32))) HurstWord {
    double d1, d2, d4, d8;
};

__device__ __forceinline__ double shape_finite(double v) { return __builtin_isfinite(v) ? v : NAN; }

// the tile of workgroup blockIdx.x whose first output is `first` + blockIdx.x * TILE, over windows of `walk` staged words ending at
// the output: outputs t0 .. t1 - 1, staged words lo .. t1 - 1
template <int TILE>
struct ShapeTile {
    int64_t t0, t1, lo, span;
    __device__ __forceinline__ ShapeTile(const ShapeArgs &a, int64_t first, int64_t walk)
    {
        t0 = first + (int64_t)blockIdx.x * TILE;
        t1 = t0 + TILE < a.n ? t0 + TILE : a.n;
        lo = t0 - (walk - 1);
        span = t1 - lo;
    }
};

__global__ __launch_bounds__(SHAPE_BLOCK) void k_kurtosis(ShapeArgs a)
{
    extern __shared__ double shape_lds[];
    const ShapeTile<SHAPE_TILE> tl(a, a.window - 1, a.window);
    const double *x = a.x;
    const int64_t lo = tl.lo;
    auto load = [x, lo](int64_t i) { return shape_finite(x[lo + i]); };

    double s[SHAPE_OPL], m[SHAPE_OPL], q[SHAPE_OPL];                 // the sum, then the sum of d^4; the mean; the sum of d^2
    double last[SHAPE_OPL];                                          // the window's last element (first walk only)
    int same[SHAPE_OPL];                                             // elements of the window == the last (a NaN never is)
#pragma unroll
    for (int r = 0; r < SHAPE_OPL; ++r) {
        const int64_t t = tl.t0 + r * SHAPE_BLOCK + threadIdx.x;
        s[r] = 0.0;
        last[r] = t < tl.t1 ? load(t - lo) : 0.0;
        same[r] = 0;
    }
    fmk_window_walk<SHAPE_BLOCK, SHAPE_OPL>(shape_lds, tl.span, a.window, a.slab, true, load, [&](int r, double v) {
        s[r] += v;
        same[r] += v == last[r];
    });
    const double w = (double)a.window;
#pragma unroll
    for (int r = 0; r < SHAPE_OPL; ++r) { m[r] = s[r] / w; s[r] = 0.0; q[r] = 0.0; }
    fmk_window_walk<SHAPE_BLOCK, SHAPE_OPL>(shape_lds, tl.span, a.window, a.slab, tl.span > (int64_t)a.slab, load, [&](int r, double v) {
        const double d = v - m[r], d2 = d * d;
        q[r] += d2;
        s[r] += d2 * d2;
    });
#pragma unroll
    for (int r = 0; r < SHAPE_OPL; ++r) {
        const int64_t t = tl.t0 + r * SHAPE_BLOCK + threadIdx.x;
        if (t >= tl.t1) continue;
        const double m2 = q[r] / w, m4 = s[r] / w;
        // all equal: no kurtosis; 0 / 0 where the squares underflow
        a.out[t] = same[r] != (int)a.window ? m4 / (m2 * m2) - 3.0 : NAN;
    }
}

__global__ __launch_bounds__(SHAPE_BLOCK) void k_trend_slope(ShapeArgs a)
{
    extern __shared__ double shape_lds[];
    const ShapeTile<SHAPE_TILE> tl(a, a.window - 1, a.window);
    const double *x = a.x;
    const int64_t lo = tl.lo;
    auto load = [x, lo](int64_t i) {
        const double v = x[lo + i];
        return (v > 0.0 && v < INFINITY) ? fmk_log_host(v) : NAN;
    };

    double s[SHAPE_OPL], m[SHAPE_OPL];                               // the sum, then the weighted centred sum; the mean
    int cnt[SHAPE_OPL];                                              // elements taken: the position in the window
#pragma unroll
    for (int r = 0; r < SHAPE_OPL; ++r) s[r] = 0.0;
    fmk_window_walk<SHAPE_BLOCK, SHAPE_OPL>(shape_lds, tl.span, a.window, a.slab, true, load, [&](int r, double v) { s[r] += v; });
    const double w = (double)a.window, centre = (w - 1.0) / 2.0;
#pragma unroll
    for (int r = 0; r < SHAPE_OPL; ++r) { m[r] = s[r] / w; s[r] = 0.0; cnt[r] = 0; }
    fmk_window_walk<SHAPE_BLOCK, SHAPE_OPL>(shape_lds, tl.span, a.window, a.slab, tl.span > (int64_t)a.slab, load, [&](int r, double v) {
        s[r] += ((double)cnt[r] - centre) * (v - m[r]);
        cnt[r] += 1;
    });
    const double ssx = w * (w * w - 1.0) / 12.0;
#pragma unroll
    for (int r = 0; r < SHAPE_OPL; ++r) {
        const int64_t t = tl.t0 + r * SHAPE_BLOCK + threadIdx.x;
        if (t >= tl.t1) continue;
        a.out[t] = atan(s[r] / ssx) * (180.0 / M_PI);                // 0 / 0 at window 1
    }
}

__global__ __launch_bounds__(SHAPE_BLOCK) void k_bipower(ShapeArgs a, double scale)
{
    extern __shared__ double shape_lds[];
    const ShapeTile<SHAPE_TILE> tl(a, a.window, a.window);           // the first output is at t = window: lo >= 1
    const double *x = a.x;
    const int64_t lo = tl.lo;
    auto load = [x, lo](int64_t i) { return fabs(shape_finite(x[lo + i])) * fabs(shape_finite(x[lo + i - 1])); };

    double s[SHAPE_OPL];
#pragma unroll
    for (int r = 0; r < SHAPE_OPL; ++r) s[r] = 0.0;
    fmk_window_walk<SHAPE_BLOCK, SHAPE_OPL>(shape_lds, tl.span, a.window, a.slab, true, load, [&](int r, double v) { s[r] += v; });
#pragma unroll
    for (int r = 0; r < SHAPE_OPL; ++r) {
        const int64_t t = tl.t0 + r * SHAPE_BLOCK + threadIdx.x;
        if (t < tl.t1) a.out[t] = scale * s[r];
    }
}

// The walk is over the window's last w - 1 elements; word i holds the sums ending at x[i], and d1 also carries x[i-1]'s finiteness:
// every window that walks word i reads x[i-1] too, and the one that starts its walk at i has x[i-1] as the element that enters no sum.
// Five waves per SIMD is what 32 KiB of LDS per workgroup allows; asking for it keeps the first walk's last words and counts within
// 96 VGPRs.
__global__ __launch_bounds__(SHAPE_BLOCK) __attribute__((amdgpu_waves_per_eu(5))) void k_hurst(ShapeArgs a)
{
    extern __shared__ HurstWord hurst_lds[];
    const int64_t walk = a.window - 1;
    const ShapeTile<HURST_TILE> tl(a, a.window - 1, walk);           // lo = t0 - window + 2 >= 1
    const double *x = a.x;
    const int64_t lo = tl.lo;
    auto load = [x, lo](int64_t i) {
        const int64_t g = lo + i;                                    // g >= 1; a sum that reaches below 0 is one no window uses
        double e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = g - k >= 0 ? shape_finite(x[g - k]) : 0.0;
        HurstWord h;
        h.d1 = e[1] == e[1] ? e[0] : NAN;
        h.d2 = e[1] + e[0];
        h.d4 = (e[3] + e[2]) + h.d2;
        h.d8 = ((e[7] + e[6]) + (e[5] + e[4])) + h.d4;
        return h;
    };

    double s1[HURST_OPL], s2[HURST_OPL], s4[HURST_OPL], s8[HURST_OPL];   // the sums, then the sums of squared deviations
    double m1[HURST_OPL], m2[HURST_OPL], m4[HURST_OPL], m8[HURST_OPL];
    int cnt[HURST_OPL];                                              // words taken: lag k's sums are whole from the k-th word on
    HurstWord last[HURST_OPL];                                       // the window's last word, which every lag takes (first walk only)
    int e1[HURST_OPL], e2[HURST_OPL], e4[HURST_OPL], e8[HURST_OPL];  // the D_k of the window == the last one (a NaN never is)
#pragma unroll
    for (int r = 0; r < HURST_OPL; ++r) {
        const int64_t t = tl.t0 + r * SHAPE_BLOCK + threadIdx.x;
        s1[r] = 0.0; s2[r] = 0.0; s4[r] = 0.0; s8[r] = 0.0; cnt[r] = 0;
        e1[r] = 0; e2[r] = 0; e4[r] = 0; e8[r] = 0;
        last[r] = load(t < tl.t1 ? t - lo : 0);
    }
    fmk_window_walk<SHAPE_BLOCK, HURST_OPL>(hurst_lds, tl.span, walk, a.slab, true, load, [&](int r, HurstWord h) {
        const int c = cnt[r];
        const double t2 = s2[r] + h.d2, t4 = s4[r] + h.d4, t8 = s8[r] + h.d8;
        s1[r] += h.d1;
        s2[r] = c >= 1 ? t2 : s2[r];
        s4[r] = c >= 3 ? t4 : s4[r];
        s8[r] = c >= 7 ? t8 : s8[r];
        e1[r] += h.d1 == last[r].d1;
        e2[r] += c >= 1 && h.d2 == last[r].d2;
        e4[r] += c >= 3 && h.d4 == last[r].d4;
        e8[r] += c >= 7 && h.d8 == last[r].d8;
        cnt[r] = c + 1;
    });
    const double w = (double)a.window;
    const int iw = (int)a.window;
#pragma unroll
    for (int r = 0; r < HURST_OPL; ++r) {
        m1[r] = s1[r] / (w - 1.0); m2[r] = s2[r] / (w - 2.0); m4[r] = s4[r] / (w - 4.0); m8[r] = s8[r] / (w - 8.0);
        s1[r] = 0.0; s2[r] = 0.0; s4[r] = 0.0; s8[r] = 0.0; cnt[r] = 0;
    }
    fmk_window_walk<SHAPE_BLOCK, HURST_OPL>(hurst_lds, tl.span, walk, a.slab, tl.span > (int64_t)a.slab, load, [&](int r, HurstWord h) {
        const int c = cnt[r];
        const double e1 = h.d1 - m1[r], e2 = h.d2 - m2[r], e4 = h.d4 - m4[r], e8 = h.d8 - m8[r];
        const double t2 = s2[r] + e2 * e2, t4 = s4[r] + e4 * e4, t8 = s8[r] + e8 * e8;
        s1[r] += e1 * e1;
        s2[r] = c >= 1 ? t2 : s2[r];
        s4[r] = c >= 3 ? t4 : s4[r];
        s8[r] = c >= 7 ? t8 : s8[r];
        cnt[r] = c + 1;
    });
#pragma unroll
    for (int r = 0; r < HURST_OPL; ++r) {
        const int64_t t = tl.t0 + r * SHAPE_BLOCK + threadIdx.x;
        if (t >= tl.t1) continue;
        const double u1 = sqrt(s1[r] / (w - 1.0)), u2 = sqrt(s2[r] / (w - 2.0)), u4 = sqrt(s4[r] / (w - 4.0)), u8 = sqrt(s8[r] / (w - 8.0));
        double o = NAN;
        const bool varies = e1[r] != iw - 1 && e2[r] != iw - 2 && e4[r] != iw - 4 && e8[r] != iw - 8;   // no lag's sums all equal
        if (varies && u1 > 0.0 && u2 > 0.0 && u4 > 0.0 && u8 > 0.0)  // a NaN fails the comparison
            o = (-1.5 * log(u1) - 0.5 * log(u2) + 0.5 * log(u4) + 1.5 * log(u8)) / (5.0 * M_LN2);
        a.out[t] = o;
    }
}

// what every entry asks before a device is needed
int shape_check(fmk_ctx *ctx, const char *what, int64_t n, int64_t window)
{
    FMK_TRY(fmk_rule_window(ctx, what, window));
    return fmk_series_check(ctx, what, n);
}

ShapeArgs shape_args(const double *d_x, int64_t n, int64_t window, double *d_out, int slab)
{
    ShapeArgs a;
    a.x = d_x; a.out = d_out; a.n = n; a.window = window; a.slab = slab;
    return a;
}

}  // namespace

extern "C" int fmk_rolling_kurtosis_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out)
{
    FMK_TRY(shape_check(ctx, "rolling_kurtosis", n, window));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    if (window > n) return FMK_OK;
    const ShapeArgs a = shape_args(d_x, n, window, d_out, fmk_slab(window, SHAPE_TILE));
    const int64_t tiles = fmk_ceil_div(n - (window - 1), SHAPE_TILE);
    k_kurtosis<<<(unsigned)tiles, SHAPE_BLOCK, (size_t)a.slab * sizeof(double), ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_trend_slope_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out)
{
    FMK_TRY(shape_check(ctx, "trend_slope", n, window));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    if (window > n) return FMK_OK;
    const ShapeArgs a = shape_args(d_x, n, window, d_out, fmk_slab(window, SHAPE_TILE));
    const int64_t tiles = fmk_ceil_div(n - (window - 1), SHAPE_TILE);
    k_trend_slope<<<(unsigned)tiles, SHAPE_BLOCK, (size_t)a.slab * sizeof(double), ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_hurst_exponent_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out)
{
    FMK_TRY(shape_check(ctx, "hurst_exponent", n, window));
    FMK_TRY(fmk_rule_hurst(ctx, window));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    if (window > n) return FMK_OK;
    const ShapeArgs a = shape_args(d_x, n, window, d_out, fmk_slab32(window - 1, HURST_TILE));
    const int64_t tiles = fmk_ceil_div(n - (window - 1), HURST_TILE);
    k_hurst<<<(unsigned)tiles, SHAPE_BLOCK, (size_t)a.slab * sizeof(HurstWord), ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_bipower_variation_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out)
{
    FMK_TRY(shape_check(ctx, "bipower_variation", n, window));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    if (window >= n) return fmk_nan_head(ctx, d_out, n, n + 1);      // NaN everywhere
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window + 1));                // the first output is at t = window
    const ShapeArgs a = shape_args(d_x, n, window, d_out, fmk_slab(window, SHAPE_TILE));
    const int64_t tiles = fmk_ceil_div(n - window, SHAPE_TILE);
    k_bipower<<<(unsigned)tiles, SHAPE_BLOCK, (size_t)a.slab * sizeof(double), ctx->stream>>>(a, sqrt(M_PI / 2.0));
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}
