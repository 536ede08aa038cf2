// fmk_corr.hip -- rolling_price_volume_correlation of the reference (feature/core/correlation.py) on two resident float64 series:
// the Pearson correlation of the one-step price returns and the volumes over each window, recomputed per window.  O(n x window);
// the contract is the reference's own evaluation order, bit for bit (the build's -ffp-contract=off).  DESIGN.md section 7c2.
//
//   ret[0] = NaN; ret[i] = (price[i] - price[i-1]) / price[i-1] where neither price is NaN and price[i-1] != 0, NaN otherwise
//   out[t] = NaN for t < window (everywhere when window >= n) and where ret[t] or volume[t] is NaN; for the others, over the pairs
//   (ret[j], volume[j]), j = t - window + 1 .. t, that hold no NaN, in ascending j: cnt < 2 -> NaN; mr = sr / cnt, mv = sv / cnt;
//   cov += dr * dv, qr += dr * dr, qv += dv * dv with dr = ret - mr, dv = volume - mv; qr > 0 and qv > 0:
//   cov / (sqrt(qr) * sqrt(qv)) clamped to [-1, 1]; NaN otherwise.
//   4 <= t < 10 (so window <= 9), the reference's special case: up, incv, decv = no price[j+1] <= price[j], no volume[j+1] <=
//   volume[j], no volume[j+1] >= volume[j] over j = t - window + 1 .. t - 1; up and incv -> 1.0, else up and decv -> -1.0.
// Schedule: the lockstep window walk of fmk_window.h over 16-byte words {ret, volume}, CORR_OPL outputs per lane.  The loader forms
// ret while it stages and makes both halves of a pair with a NaN NaN, so that one comparison tells a valid pair.  Two walks, as the
// z-score's: sr, sv, cnt under a select, then cov, qr, qv against the lane's own means; staged twice only when the span takes more
// than one slab.  The special case is a launch of its own after the tiles: six lanes, at most eight steps each.
#include <limits.h>

#include "fmk_common.h"
#include "fmk_window.h"

#define CORR_BLOCK 256               // lanes per workgroup
#ifndef CORR_OPL
#define CORR_OPL 4                   // outputs per lane (independent float64 add chains)
#endif
#define CORR_TILE (CORR_BLOCK * CORR_OPL)
#define CORR_SPECIAL_LO 4            // the special case holds for CORR_SPECIAL_LO <= t < CORR_SPECIAL_HI
#define CORR_SPECIAL_HI 10

namespace {

struct CorrArgs {
    const double *price, *volume;
    double *out;
    int64_t n, window;
    int slab;                        // LDS words per staging
};

// ret[i], i >= 1
__device__ __forceinline__ double corr_ret(const double *__restrict__ price, int64_t i)
{
    const double c = price[i], b = price[i - 1];
    return (c == c && b == b && b != 0.0) ? (c - b) / b : NAN;
}

__global__ __launch_bounds__(CORR_BLOCK) void k_corr(CorrArgs a)
{
    extern __shared__ double2 corr_lds[];
    const int64_t t0 = a.window + (int64_t)blockIdx.x * CORR_TILE;
    const int64_t t1 = t0 + CORR_TILE < a.n ? t0 + CORR_TILE : a.n;
    const int64_t lo = t0 - (a.window - 1), span = t1 - lo;          // the tile reads pairs lo .. t1 - 1; lo >= 1
    const double *price = a.price, *volume = a.volume;
    auto load = [price, volume, lo](int64_t i) {
        const double r = corr_ret(price, lo + i), v = volume[lo + i];
        const bool ok = r == r && v == v;
        return make_double2(ok ? r : NAN, ok ? v : NAN);
    };

    double s0[CORR_OPL], s1[CORR_OPL], s2[CORR_OPL];                 // sr, sv, -; then cov, qr, qv
    double mr[CORR_OPL], mv[CORR_OPL];
    int cnt[CORR_OPL];
#pragma unroll
    for (int r = 0; r < CORR_OPL; ++r) { s0[r] = 0.0; s1[r] = 0.0; cnt[r] = 0; }
    fmk_window_walk<CORR_BLOCK, CORR_OPL>(corr_lds, span, a.window, a.slab, true, load, [&](int r, double2 w) {
        const bool ok = w.x == w.x;                                  // a pair with a NaN skipped by select
        const double sr = s0[r] + w.x, sv = s1[r] + w.y;
        s0[r] = ok ? sr : s0[r];
        s1[r] = ok ? sv : s1[r];
        cnt[r] += ok ? 1 : 0;
    });
#pragma unroll
    for (int r = 0; r < CORR_OPL; ++r) {
        const double c = (double)cnt[r];
        mr[r] = s0[r] / c;
        mv[r] = s1[r] / c;
        s0[r] = 0.0; s1[r] = 0.0; s2[r] = 0.0;
    }
    fmk_window_walk<CORR_BLOCK, CORR_OPL>(corr_lds, span, a.window, a.slab, span > (int64_t)a.slab, load, [&](int r, double2 w) {
        const bool ok = w.x == w.x;
        const double dr = w.x - mr[r], dv = w.y - mv[r];
        const double cov = s0[r] + dr * dv, qr = s1[r] + dr * dr, qv = s2[r] + dv * dv;
        s0[r] = ok ? cov : s0[r];
        s1[r] = ok ? qr : s1[r];
        s2[r] = ok ? qv : s2[r];
    });
#pragma unroll
    for (int r = 0; r < CORR_OPL; ++r) {
        const int64_t t = t0 + r * CORR_BLOCK + threadIdx.x;
        if (t >= t1) continue;
        const double rt = corr_ret(price, t), vt = volume[t];
        double o = NAN;
        if (rt == rt && vt == vt && cnt[r] >= 2 && s1[r] > 0.0 && s2[r] > 0.0) {
            o = s0[r] / (sqrt(s1[r]) * sqrt(s2[r]));
            o = o > 1.0 ? 1.0 : (o < -1.0 ? -1.0 : o);               // a NaN quotient stays NaN
        }
        a.out[t] = o;
    }
}

// the special case: lane k decides output max(window, CORR_SPECIAL_LO) + k, after the tiles have written it
__global__ __launch_bounds__(64) void k_corr_special(CorrArgs a)
{
    const int64_t t = (a.window > CORR_SPECIAL_LO ? a.window : CORR_SPECIAL_LO) + threadIdx.x;
    if (t >= CORR_SPECIAL_HI || t >= a.n) return;
    const double rt = corr_ret(a.price, t), vt = a.volume[t];
    if (rt != rt || vt != vt) return;                                // NaN at the current position comes first
    bool up = true, incv = true, decv = true;
    for (int64_t j = t - a.window + 1; j < t; ++j) {                 // j >= 1, j + 1 <= t < n
        const double p0 = a.price[j], p1 = a.price[j + 1], v0 = a.volume[j], v1 = a.volume[j + 1];
        if (p1 <= p0) up = false;
        if (v1 <= v0) incv = false;
        if (v1 >= v0) decv = false;
    }
    if (up && incv) a.out[t] = 1.0;
    else if (up && decv) a.out[t] = -1.0;
}

}  // namespace

extern "C" int fmk_price_volume_corr_dev(fmk_ctx *ctx, const double *d_price, const double *d_volume, int64_t n, int64_t window,
                                         double *d_out)
{
    FMK_TRY(fmk_rule_window(ctx, "rolling_price_volume_correlation", window));
    FMK_TRY(fmk_series_check(ctx, "rolling_price_volume_correlation", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    if (window >= n) return fmk_nan_head(ctx, d_out, n, n + 1);      // NaN everywhere
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window + 1));                // the first output is at t = window
    CorrArgs a;
    a.price = d_price; a.volume = d_volume; a.out = d_out; a.n = n; a.window = window;
    a.slab = fmk_slab16(window, CORR_TILE);
    const int64_t tiles = fmk_ceil_div(n - window, CORR_TILE);
    k_corr<<<(unsigned)tiles, CORR_BLOCK, (size_t)a.slab * sizeof(double2), ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    if (window < CORR_SPECIAL_HI && n > CORR_SPECIAL_LO) {
        k_corr_special<<<1, 64, 0, ctx->stream>>>(a);
        FMK_LAUNCH_CHECK(ctx);
    }
    return FMK_OK;
}
