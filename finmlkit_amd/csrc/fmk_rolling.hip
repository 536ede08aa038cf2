// fmk_rolling.hip -- the rolling-window moments of the reference on a resident float64 series: sma (feature/core/ma.py), comp_zscore
// (feature/core/utils.py), rolling_variance_nb and variance_ratio_1_4_core (feature/core/volatility.py).  O(n x window) float64
// additions; the contract is the reference's own evaluation order, bit for bit: every window is summed on its own, in ascending index
// order, one rounded addition per element, nothing contracted (the build's -ffp-contract=off).  DESIGN.md section 7c.
//
// Per output t >= window - 1 over x[t - window + 1 .. t]:
//   mean      out = (1.0 / window) * (x[..] + ... + x[t])                                  (the reciprocal rounded first)
//   variance  cnt, s, q over the non-NaN elements (q += v * v); cnt >= min_periods and cnt > ddof: m = s / cnt,
//             v = q / cnt - m * m, v *= cnt / (cnt - ddof), out = max(0.0, v); otherwise NaN
//   z-score   mean = sum / window, var = sum((x - mean)^2) / (window - ddof), std = sqrt(var), out = (x[t] - mean) / std, NaN when
//             std == 0 (a NaN std divides through)
// Schedule: the lockstep window walk of fmk_window.h, ROLL_OPL outputs per lane: that many independent add chains.  The z-score walks
// twice (the sum, then the squared deviations from the lane's own mean) and stages twice only when the span takes more than one slab.
// The variance ratio is r1 (one-step log or simple returns, the host's log: fmk_log.h) and r4 (four of them added, newest first) by
// two elementwise kernels, the variance mode on both, and a kernel for the quotient.
#include <limits.h>

#include "fmk_common.h"
#include "fmk_log.h"
#include "fmk_window.h"

#define ROLL_BLOCK 256               // lanes per workgroup
#ifndef ROLL_OPL
#define ROLL_OPL 4                   // outputs per lane: the tuning knob (independent float64 add chains)
#endif
#define ROLL_TILE (ROLL_BLOCK * ROLL_OPL)

namespace {

enum { ROLL_MEAN = 0, ROLL_VAR = 1, ROLL_Z = 2 };

struct RollArgs {
    const double *x;
    double *out;
    int64_t n, window;
    int64_t ddof, min_periods;       // variance
    double scale;                    // mean: 1.0 / window; z-score: (double)window
    double denom;                    // z-score: (double)(window - ddof)
    int slab;                        // LDS elements per staging
};

struct RollState {
    double s[ROLL_OPL];              // the sum (z-score, second walk: the sum of squared deviations)
    double q[ROLL_OPL];              // variance: the sum of squares; z-score: the mean
    int cnt[ROLL_OPL];               // variance: non-NaN elements
};

template <int MODE>
__global__ __launch_bounds__(ROLL_BLOCK) void k_roll(RollArgs a)
{
    extern __shared__ double roll_lds[];
    const int64_t t0 = a.window - 1 + (int64_t)blockIdx.x * ROLL_TILE;
    const int64_t t1 = t0 + ROLL_TILE < a.n ? t0 + ROLL_TILE : a.n;
    const int64_t lo = t0 - (a.window - 1), span = t1 - lo;          // the tile reads x[lo .. t1 - 1]
    const double *x = a.x;
    auto load = [x, lo](int64_t i) { return x[lo + i]; };

    RollState st;
#pragma unroll
    for (int r = 0; r < ROLL_OPL; ++r) { st.s[r] = 0.0; st.q[r] = 0.0; st.cnt[r] = 0; }
    fmk_window_walk<ROLL_BLOCK, ROLL_OPL>(roll_lds, span, a.window, a.slab, true, load, [&](int r, double v) {
        if constexpr (MODE == ROLL_VAR) {
            const bool ok = v == v;                                  // NaN skipped by select
            const double s = st.s[r] + v, q = st.q[r] + v * v;
            st.s[r] = ok ? s : st.s[r];
            st.q[r] = ok ? q : st.q[r];
            st.cnt[r] += ok ? 1 : 0;
        } else {
            st.s[r] += v;
        }
    });
    if constexpr (MODE == ROLL_Z) {
#pragma unroll
        for (int r = 0; r < ROLL_OPL; ++r) { st.q[r] = st.s[r] / a.scale; st.s[r] = 0.0; }
        fmk_window_walk<ROLL_BLOCK, ROLL_OPL>(roll_lds, span, a.window, a.slab, span > (int64_t)a.slab, load, [&](int r, double v) {
            const double d = v - st.q[r];
            st.s[r] += d * d;
        });
    }
#pragma unroll
    for (int r = 0; r < ROLL_OPL; ++r) {
        const int64_t t = t0 + r * ROLL_BLOCK + threadIdx.x;
        if (t >= t1) continue;
        double o;
        if constexpr (MODE == ROLL_MEAN) {
            o = a.scale * st.s[r];
        } else if constexpr (MODE == ROLL_VAR) {
            o = NAN;
            const int64_t cnt = st.cnt[r];
            if (cnt >= a.min_periods && cnt > a.ddof) {
                const double m = st.s[r] / (double)cnt;
                double v = st.q[r] / (double)cnt - m * m;
                v = v * ((double)cnt / (double)(cnt - a.ddof));
                o = v > 0.0 ? v : 0.0;                               // max(0.0, v): a NaN v gives 0.0
            }
        } else {
            const double mean = st.q[r], sd = sqrt(st.s[r] / a.denom);
            o = sd == 0.0 ? NAN : (a.x[t] - mean) / sd;
        }
        a.out[t] = o;
    }
}

__global__ __launch_bounds__(256) void k_nan_fill(double *out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = NAN;
}

// r1[i]: the one-step return of p[i] over p[i-1], NaN at 0 and where the reference refuses the pair
template <bool LOG>
__global__ __launch_bounds__(256) void k_vr_r1(const double *__restrict__ p, int64_t n, double *__restrict__ r1)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double r = NAN;
        if (i > 0) {
            const double c = p[i], b = p[i - 1];
            if constexpr (LOG) {
                if (c == c && b == b && !(b <= 0.0) && !(c <= 0.0)) r = fmk_log_host(c / b);
            } else {
                if (c == c && b == b && !(b <= 0.0)) r = c / b - 1.0;
            }
        }
        r1[i] = r;
    }
}

// r4[i] = ((r1[i] + r1[i-1]) + r1[i-2]) + r1[i-3] for i >= 4, NaN when one of the four is
__global__ __launch_bounds__(256) void k_vr_r4(const double *__restrict__ r1, int64_t n, double *__restrict__ r4)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double r = NAN;
        if (i >= 4) {
            const double a0 = r1[i], a1 = r1[i - 1], a2 = r1[i - 2], a3 = r1[i - 3];
            if (a0 == a0 && a1 == a1 && a2 == a2 && a3 == a3) r = ((a0 + a1) + a2) + a3;
        }
        r4[i] = r;
    }
}

// v1 (in place) -> v1 / (v4 / 4) where both are numbers and v4 > 0, NaN elsewhere
__global__ __launch_bounds__(256) void k_vr_ratio(double *v1, const double *__restrict__ v4, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double a = v1[i], b = v4[i];
        v1[i] = (a == a && b > 0.0) ? a / (b / 4.0) : NAN;
    }
}

// the checks every entry makes before a device is needed
int roll_check(fmk_ctx *ctx, const char *what, int64_t n, int64_t window)
{
    FMK_TRY(fmk_rule_window(ctx, what, window));
    return fmk_series_check(ctx, what, n);
}

// one mode over d_x[0 .. n) on the context's stream: NaN below window - 1 (everywhere when window > n), then the tiles
template <int MODE>
int roll_launch(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t ddof, int64_t min_periods, double *d_out)
{
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    if (window > n) return FMK_OK;
    RollArgs a;
    a.x = d_x; a.out = d_out; a.n = n; a.window = window; a.ddof = ddof; a.min_periods = min_periods;
    a.scale = MODE == ROLL_MEAN ? 1.0 / (double)window : (double)window;
    a.denom = (double)(window - ddof);
    a.slab = fmk_slab(window, ROLL_TILE);
    const int64_t tiles = fmk_ceil_div(n - (window - 1), ROLL_TILE);
    k_roll<MODE><<<(unsigned)tiles, ROLL_BLOCK, (size_t)a.slab * sizeof(double), ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

}  // namespace

int fmk_nan_head(fmk_ctx *ctx, double *d_out, int64_t n, int64_t window)
{
    const int64_t n_nan = window - 1 < n ? window - 1 : n;
    if (n_nan > 0) {
        k_nan_fill<<<fmk_grid_blocks(ctx, n_nan), 256, 0, ctx->stream>>>(d_out, n_nan);
        FMK_LAUNCH_CHECK(ctx);
    }
    return FMK_OK;
}

extern "C" int fmk_sma_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out)
{
    FMK_TRY(roll_check(ctx, "sma", n, window));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    return roll_launch<ROLL_MEAN>(ctx, d_x, n, window, 0, 0, d_out);
}

extern "C" int fmk_zscore_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t ddof, double *d_out)
{
    FMK_TRY(roll_check(ctx, "comp_zscore", n, window));
    FMK_TRY(fmk_rule_zscore(ctx, window, ddof));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    return roll_launch<ROLL_Z>(ctx, d_x, n, window, ddof, 0, d_out);
}

extern "C" int fmk_rolling_variance_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t ddof, int64_t min_periods,
                                        double *d_out)
{
    FMK_TRY(roll_check(ctx, "rolling_variance_nb", n, window));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    return roll_launch<ROLL_VAR>(ctx, d_x, n, window, ddof, min_periods, d_out);
}

extern "C" int fmk_variance_ratio_1_4_dev(fmk_ctx *ctx, const double *d_price, int64_t n, int64_t window, int64_t ddof, int is_log,
                                          double *d_out)
{
    FMK_TRY(roll_check(ctx, "variance_ratio_1_4_core", n, window));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    if (n < window + 4) return fmk_nan_head(ctx, d_out, n, n + 1);   // NaN everywhere
    const unsigned blocks = fmk_grid_blocks(ctx, n);
    void *work;
    FMK_TRY(fmk_alloc(ctx, (size_t)(3 * n) * sizeof(double), &work));
    double *r1 = (double *)work, *r4 = r1 + n, *v4 = r4 + n;         // v1 goes to d_out, the quotient over it
    if (is_log) k_vr_r1<true><<<blocks, 256, 0, ctx->stream>>>(d_price, n, r1);
    else k_vr_r1<false><<<blocks, 256, 0, ctx->stream>>>(d_price, n, r1);
    k_vr_r4<<<blocks, 256, 0, ctx->stream>>>(r1, n, r4);
    hipError_t le = hipGetLastError();
    int rc = le != hipSuccess ? fmk_set_error(ctx, FMK_E_HIP, "variance_ratio_1_4_core: %s", hipGetErrorString(le)) : FMK_OK;
    if (rc == FMK_OK) rc = roll_launch<ROLL_VAR>(ctx, r1, n, window, ddof, 1, d_out);
    if (rc == FMK_OK) rc = roll_launch<ROLL_VAR>(ctx, r4, n, window, ddof, 1, v4);
    if (rc == FMK_OK) {
        k_vr_ratio<<<blocks, 256, 0, ctx->stream>>>(d_out, v4, n);
        le = hipGetLastError();
        if (le != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "variance_ratio_1_4_core: %s", hipGetErrorString(le));
    }
    const int frc = fmk_free(ctx, work);                             // stream-ordered: the next user comes after the kernels
    return rc != FMK_OK ? rc : frc;
}
