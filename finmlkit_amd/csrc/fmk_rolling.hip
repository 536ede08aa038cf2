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
// Schedule (that of fmk_break.hip): a workgroup owns ROLL_TILE consecutive outputs, a lane ROLL_OPL of them, ROLL_BLOCK apart: that
// many independent add chains per lane.  All lanes walk the position p inside their windows upwards in lockstep, so a wave reads 64
// consecutive LDS words per step and output.  The span [t0 - window + 1, t1) of the tile is staged in LDS in slabs of at most
// ROLL_SLAB_MAX elements; from each slab an output takes the part of its window that lies in it, slabs and positions ascending.  The
// z-score walks twice (the sum, then the squared deviations from the lane's own mean) and stages twice only when the span takes
// more than one slab.  No atomics, no cross-lane exchange.
// The variance ratio is r1 (one-step log or simple returns, the host's log: fmk_log.h) and r4 (four of them added, newest first) by
// two elementwise kernels, the variance mode on both, and a kernel for the quotient.
#include <limits.h>

#include "fmk_common.h"
#include "fmk_log.h"

#define ROLL_BLOCK 256               // lanes per workgroup
#ifndef ROLL_OPL
#define ROLL_OPL 4                   // outputs per lane: the tuning knob (independent float64 add chains)
#endif
#define ROLL_TILE (ROLL_BLOCK * ROLL_OPL)
#define ROLL_SLAB_MAX 4096           // LDS elements per staging (32 KiB): five workgroups per CU

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

// one element of output r; PASS 1 is the second walk of the z-score
template <int MODE, int PASS>
__device__ __forceinline__ void roll_take(RollState &st, int r, double v)
{
    if constexpr (MODE == ROLL_VAR) {
        const bool ok = v == v;                                      // NaN skipped by select
        const double s = st.s[r] + v, q = st.q[r] + v * v;
        st.s[r] = ok ? s : st.s[r];
        st.q[r] = ok ? q : st.q[r];
        st.cnt[r] += ok ? 1 : 0;
    } else if constexpr (PASS == 0) {
        st.s[r] += v;
    } else {
        const double d = v - st.q[r];
        st.s[r] += d * d;
    }
}

// One walk over the tile's span [lo, hi) in slabs.  woff0 = (first output of this wave's lane 0) - (window - 1): the element
// its window starts with; output r of lane l starts r * ROLL_BLOCK + l elements later.  With q = woff0 - s0 + p wave-uniform, position
// p of every window of the wave is LDS word q + r * ROLL_BLOCK + l of the slab that starts at s0.  Every lane of the workgroup comes
// here (barriers); lanes without an output read staged words and drop what they add.
template <int MODE, int PASS>
__device__ __forceinline__ void roll_walk(const RollArgs &a, double *lds, int64_t lo, int64_t hi, int64_t woff0, bool stage,
                                          RollState &st)
{
    const int lane = fmk_lane();
    constexpr int REACH = (ROLL_OPL - 1) * ROLL_BLOCK + 63;          // the last word a wave reads at q: q + REACH
    for (int64_t s0 = lo; s0 < hi; s0 += a.slab) {
        const int len = (int)(hi - s0 < (int64_t)a.slab ? hi - s0 : (int64_t)a.slab);
        if (stage) {
            __syncthreads();                                         // the readers of the previous slab are done
            for (int i = threadIdx.x; i < len; i += ROLL_BLOCK) lds[i] = a.x[s0 + i];
            __syncthreads();
        }
        // q over the positions 0 .. window - 1 that reach into the slab for some lane and output of the wave
        const int64_t w0 = woff0 - s0;
        int64_t qa = w0 > -(int64_t)REACH ? w0 : -(int64_t)REACH;
        int64_t qb = w0 + a.window - 1 < (int64_t)len - 1 ? w0 + a.window - 1 : (int64_t)len - 1;
        if (qa > qb) continue;
        const int qlo = fmk_uniform((int)qa), qhi = fmk_uniform((int)qb);
        // [fa, fb]: every word q .. q + REACH lies in the slab, no lane needs a check
        const int fa = qlo > 0 ? qlo : 0;
        int fb = qhi < len - 1 - REACH ? qhi : len - 1 - REACH;
        if (fb < fa) fb = fa - 1;
        const int hb = fa - 1 < qhi ? fa - 1 : qhi;                  // the steps before word 0: some lanes are not in the slab yet
        for (int q = qlo; q <= hb; ++q) {
#pragma unroll
            for (int r = 0; r < ROLL_OPL; ++r) {
                const int i = q + r * ROLL_BLOCK + lane;
                if ((unsigned)i < (unsigned)len) roll_take<MODE, PASS>(st, r, lds[i]);
            }
        }
        const double *row = lds + lane;
#pragma unroll 4
        for (int q = fa; q <= fb; ++q) {
#pragma unroll
            for (int r = 0; r < ROLL_OPL; ++r) roll_take<MODE, PASS>(st, r, row[q + r * ROLL_BLOCK]);
        }
        for (int q = fb + 1; q <= qhi; ++q) {
#pragma unroll
            for (int r = 0; r < ROLL_OPL; ++r) {
                const int i = q + r * ROLL_BLOCK + lane;
                if ((unsigned)i < (unsigned)len) roll_take<MODE, PASS>(st, r, lds[i]);
            }
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(ROLL_BLOCK) void k_roll(RollArgs a)
{
    extern __shared__ double roll_lds[];
    const int64_t t0 = a.window - 1 + (int64_t)blockIdx.x * ROLL_TILE;
    const int64_t t1 = t0 + ROLL_TILE < a.n ? t0 + ROLL_TILE : a.n;
    const int64_t lo = t0 - (a.window - 1), hi = t1;                 // the tile reads x[lo .. hi - 1]
    const int64_t woff0 = lo + (threadIdx.x & ~63);
    const bool one_slab = hi - lo <= (int64_t)a.slab;

    RollState st;
#pragma unroll
    for (int r = 0; r < ROLL_OPL; ++r) { st.s[r] = 0.0; st.q[r] = 0.0; st.cnt[r] = 0; }
    roll_walk<MODE, 0>(a, roll_lds, lo, hi, woff0, true, st);
    if constexpr (MODE == ROLL_Z) {
#pragma unroll
        for (int r = 0; r < ROLL_OPL; ++r) { st.q[r] = st.s[r] / a.scale; st.s[r] = 0.0; }
        roll_walk<MODE, 1>(a, roll_lds, lo, hi, woff0, !one_slab, st);
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

__global__ __launch_bounds__(256) void k_roll_nan(double *out, int64_t n)
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

unsigned roll_blocks(fmk_ctx *ctx, int64_t n)
{
    int64_t blocks = fmk_ceil_div(n, 256);
    if (blocks > (int64_t)ctx->n_cu * 16) blocks = (int64_t)ctx->n_cu * 16;
    return (unsigned)(blocks > 0 ? blocks : 1);
}

// the checks every entry makes before a device is needed
int roll_check(fmk_ctx *ctx, const char *what, int64_t n, int64_t window)
{
    if (window < 1) return fmk_set_error(ctx, FMK_E_ARG, "%s: window must be at least 1.", what);
    if (n < 0 || n >= ((int64_t)1 << 31)) return fmk_set_error(ctx, FMK_E_ARG, "%s: the series must hold fewer than 2^31 elements.", what);
    return FMK_OK;
}

// one mode over d_x[0 .. n) on the context's stream: NaN below window - 1 (everywhere when window > n), then the tiles
template <int MODE>
int roll_launch(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t ddof, int64_t min_periods, double *d_out)
{
    const int64_t n_nan = window - 1 < n ? window - 1 : n;
    if (n_nan > 0) {
        k_roll_nan<<<roll_blocks(ctx, n_nan), 256, 0, ctx->stream>>>(d_out, n_nan);
        FMK_LAUNCH_CHECK(ctx);
    }
    if (window > n) return FMK_OK;
    const int64_t span = window - 1 + ROLL_TILE;                     // what a full tile reads
    RollArgs a;
    a.x = d_x; a.out = d_out; a.n = n; a.window = window; a.ddof = ddof; a.min_periods = min_periods;
    a.scale = MODE == ROLL_MEAN ? 1.0 / (double)window : (double)window;
    a.denom = (double)(window - ddof);
    a.slab = (int)(span < ROLL_SLAB_MAX ? span : ROLL_SLAB_MAX);
    const int64_t tiles = fmk_ceil_div(n - (window - 1), ROLL_TILE);
    k_roll<MODE><<<(unsigned)tiles, ROLL_BLOCK, (size_t)a.slab * sizeof(double), ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

}  // namespace

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
    if (ddof >= window) return fmk_set_error(ctx, FMK_E_ARG, "comp_zscore: window - ddof must be positive.");
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
    const unsigned blocks = roll_blocks(ctx, n);
    if (n < window + 4) {
        k_roll_nan<<<blocks, 256, 0, ctx->stream>>>(d_out, n);
        FMK_LAUNCH_CHECK(ctx);
        return FMK_OK;
    }
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
