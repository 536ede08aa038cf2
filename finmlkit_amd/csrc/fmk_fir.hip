// fmk_fir.hip -- a causal FIR filter on a resident float64 series, and with the weights of feature/core/fracdiff.py the fixed-width
// window fractional differentiation (Lopez de Prado, Advances in Financial Machine Learning, ch. 5: "FFD").  DESIGN.md section 7k.
//
// With W weights, w[k] multiplying x[t-k], and x~ = x where x is finite, NaN elsewhere:
//   y[t] = NaN                                                                    for t < W - 1
//   y[t] = acc after  acc = +0.0;  for k = W-1, W-2, .. 0: acc = fma(w[k], x~[t-k], acc)
// one correctly rounded fused multiply-add per tap, oldest tap first, one chain per output: the bits do not depend on the schedule.
//
// Schedule: a workgroup is ONE wave and owns FMK_FIR_TILE = 64 * FIR_OPL consecutive outputs from t = W - 1 on (the head is
// fmk_nan_head's); a lane owns FIR_OPL CONSECUTIVE outputs and keeps their accumulators in registers.  The taps are walked in passes
// of at most FMK_FIR_TAPS, oldest first; per pass the span of x~ that the tile's outputs meet in those taps (tile + taps - 1
// elements) is staged in LDS, non-finite -> NaN while staging.  Inside a pass a lane steps through its FIR_OPL + taps - 1 elements
// in ascending order: at step s it reads ONE element and output r of the lane takes it with tap kb - s + r (kb: the pass's oldest
// tap), so a step is one LDS read and FIR_OPL fused multiply-adds on FIR_OPL independent chains, and every chain meets its taps in
// descending order.  The tap of a step is the same in every lane: the weights are wave-uniform reads of global memory (scalar loads,
// a weight is a scalar operand of the multiply-add).  The first and last FIR_OPL - 1 steps of a pass serve only some of the lane's
// outputs -- a fixed triangle each, unrolled; a pass of fewer than FIR_OPL taps asks at every step -- the steps between serve all.
// LDS: a lane reads elements FIR_OPL apart, so element i sits at word i + i / FIR_OPL: lanes are 9 words apart and a 32-lane group
// of an 8-byte read meets 32 different bank pairs.  The outputs leave through LDS too, so that a wave stores 64 consecutive words.
// No atomics, no cross-lane exchange, no second kernel.  8-byte loads and stores only: the pointers need no more alignment.
#include <math.h>

#include "fmk_common.h"

#define FIR_LANES 64
#define FIR_OPL 8                                                    // consecutive outputs per lane
#define FIR_BATCH 8                                                  // global loads a lane has in flight while staging
static_assert(FMK_FIR_TILE == FIR_LANES * FIR_OPL, "a lane owns FIR_OPL consecutive outputs of the tile");
static_assert(FIR_OPL == 8, "fir_word pads one word per 8 elements");
static_assert(FMK_FIR_TAPS >= FIR_OPL, "a pass has steps that serve every output of the lane");

namespace {

__host__ __device__ __forceinline__ int fir_word(int i) { return i + (i >> 3); }

// LDS words of a launch: the widest pass's span, and the tile itself on the way out
size_t fir_lds_words(int64_t width)
{
    const int taps = (int)(width < FMK_FIR_TAPS ? width : FMK_FIR_TAPS);
    return (size_t)fir_word(FMK_FIR_TILE + taps - 2) + 1;
}

// one step of a pass: the lane's element s, taken by output r with tap kb - s + r; CHECKED: only taps ka .. kb exist in this pass
template <bool CHECKED>
__device__ __forceinline__ void fir_step(const double *row, const double *__restrict__ w, int s, int ka, int kb, double (&acc)[FIR_OPL])
{
    const double v = row[fir_word(s)];
#pragma unroll
    for (int r = 0; r < FIR_OPL; ++r) {
        const int k = kb - s + r;
        if (!CHECKED || (k >= ka && k <= kb)) acc[r] = fma(w[k], v, acc[r]);
    }
}

__global__ __launch_bounds__(FIR_LANES) void k_fir(const double *__restrict__ x, const double *__restrict__ w, double *__restrict__ out,
                                                   int64_t n, int width)
{
    extern __shared__ double lds[];                                  // fir_lds_words(width) words
    const int lane = threadIdx.x;
    const int64_t t0 = (int64_t)(width - 1) + (int64_t)blockIdx.x * FMK_FIR_TILE;     // the tile's first output
    const double *row = lds + lane * (FIR_OPL + 1);                  // fir_word(lane * FIR_OPL + s) = lane * 9 + fir_word(s)

    double acc[FIR_OPL];
#pragma unroll
    for (int r = 0; r < FIR_OPL; ++r) acc[r] = 0.0;

    for (int kb = width - 1; kb >= 0; kb -= FMK_FIR_TAPS) {          // taps ka .. kb, oldest first
        const int ka = kb - FMK_FIR_TAPS + 1 > 0 ? kb - FMK_FIR_TAPS + 1 : 0;
        const int taps = kb - ka + 1;
        const int64_t lo = t0 - kb;                                  // the first element staged: >= 0
        const int span = FMK_FIR_TILE + taps - 1;
        __syncthreads();                                             // the readers of the previous pass are done
        for (int i0 = lane; i0 < span; i0 += FIR_LANES * FIR_BATCH) {   // FIR_BATCH loads in flight per lane
            double v[FIR_BATCH];
#pragma unroll
            for (int u = 0; u < FIR_BATCH; ++u) {
                const int i = i0 + u * FIR_LANES;
                const int64_t g = lo + i;
                v[u] = i < span && g < n ? x[g] : NAN;               // beyond the series: met only by outputs that are not stored
            }
#pragma unroll
            for (int u = 0; u < FIR_BATCH; ++u) {
                const int i = i0 + u * FIR_LANES;
                if (i < span) lds[fir_word(i)] = __builtin_isfinite(v[u]) ? v[u] : NAN;
            }
        }
        __syncthreads();
        // steps 0 .. taps + FIR_OPL - 2; every output of the lane is served at FIR_OPL - 1 <= s <= taps - 1.  Before that output r
        // is served from step r on (its oldest tap of the pass is kb), after that up to step taps - 1 + r (its newest is ka)
        if (taps >= FIR_OPL) {
#pragma unroll
            for (int s = 0; s < FIR_OPL - 1; ++s) {
                const double v = row[s];                             // fir_word(s) = s below FIR_OPL
#pragma unroll
                for (int r = 0; r <= s; ++r) acc[r] = fma(w[kb - s + r], v, acc[r]);
            }
            int s = FIR_OPL - 1;
            for (; s + FIR_OPL <= taps; s += FIR_OPL) {
#pragma unroll
                for (int u = 0; u < FIR_OPL; ++u) fir_step<false>(row, w, s + u, ka, kb, acc);
            }
            for (; s < taps; ++s) fir_step<false>(row, w, s, ka, kb, acc);
#pragma unroll
            for (int j = 1; j < FIR_OPL; ++j) {
                const double v = row[fir_word(taps - 1 + j)];
#pragma unroll
                for (int r = j; r < FIR_OPL; ++r) acc[r] = fma(w[ka - j + r], v, acc[r]);
            }
        } else {                                                     // fewer taps than outputs per lane: every step asks
            for (int s = 0; s < taps + FIR_OPL - 1; ++s) fir_step<true>(row, w, s, ka, kb, acc);
        }
    }

    __syncthreads();
    double *mine = lds + lane * (FIR_OPL + 1);
#pragma unroll
    for (int r = 0; r < FIR_OPL; ++r) mine[r] = acc[r];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FIR_OPL; ++j) {
        const int i = j * FIR_LANES + lane;
        if (t0 + i < n) out[t0 + i] = lds[fir_word(i)];
    }
}

}  // namespace

extern "C" int fmk_fir_geometry(int64_t *out2)
{
    out2[0] = FMK_FIR_TILE;
    out2[1] = FMK_FIR_TAPS;
    return FMK_OK;
}

extern "C" int fmk_fir_dev(fmk_ctx *ctx, const double *d_x, int64_t n, const double *w, int64_t width, double *d_out)
{
    FMK_TRY(fmk_rule_fir(ctx, w, width, d_x, d_out));
    FMK_TRY(fmk_series_check(ctx, "fir", n));
    if (n == 0) return FMK_OK;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    FMK_TRY(fmk_nan_head(ctx, d_out, n, width));
    if (width > n) return FMK_OK;
    void *d_w;
    FMK_TRY(fmk_alloc(ctx, sizeof(double) * (size_t)width, &d_w));
    int rc = fmk_h2d(ctx, d_w, w, sizeof(double) * (size_t)width);   // in the stream's order; w is the caller's again on return
    if (rc == FMK_OK) {
        const int64_t tiles = fmk_ceil_div(n - (width - 1), FMK_FIR_TILE);
        k_fir<<<(unsigned)tiles, FIR_LANES, fir_lds_words(width) * sizeof(double), ctx->stream>>>(d_x, (const double *)d_w, d_out, n, (int)width);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "k_fir launch failed: %s", hipGetErrorString(e));
    }
    const int rf = fmk_free(ctx, d_w);                               // the allocator follows the stream: the kernel is ahead
    return rc != FMK_OK ? rc : rf;
}
