// fmk_entropy.hip -- rolling approximate entropy on a resident float64 series: the reference's ApproximateEntropy transform
// (transforms.py:1400-1457), which runs antropy.app_entropy(x, order=m, metric="chebyshev", tolerance=tol * std(x)) under pandas'
// rolling.apply.  O(n x window^2): the tolerance is each window's own, so every window is a fresh all-pairs problem.  The contract
// is the published algorithm within the measured tolerance of tests/golden/entropy.json, NaN positions exactly.  DESIGN.md
// section 7c4.
//
// For the window x[t-w+1 .. t], t >= w - 1, written x_0 .. x_{w-1}:
//   r      = tol * sqrt(sum((x_p - mean)^2) / w), mean = sum(x_p) / w, both sums oldest first
//   k in (m, m + 1): N_k = w - k + 1 vectors v_i = (x_i .. x_{i+k-1}); C_k[i] = #{j : max_q |x_{i+q} - x_{j+q}| <= r}, j = i included
//   phi_k  = sum_i (ln C_k[i] - ln N_k) / N_k, i ascending
//   out[t] = phi_m - phi_{m+1}
// A window that reads a NaN or an infinity gives NaN (pandas' rolling turns +-inf into NaN and wants a full window): the loader
// makes every non-finite element NaN, r is then NaN, no comparison holds, every count is 0 and ln 0 is tabulated as NaN.  A window
// in which every pair matches (a constant one, a huge tolerance) gives exactly 0.0: every term ln C - ln N is 0.0.
//
// Schedule: one lane per output, 256 outputs per workgroup.  The workgroup stages its span (window + 256 + 1 words: a full tile's
// span, and two words more that are read and masked away) and the table ln 0 .. ln window (ln as the host computes it, fmk_log.h)
// into LDS once, behind one barrier; lanes past n are fed NaN and only their store is dropped.  Element p of lane l's window is
// word l + p, so a wave reads 64 consecutive 8-byte words per step and every loop bound is uniform over the wave.
//   window <= 64  row masks: D_i has bit j set where |x_i - x_j| <= r.  With the last m + 1 rows in registers,
//                 C_m[i] = popcount(D_i & D_{i+1} >> 1 & .. & D_{i+m-1} >> (m-1)) over the low N_m bits and one more AND gives
//                 C_{m+1}[i]: one comparison per pair.  Two rows are built per pass over the window, so a staged word is read
//                 once for two rows.
//   window > 64   the plain path: per pair of vectors m + 1 comparisons with a running AND, the window sliding through registers.
#include <limits.h>

#include "fmk_common.h"
#include "fmk_log.h"

#define APEN_BLOCK 256               // lanes, and outputs, per workgroup
#define APEN_MASK_WINDOW 64          // the longest window whose row mask is one 64-bit word

namespace {

struct ApenArgs {
    const double *x;
    double *out;
    int64_t n;
    int window;
    double tolerance;
};

__device__ __forceinline__ double apen_finite(double v) { return __builtin_isfinite(v) ? v : NAN; }

// words of the staged span, and of the table behind it
__host__ __device__ __forceinline__ int apen_span_words(int window) { return window + APEN_BLOCK + 1; }
__host__ __device__ __forceinline__ int apen_lds_words(int window) { return apen_span_words(window) + window + 1; }

template <int M, bool MASK>
__global__ __launch_bounds__(APEN_BLOCK) void k_apen(ApenArgs a)
{
    extern __shared__ double apen_lds[];
    const int w = a.window;
    const int64_t lo = (int64_t)blockIdx.x * APEN_BLOCK;             // the tile's first output is lo + w - 1, its first element lo
    const int words = apen_span_words(w);
    double *tab = apen_lds + words;
    for (int i = threadIdx.x; i < words; i += APEN_BLOCK) apen_lds[i] = lo + i < a.n ? apen_finite(a.x[lo + i]) : NAN;
    for (int k = threadIdx.x; k <= w; k += APEN_BLOCK) tab[k] = k ? fmk_log_host((double)k) : NAN;
    __syncthreads();
    const double *row = apen_lds + threadIdx.x;                      // element p of this lane's window

    double s = 0.0;
    for (int p = 0; p < w; ++p) s += row[p];
    const double mean = s / (double)w;
    s = 0.0;
    for (int p = 0; p < w; ++p) {
        const double d = row[p] - mean;
        s += d * d;
    }
    const double r = a.tolerance * sqrt(s / (double)w);

    const int nm = w - M + 1, nm1 = w - M;                           // vectors of order m and of order m + 1
    const double lm = tab[nm], lm1 = tab[nm1];
    double sm = 0.0, sm1 = 0.0;                                      // the sums of ln C - ln N
    if (MASK) {
        const uint64_t keep_m = nm >= 64 ? ~0ull : (1ull << nm) - 1ull, keep_m1 = (1ull << nm1) - 1ull;
        uint64_t rows[M + 1];                                        // after row p went in: D_{p-M} .. D_p
#pragma unroll
        for (int q = 0; q <= M; ++q) rows[q] = 0;
        auto push = [&](uint64_t d, int p) {
#pragma unroll
            for (int q = 0; q < M; ++q) rows[q] = rows[q + 1];
            rows[M] = d;
            const int v = p - M;                                     // the vector whose rows these are; v <= nm - 1
            if (v < 0) return;
            uint64_t c = rows[0];
#pragma unroll
            for (int q = 1; q < M; ++q) c &= rows[q] >> q;
            sm += tab[__popcll(c & keep_m)] - lm;
            if (v < nm1) sm1 += tab[__popcll(c & (rows[M] >> M) & keep_m1)] - lm1;
        };
        const int jl = w < 32 ? w : 32;
        for (int p = 0; p <= w; p += 2) {                            // rows p and p + 1; row w is empty and closes C_m[nm - 1]
            const double xa = p < w ? row[p] : NAN, xb = p + 1 < w ? row[p + 1] : NAN;
            uint32_t alo = 0, ahi = 0, blo = 0, bhi = 0;
            for (int j = 0; j < jl; ++j) {
                const double xj = row[j];
                const uint32_t bit = 1u << j;
                alo |= fabs(xa - xj) <= r ? bit : 0u;
                blo |= fabs(xb - xj) <= r ? bit : 0u;
            }
            for (int j = 32; j < w; ++j) {
                const double xj = row[j];
                const uint32_t bit = 1u << (j - 32);
                ahi |= fabs(xa - xj) <= r ? bit : 0u;
                bhi |= fabs(xb - xj) <= r ? bit : 0u;
            }
            push((uint64_t)ahi << 32 | alo, p);
            if (p + 1 <= w) push((uint64_t)bhi << 32 | blo, p + 1);
        }
    } else {
        for (int i = 0; i < nm; ++i) {
            double xi[M + 1], xj[M + 1];
#pragma unroll
            for (int q = 0; q <= M; ++q) xi[q] = row[i + q];         // row[w] at i = nm - 1: read, and masked by i < nm1
#pragma unroll
            for (int q = 0; q < M; ++q) xj[q] = row[q];
            int cm = 0, cm1 = 0;
            for (int j = 0; j < nm; ++j) {
                xj[M] = row[j + M];
                bool ok = true;
#pragma unroll
                for (int q = 0; q < M; ++q) ok &= fabs(xi[q] - xj[q]) <= r;
                cm += ok;
                cm1 += ok & (fabs(xi[M] - xj[M]) <= r) & (j < nm1);
#pragma unroll
                for (int q = 0; q < M; ++q) xj[q] = xj[q + 1];
            }
            sm += tab[cm] - lm;
            if (i < nm1) sm1 += tab[cm1] - lm1;
        }
    }
    const int64_t t = lo + (w - 1) + threadIdx.x;
    if (t < a.n) a.out[t] = sm / (double)nm - sm1 / (double)nm1;
}

template <int M>
void apen_launch(fmk_ctx *ctx, const ApenArgs &a, unsigned tiles, size_t lds)
{
    if (a.window <= APEN_MASK_WINDOW) k_apen<M, true><<<tiles, APEN_BLOCK, lds, ctx->stream>>>(a);
    else k_apen<M, false><<<tiles, APEN_BLOCK, lds, ctx->stream>>>(a);
}

}  // namespace

static_assert(FMK_APEN_MAX_M == 4, "apen_launch is instantiated for m = 1 .. 4");

extern "C" int fmk_approximate_entropy_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t m, double tolerance,
                                           double *d_out)
{
    FMK_TRY(fmk_rule_apen(ctx, window, m, tolerance));
    FMK_TRY(fmk_series_check(ctx, "approximate_entropy", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    if (window > n) return FMK_OK;
    ApenArgs a;
    a.x = d_x; a.out = d_out; a.n = n; a.window = (int)window; a.tolerance = tolerance;
    const unsigned tiles = (unsigned)fmk_ceil_div(n - (window - 1), APEN_BLOCK);
    const size_t lds = (size_t)apen_lds_words(a.window) * sizeof(double);
    switch (m) {
    case 1: apen_launch<1>(ctx, a, tiles, lds); break;
    case 2: apen_launch<2>(ctx, a, tiles, lds); break;
    case 3: apen_launch<3>(ctx, a, tiles, lds); break;
    default: apen_launch<4>(ctx, a, tiles, lds); break;
    }
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}
