// fmk_break.hip -- the Chu-Stinchcombe-White CUSUM test on levels (finmlkit/feature/core/structural_break/cusum.py), rolling and
// developing: the one O(n x window) / O(n^2) function of the reference.  Compute bound: per (t, n) pair a subtraction, a product, a
// quotient and two comparisons in float64; nothing a roofline would count moves.  DESIGN.md section 7b.
//
// Per output t with window start base(t) = max(0, t - window) (developing: 0), T = t - base:
//   S      = d2[base] + ... + d2[t-1], added in that order (np.cumsum), d2[i] = (y[i+1] - y[i])^2, y = log(x) as the host rounds it;
//   sigma  = sqrt(S / (T - 1)); sigma <= 0 -> (-1e-6, -1e-6, 0, 0) (a NaN sigma walks on and never wins);
//   n_rel  = 1 .. T-2 in this order, k = T - n_rel: dyn = y[t] - y[base + n_rel], den = sigma * sqrt(k), skipped when den <= 1e-16,
//            s_up = max(dyn, 0) / den, s_down = max(-dyn, 0) / den; a side takes a strictly greater value only, and with it the
//            critical value sqrt(4.6 + log(k)).
// Schedule: a workgroup owns BRK_TILE consecutive t, a lane one t.  The wave walks k DOWNWARDS in lockstep (that is n_rel upwards, so
// the first n_rel that attains the maximum keeps it): element j = t - k, so the 64 lanes read 64 consecutive LDS words, and k,
// sqrt(k) are wave-uniform for every t (rolling and developing alike; lanes with a shorter window join late).  The span
// [base(t0), t1 - 1) of the tile is staged in LDS in slabs of at most BRK_SLAB_MAX elements -- d2 for the pass that sums S, then y
// for the pass over the pairs; a lane takes from each slab the part of its own range that lies in it, in ascending order.
// Not the walk of fmk_window.h, which the fixed-window features share: here k runs downwards over per-lane ranges of different
// length (developing windows), and the wave's bounds are max / min reductions over its lanes.
#include <limits.h>
#include <stdlib.h>

#include "fmk_common.h"
#include "fmk_log.h"

#define BRK_TILE 256                 // outputs per workgroup, one per lane
#define BRK_SLAB_MAX 4096            // LDS elements per staging (32 KiB): five workgroups per CU
#define BRK_SLAB_MIN 64

namespace {

// y = log(x) with the host's log; *nonpos is set when an element is <= 0 (NaN passes), as cusum_test_rolling checks
__global__ __launch_bounds__(256) void k_brk_log(const double *__restrict__ x, int64_t n, double *__restrict__ y, int *nonpos)
{
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = x[i];
        bad |= v <= 0.0;
        y[i] = fmk_log_host(v);
    }
    if (__ballot(bad) != 0 && fmk_lane() == 0) atomicOr(nonpos, 1);
}

// d2[i] = (y[i+1] - y[i])^2 (the difference rounded before the square), the tables sqrt(k) and sqrt(4.6 + log(k)) for k < nk,
// and NaN in the first n_nan elements of the four outputs
__global__ __launch_bounds__(256) void k_brk_prep(const double *__restrict__ y, int64_t n, double *__restrict__ d2,
                                                  double *__restrict__ sqk, double *__restrict__ crit, int64_t nk, double *o0,
                                                  double *o1, double *o2, double *o3, int64_t n_nan)
{
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = first; i < n - 1; i += stride) {
        const double d = y[i + 1] - y[i];
        d2[i] = d * d;
    }
    for (int64_t k = first; k < nk; k += stride) {
        sqk[k] = sqrt((double)k);
        crit[k] = sqrt(4.6 + fmk_log_host((double)k));
    }
    for (int64_t i = first; i < n_nan; i += stride) o0[i] = o1[i] = o2[i] = o3[i] = NAN;
}

__global__ __launch_bounds__(256) void k_brk_sqrt(const double *in, int64_t n, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sqrt(in[i]);
}

struct BrkArgs {
    const double *y, *d2, *sqk, *crit;
    int64_t n, window, first;        // outputs first .. n-1; window: INT64_MAX for developing
    int slab;                        // LDS elements per staging
    double *up, *down, *cup, *cdn;
    fmk_mail::Brk *mail;
};

struct BrkState {
    double S, sigma, yt, mu, md;
    int ku, kd;
    long long pairs, skipped;
};

// One pass over the tile's span [lo, hi) in slabs: PASS 0 adds d2[jlo .. jhi] to st.S, PASS 1 walks the pairs y[jlo .. jhi]
// against st.yt.  The lane's range is empty when jlo > jhi.  Every lane of the workgroup comes here (barriers).
template <int PASS>
__device__ __forceinline__ void brk_walk(const BrkArgs &a, double *lds, int64_t lo, int64_t hi, int64_t t, int64_t jlo, int64_t jhi,
                                         BrkState &st)
{
    const double *__restrict__ src = PASS == 0 ? a.d2 : a.y;
    for (int64_t s0 = lo; s0 < hi; s0 += a.slab) {
        const int len = (int)(hi - s0 < (int64_t)a.slab ? hi - s0 : (int64_t)a.slab);
        __syncthreads();                                             // the readers of the previous slab are done
        for (int i = threadIdx.x; i < len; i += BRK_TILE) lds[i] = src[s0 + i];
        __syncthreads();
        const int64_t ja = jlo > s0 ? jlo : s0, jb = jhi < s0 + len - 1 ? jhi : s0 + len - 1;
        const bool some = ja <= jb;
        const int khi = some ? (int)(t - ja) : 0, klo = some ? (int)(t - jb) : 1;       // k = t - j, descending
        const int kmax = fmk_uniform((int)fmk_wave_max((int64_t)khi));
        if (kmax == 0) continue;                                     // no lane of this wave has an element in the slab
        const int kmin = fmk_uniform((int)fmk_wave_min((int64_t)(some ? klo : INT_MAX)));
        const int off = (int)(t - s0);                               // LDS word of element j = t - k: off - k
        if constexpr (PASS == 0) {
            double S = st.S;
            for (int k = kmax; k >= kmin; --k)
                if (k <= khi && k >= klo) S += lds[off - k];
            st.S = S;
        } else {
            const double sigma = st.sigma, yt = st.yt;
            double mu = st.mu, md = st.md;
            int ku = st.ku, kd = st.kd, skipped = 0;
            for (int k = kmax; k >= kmin; --k) {
                const double sq = a.sqk[k];                          // wave-uniform: a scalar load
                if (k <= khi && k >= klo) {
                    const double dyn = yt - lds[off - k];
                    const double den = sigma * sq;
                    if (den <= 1e-16) {
                        ++skipped;
                    } else {
                        // one quotient serves both sides: the side dyn does not point to has 0.0 / den, which is 0.0, or NaN
                        // under a NaN den
                        const double mag = dyn > 0.0 ? dyn : (dyn < 0.0 ? -dyn : 0.0);
                        const double q = mag / den;
                        const double z = den != den ? den : 0.0;
                        const double su = dyn > 0.0 ? q : z, sd = dyn < 0.0 ? q : z;
                        if (su > mu) { mu = su; ku = k; }
                        if (sd > md) { md = sd; kd = k; }
                    }
                }
            }
            st.mu = mu; st.md = md; st.ku = ku; st.kd = kd;
            st.skipped += skipped;
            st.pairs += some ? khi - klo + 1 : 0;
        }
    }
}

__global__ __launch_bounds__(BRK_TILE) void k_brk_pairs(BrkArgs a)
{
    extern __shared__ double brk_lds[];
    const int64_t tile = (int64_t)gridDim.x - 1 - blockIdx.x;       // the longest windows first; tiles are cut by outputs, not by pairs
    const int64_t t0 = a.first + tile * BRK_TILE;
    const int64_t t1 = t0 + BRK_TILE < a.n ? t0 + BRK_TILE : a.n;
    const int64_t t = t0 + threadIdx.x;
    const bool live = t < t1;
    const int64_t base = t > a.window ? t - a.window : 0;
    const int64_t lo = t0 > a.window ? t0 - a.window : 0, hi = t1 - 1;   // the tile reads d2[lo .. hi-1], y[lo+1 .. hi-1] and y[t]
    const int64_t T = t - base;

    BrkState st;
    st.S = 0.0; st.sigma = 0.0; st.mu = st.md = -1e-6; st.ku = st.kd = 0; st.pairs = st.skipped = 0;
    st.yt = live ? a.y[t] : 0.0;
    brk_walk<0>(a, brk_lds, lo, hi, t, live ? base : 1, live ? t - 1 : 0, st);
    bool go = false;
    if (live) {
        st.sigma = sqrt(st.S / (double)(T - 1));
        go = !(st.sigma <= 0.0);
    }
    brk_walk<1>(a, brk_lds, lo, hi, t, go ? base + 1 : 1, go ? t - 2 : 0, st);
    if (live) {
        a.up[t] = st.mu;
        a.down[t] = st.md;
        a.cup[t] = st.ku ? a.crit[st.ku] : 0.0;
        a.cdn[t] = st.kd ? a.crit[st.kd] : 0.0;
    }
    const long long pairs = fmk_wave_sum(st.pairs), skipped = fmk_wave_sum(st.skipped);
    if (fmk_lane() == 0) {
        if (pairs) atomicAdd(&a.mail->pairs, (unsigned long long)pairs);
        if (skipped) atomicAdd(&a.mail->skipped, (unsigned long long)skipped);
    }
}

// rolling (window < INT64_MAX: the positivity check, window raised to warmup + 2, nothing computed when n < warmup + 2) and
// developing (window == INT64_MAX) through one path
int brk_run(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t warmup, bool rolling, double *d_up, double *d_down,
            double *d_cup, double *d_cdn)
{
    if (warmup < 2) return fmk_set_error(ctx, FMK_E_ARG, "warmup_period must be at least 2.");
    if (warmup > n) warmup = n > 2 ? n : 2;                          // nothing is computed either way; keeps warmup + 2 in range
    if (n < 0 || n >= ((int64_t)1 << 31)) return fmk_set_error(ctx, FMK_E_ARG, "cusum_test: the series must hold fewer than 2^31 elements.");
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    int64_t *last = ctx->h_mail->brk.last;
    last[0] = last[1] = last[2] = last[3] = 0;
    fmk_mail::Brk *mail = &ctx->d_mail->brk;
    FMK_HIP(ctx, hipMemsetAsync(mail, 0, sizeof *mail, ctx->stream));
    if (n == 0) return FMK_OK;
    if (rolling && window < warmup + 2) window = warmup + 2;
    const bool compute = rolling ? n >= warmup + 2 : n > warmup;
    const int64_t kmax = n - 1 < window ? n - 1 : window;            // the longest window
    const int64_t nk = compute ? kmax + 1 : 0;

    void *work;
    FMK_TRY(fmk_alloc(ctx, (size_t)(2 * n + 2 * nk) * sizeof(double), &work));
    double *y = (double *)work, *d2 = y + n, *sqk = d2 + n, *crit = sqk + nk;
    const unsigned blocks = fmk_grid_blocks(ctx, n);
    k_brk_log<<<blocks, 256, 0, ctx->stream>>>(d_x, n, y, &mail->nonpos);
    hipError_t le = hipGetLastError();
    int rc = le != hipSuccess ? fmk_set_error(ctx, FMK_E_HIP, "cusum_test: %s", hipGetErrorString(le)) : FMK_OK;
    if (rc == FMK_OK && rolling) {
        int nonpos = 0;
        rc = fmk_read_back(ctx, &nonpos, &mail->nonpos, sizeof nonpos);
        if (rc == FMK_OK && nonpos) rc = fmk_set_error(ctx, FMK_E_ARG, "All close prices must be positive.");
    }
    if (rc == FMK_OK) {
        k_brk_prep<<<blocks, 256, 0, ctx->stream>>>(y, n, d2, sqk, crit, nk, d_up, d_down, d_cup, d_cdn,
                                                            compute ? (warmup < n ? warmup : n) : n);
        le = hipGetLastError();
        if (le != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "cusum_test: %s", hipGetErrorString(le));
    }
    if (rc == FMK_OK && compute) {
        const int64_t span = kmax + BRK_TILE;                        // what a full tile reads
        int64_t slab = span < BRK_SLAB_MAX ? span : BRK_SLAB_MAX;
        if (const char *v = getenv("FMK_BREAK_SLAB")) {              // tests only: a smaller slab, so that small windows take several
            const int64_t f = atoll(v);
            if (f > 0 && f < slab) slab = f < BRK_SLAB_MIN ? BRK_SLAB_MIN : f;
        }
        BrkArgs a;
        a.y = y; a.d2 = d2; a.sqk = sqk; a.crit = crit; a.n = n; a.window = window; a.first = warmup; a.slab = (int)slab;
        a.up = d_up; a.down = d_down; a.cup = d_cup; a.cdn = d_cdn; a.mail = mail;
        const int64_t tiles = fmk_ceil_div(n - warmup, BRK_TILE);
        k_brk_pairs<<<(unsigned)tiles, BRK_TILE, (size_t)slab * sizeof(double), ctx->stream>>>(a);
        le = hipGetLastError();
        if (le != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "cusum_test: %s", hipGetErrorString(le));
        last[0] = n - warmup;
        last[1] = fmk_ceil_div(span < n - 1 ? span : n - 1, slab);
        last[2] = slab;
        last[3] = tiles;
    }
    const int frc = fmk_free(ctx, work);                             // stream-ordered: the next user comes after the kernels
    return rc != FMK_OK ? rc : frc;
}

}  // namespace

extern "C" int fmk_cusum_test_rolling_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window_size, int64_t warmup_period,
                                          double *d_up, double *d_down, double *d_crit_up, double *d_crit_down)
{
    if (window_size == INT64_MAX) --window_size;                     // INT64_MAX means "developing" inside
    return brk_run(ctx, d_x, n, window_size, warmup_period, true, d_up, d_down, d_crit_up, d_crit_down);
}

extern "C" int fmk_cusum_test_developing_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t warmup_period, double *d_up,
                                             double *d_down, double *d_crit_up, double *d_crit_down)
{
    return brk_run(ctx, d_x, n, INT64_MAX, warmup_period, false, d_up, d_down, d_crit_up, d_crit_down);
}

extern "C" int fmk_diag_cusum_test_last(fmk_ctx *ctx, int64_t *out6)
{
    fmk_mail::Brk m;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    FMK_TRY(fmk_read_back(ctx, &m, &ctx->d_mail->brk, sizeof m));
    const int64_t *last = ctx->h_mail->brk.last;
    out6[0] = last[0];
    out6[1] = (int64_t)m.pairs;
    out6[2] = last[1];
    out6[3] = (int64_t)(m.pairs - m.skipped);
    out6[4] = last[2];
    out6[5] = last[3];
    return FMK_OK;
}

extern "C" int fmk_diag_device_sqrt(fmk_ctx *ctx, const double *d_in, int64_t n, double *d_out)
{
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n <= 0) return FMK_OK;
    k_brk_sqrt<<<(unsigned)fmk_ceil_div(n, 256), 256, 0, ctx->stream>>>(d_in, n, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}
