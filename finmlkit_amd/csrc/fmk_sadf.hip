// fmk_sadf.hip -- the augmented Dickey-Fuller statistic of every backward window of an end point and its supremum (SADF: Lopez de
// Prado, Advances in Financial Machine Learning, ch. 17; Phillips, Wu and Yu).  The reference has no such function, so DESIGN.md
// section 7l IS the definition; include/fmk.h restates it.
//
// With dy_i = y_i - y_{i-1}, row i (i >= L + 1) of end point t has the target dy_i and the k = L + 2 (+ 1 for "ct") regressors
//   1, (i - t if "ct"), dy_{i-1}, .., dy_{i-L}, y_{i-1} - y_t                       (the columns in the order of the factor)
// and the window of m rows is i in [s, t], s = t - m + 1.  A is the (k+1) x (k+1) moment matrix of the window with the target as its
// last row and column; k steps of the LDL^T elimination (one reciprocal per pivot) leave SSR in A[k][k], and with z = A[k][k-1] and
// d = A[k-1][k-1] as the last pivot meets them
//   ADF(s, t) = z / sqrt(d * SSR / (m - k)).
// A pivot that is not above 2^-26 of its own diagonal moment makes the window degenerate (never chosen); SSR / sum dy^2 <= 2^-26 is
// an exact fit, copysign(inf, z).  An element that is not finite counts as NaN, a NaN sum fails the pivot test: such a window is
// never chosen.  SADF_t is the largest ADF(s, t) over m = min_len, min_len + step, .. <= max_len with s >= L + 1, the shortest
// window among equals.
//
// Schedule (fmk_trend.hip's, mirrored): one wave per end point over a persistent grid with a work counter, SADF_BATCH end points per
// visit to the counter.  The wave walks the window BACKWARDS from t, 64 rows per step, the next step's loads in flight; the lane of
// row i = t - j forms the row's products, every running moment is a wave-inclusive scan (fmk_dpp_iscan) plus a carried total, and
// the moments of 1 and i - t are closed forms of m.  The lane that holds row s owns window [s, t]: it solves its system in registers
// and keeps its own best with a strict >, so the shortest window wins inside a lane; one cross-lane arg-max after the walk takes the
// shortest among equals.  The kernel is instantiated per (L, trend): k alone does not say which columns there are.  By construction
// an end point reads 8 B x (L + 2) x rows walked, the repeats out of L1 / L2.
#include <math.h>

#include "fmk_common.h"
#include "fmk_dpp.h"

#define SADF_DEGENERATE 0x1p-26  // a pivot at or below this share of its diagonal moment: the window is degenerate (TR_EXACT_U's value)
#define SADF_EXACT 0x1p-26       // SSR / sum dy^2 at or below this: the fit counts as exact
#define SADF_BATCH 8             // end points a wave takes from the work counter at a time (fmk_trend.hip: TR_BATCH)
#define SADF_CLAIMS 4            // batches per wave the grid is sized for, below the persistent size

struct SadfArgs {
    const double *y;
    int64_t n;
    const int64_t *ev;           // NULL: end point e is element e
    int64_t n_end, min_len, max_len, step;
    double *stat;
    int64_t *start;
    int64_t *n_skipped;          // may be NULL
    fmk_mail::Sadf *mail;
};

__device__ __forceinline__ double sadf_finite(double v) { return v - v == 0.0 ? v : NAN; }

// The statistic of one window of m rows from its moment matrix (the lower triangle is read, and destroyed).  A NaN moment fails a
// pivot test, so a window that holds a NaN comes out NaN, as a degenerate one does.
template <int K>
__device__ __forceinline__ double sadf_solve(double (&A)[K + 1][K + 1], double m)
{
    const double yy = A[K][K];
    double g[K];
#pragma unroll
    for (int j = 0; j < K; ++j) g[j] = A[j][j];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double d = A[j][j];
        ok = ok && d > SADF_DEGENERATE * g[j];
        const double inv = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i <= K; ++i) {
            const double l = A[i][j] * inv;
#pragma unroll
            for (int r = j + 1; r <= i; ++r) A[i][r] -= l * A[r][j];
        }
    }
    if (!ok) return NAN;
    const double zl = A[K][K - 1], dl = A[K - 1][K - 1], ssr = A[K][K];      // the last pivot leaves its own column as it met it
    if (ssr / yy <= SADF_EXACT) return copysign(INFINITY, zl);
    return zl / sqrt(dl * ssr / (m - (double)K));
}

template <int L, bool CT>
__global__ __launch_bounds__(256) void k_sadf(const SadfArgs a)
{
    constexpr int K = L + 2 + (CT ? 1 : 0);           // regressors
    constexpr int P = L + 2;                          // a row's own numbers: the target, L lagged differences, the level
    constexpr int D0 = CT ? 2 : 1;                    // the first lagged difference's column
    const int lane = fmk_lane();
    long long skipped = 0, bad = 0;
    for (;;) {
        unsigned long long ew = 0;
        if (lane == 0) ew = atomicAdd(&a.mail->work, (unsigned long long)SADF_BATCH);
        const int64_t e0 = fmk_uniform((int64_t)ew);
        if (e0 >= a.n_end) break;
        const int cnt = a.n_end - e0 < SADF_BATCH ? (int)(a.n_end - e0) : SADF_BATCH;
        const int64_t my_t = lane < cnt ? (a.ev ? a.ev[e0 + lane] : e0 + lane) : 0;   // lane b keeps end point e0 + b and its outputs
        double o_stat = NAN;
        int64_t o_start = -1;                         // an end point without a usable window
        for (int b = 0; b < cnt; ++b) {
            const int64_t t = fmk_readlane(my_t, b);
            if (t < 0 || t >= a.n) { ++bad; continue; }                  // an index outside the series is counted: the call fails
            const int64_t rows = t - L < a.max_len ? t - L : a.max_len;  // rows L + 1 .. t exist: every load below stays in [0, t]
            double best = -INFINITY;
            int64_t best_m = 0;                       // 0: this lane has no window yet
            if (rows >= a.min_len) {
                const double *__restrict__ w = a.y + t;
                const double yt = sadf_finite(w[0]);
                double C[K + 1][K + 1];               // the carried totals (wave-uniform); only what the scans below name is used
#pragma unroll
                for (int r = 0; r <= K; ++r)
#pragma unroll
                    for (int c = 0; c <= K; ++c) C[r][c] = 0.0;
                double nx[P];
#pragma unroll
                for (int q = 0; q < P; ++q) nx[q] = lane < rows ? w[-(int64_t)lane - q] : 0.0;
                for (int64_t base = 0; base < rows; base += 64) {
                    const int64_t j = base + lane;    // row i = t - j; the window that starts there has j + 1 rows
                    const bool valid = j < rows;      // rows past the last: every product 0, and no window starts there
                    double u[P];
                    u[0] = sadf_finite(nx[0]) - sadf_finite(nx[1]);
#pragma unroll
                    for (int q = 1; q <= L; ++q) u[q] = sadf_finite(nx[q]) - sadf_finite(nx[q + 1]);
                    u[L + 1] = sadf_finite(nx[1]) - yt;
#pragma unroll
                    for (int q = 0; q < P; ++q) {
                        if (!valid) u[q] = 0.0;
                        nx[q] = j + 64 < rows ? w[-(j + 64) - q] : 0.0;
                    }
                    const double tau = -(double)j, mm = (double)(j + 1);
                    double A[K + 1][K + 1];
                    A[0][0] = mm;
                    if (CT) {
                        A[1][0] = -(mm * (mm - 1.0)) / 2.0;
                        A[1][1] = (mm - 1.0) * mm * (2.0 * mm - 1.0) / 6.0;
                    }
#define SADF_ACC(r, c, v)                                                      \
    {                                                                          \
        const double s_ = C[r][c] + fmk_dpp_iscan((v), 0.0, FmkOpAdd());       \
        C[r][c] = fmk_last_lane(s_);                                           \
        A[r][c] = s_;                                                          \
    }
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        const int cp = p == 0 ? K : p == L + 1 ? K - 1 : D0 + p - 1;
                        SADF_ACC(cp, 0, u[p]);
                        if (CT) SADF_ACC(cp, 1, tau * u[p]);
#pragma unroll
                        for (int q = p; q < P; ++q) {
                            const int cq = q == 0 ? K : q == L + 1 ? K - 1 : D0 + q - 1;
                            SADF_ACC(cp > cq ? cp : cq, cp > cq ? cq : cp, u[p] * u[q]);
                        }
                    }
#undef SADF_ACC
                    if (base + 64 >= a.min_len) {     // some lane of this step may own a window that counts
                        const double st = sadf_solve<K>(A, mm);
                        const int64_t m = j + 1;
                        if (valid && m >= a.min_len && (a.step == 1 || (uint64_t)(m - a.min_len) % (uint64_t)a.step == 0) && st == st &&
                            (best_m == 0 || st > best)) {
                            best = st;
                            best_m = m;
                        }
                    }
                    if (C[K][K] != C[K][K]) break;    // every longer window holds the NaN
                }
            }
            if (__ballot(best_m != 0) == 0) {         // no window fits, or none is usable
                ++skipped;
                continue;
            }
            const double mx = fmk_wave_max(best);     // (lanes without a window hold -inf and are left out of the minimum below)
            const int64_t m = fmk_wave_min(best_m != 0 && best == mx ? best_m : INT64_MAX);
            if (lane == b) {
                o_stat = mx;
                o_start = t - m + 1;
            }
        }
        if (lane < cnt) { a.stat[e0 + lane] = o_stat; a.start[e0 + lane] = o_start; }
    }
    if (lane == 0) {
        if (skipped) {
            atomicAdd((unsigned long long *)&a.mail->skipped, (unsigned long long)skipped);
            if (a.n_skipped) atomicAdd((unsigned long long *)a.n_skipped, (unsigned long long)skipped);
        }
        if (bad) atomicAdd((unsigned long long *)&a.mail->bad, (unsigned long long)bad);
    }
}

extern "C" int fmk_sadf_dev(fmk_ctx *ctx, const double *d_y, int64_t n, const int64_t *d_end_idx, int64_t n_end, int64_t min_len,
                            int64_t max_len, int64_t step, int64_t lags, int trend, double *d_stat, int64_t *d_start,
                            int64_t *d_n_skipped)
{
    FMK_TRY(fmk_rule_sadf(ctx, min_len, max_len, step, lags, trend, d_y, d_stat, d_start));
    if (n_end < 0 || n < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    if (n_end == 0) return FMK_OK;
    if (n == 0) return fmk_set_error(ctx, FMK_E_ARG, "sadf: end points outside the (empty) series");
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    fmk_mail::Sadf *mail = &ctx->d_mail->sadf;
    FMK_HIP(ctx, hipMemsetAsync(mail, 0, sizeof *mail, ctx->stream));
    SadfArgs a;
    a.y = d_y; a.n = n; a.ev = d_end_idx; a.n_end = n_end; a.min_len = min_len; a.max_len = max_len; a.step = step;
    a.stat = d_stat; a.start = d_start; a.n_skipped = d_n_skipped; a.mail = mail;
    int64_t grid = (int64_t)ctx->n_cu * 8;                           // persistent: 32 waves per CU take batches from the counter
    if (grid > fmk_ceil_div(n_end, 4 * SADF_BATCH * SADF_CLAIMS)) grid = fmk_ceil_div(n_end, 4 * SADF_BATCH * SADF_CLAIMS);
    switch (lags * 2 + trend) {
#define SADF_CASE(L, CT) case L * 2 + CT: k_sadf<L, CT != 0><<<(unsigned)grid, 256, 0, ctx->stream>>>(a); break
        SADF_CASE(0, 0); SADF_CASE(0, 1); SADF_CASE(1, 0); SADF_CASE(1, 1); SADF_CASE(2, 0); SADF_CASE(2, 1);
        SADF_CASE(3, 0); SADF_CASE(3, 1); SADF_CASE(4, 0); SADF_CASE(4, 1);
#undef SADF_CASE
    }
    FMK_LAUNCH_CHECK(ctx);
    fmk_mail::Sadf m;                                                // the call's one wait: the index check
    FMK_TRY(fmk_read_back(ctx, &m, mail, sizeof m));
    if (m.bad) return fmk_set_error(ctx, FMK_E_ARG, "sadf: %lld end points outside [0, %lld)", m.bad, (long long)n);
    return FMK_OK;
}
