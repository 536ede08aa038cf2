// fmk_trend.hip -- trend-scanning labels on the raw tick tape (Lopez de Prado, Machine Learning for Asset Managers, ch. 5; the
// reference reserves finmlkit/label/trend_scanning.py and leaves it empty, so DESIGN.md section 7j IS the definition).
//
// From an event t0, span L covers y[t0 .. t0+L-1], L in {min_len, min_len+step, ...} up to max_len.  With d_j = y[t0+j] - y[t0]:
//   S1 = sum d_j, Sx = sum j*d_j, S2 = sum d_j^2                        (prefix sums over the window: one walk serves every span)
//   Sxx = L(L^2-1)/12, Sxy = Sx - (L-1)/2*S1, Syy = S2 - S1^2/L, u = 1 - Sxy^2/(Sxx*Syy)
//   t(L) = Sxy / sqrt(Sxx*Syy) * sqrt((L-2)/u);  S2 == 0 -> 0;  u <= 2^-26 -> copysign(inf, Sxy);  a NaN in the span -> NaN.
// The event's span is the one of largest |t| among the non-NaN ones, the smallest L among equals.
//
// Schedule: one wave per event over a persistent grid with a work counter (k_tb's, fmk_label.hip), TR_BATCH events per visit to the
// counter.  The wave walks the window 64 ticks per step, the next step's load in flight; lane k of a step forms d, j*d, d^2 and the
// three running sums are three wave-inclusive scans (fmk_dpp_iscan) plus a carried total.  The lane that holds position j owns span
// L = j+1: it keeps its own best (|t|, L) with a strict >, so the first (smallest) L wins inside a lane, and one cross-lane arg-max
// after the walk takes the smallest L among equal |t|.  A NaN poisons every later prefix sum: what the definition asks for, so
// nothing special-cases it (the walk only stops early once the carry is NaN).  By construction an event reads 8 B x max_len: dense
// events re-read their neighbours' ticks from L2 / HBM.
#include <math.h>

#include "fmk_common.h"
#include "fmk_dpp.h"

#define TR_EXACT_U 0x1p-26       // u at or below this: the fit counts as exact
#define TR_BATCH 8               // events a wave takes from the work counter at a time (one atomic, one load of their indices, one
                                 // store of their outputs): with one event per atomic the counter's address bounds short windows
#define TR_CLAIMS 4              // batches per wave the grid is sized for, below the persistent size

struct TrArgs {
    const double *y;
    int64_t n;
    const int64_t *ev;
    int64_t n_events, min_len, max_len, step;
    int8_t *labels;
    double *t_value;
    int64_t *touch;
    double *ret;
    int64_t *n_skipped;          // may be NULL
    fmk_mail::Trend *mail;
};

__device__ __forceinline__ double tr_readlane(double v, int src)
{
    return __longlong_as_double(fmk_readlane((int64_t)__double_as_longlong(v), src));
}

// t(L) from the prefix sums of the span.  A NaN sum fails every comparison and comes out of the last line as NaN.
__device__ __forceinline__ double tr_tvalue(double S1, double Sx, double S2, int64_t L)
{
    if (S2 == 0.0) return 0.0;
    const double l = (double)L;
    const double Sxx = l * (l * l - 1.0) / 12.0;
    const double Sxy = Sx - (l - 1.0) / 2.0 * S1;
    const double Syy = S2 - S1 * S1 / l;
    const double den = Sxx * Syy;
    const double u = 1.0 - Sxy * Sxy / den;
    if (u <= TR_EXACT_U) return copysign(INFINITY, Sxy);
    return Sxy / sqrt(den) * sqrt((l - 2.0) / u);
}

__global__ __launch_bounds__(256) void k_trend(const TrArgs a)
{
    const int lane = fmk_lane();
    long long skipped = 0, bad = 0;
    for (;;) {
        unsigned long long ew = 0;
        if (lane == 0) ew = atomicAdd(&a.mail->work, (unsigned long long)TR_BATCH);
        const int64_t e0 = fmk_uniform((int64_t)ew);
        if (e0 >= a.n_events) break;
        const int cnt = a.n_events - e0 < TR_BATCH ? (int)(a.n_events - e0) : TR_BATCH;
        const int64_t my_t0 = lane < cnt ? a.ev[e0 + lane] : 0;      // lane k keeps event e0 + k: its index here, its outputs below
        int8_t o_label = 0;
        double o_t = NAN, o_ret = NAN;
        int64_t o_touch = my_t0;                                     // a skipped event: label 0, NaN, the event's own tick
        for (int k = 0; k < cnt; ++k) {
            const int64_t t0 = fmk_readlane(my_t0, k);
            const bool inside = t0 >= 0 && t0 < a.n;                 // an index outside the series is counted: the call fails
            double m = -1.0, best_t = NAN;
            int64_t best_l = 0;
            const double *__restrict__ w = a.y + (inside ? t0 : 0);
            double y0 = NAN;
            if (inside && a.max_len <= a.n - t0) {    // the longest span fits: every load below stays inside [t0, t0 + max_len)
                y0 = w[0];
                double best_abs = -1.0, c1 = 0.0, cx = 0.0, c2 = 0.0;
                double nxt = lane < a.max_len ? w[lane] : y0;
                for (int64_t base = 0; base < a.max_len; base += 64) {
                    const int64_t j = base + lane;
                    const double d = nxt - y0;        // positions past max_len: d = 0, and no span ends there
                    nxt = j + 64 < a.max_len ? w[j + 64] : y0;
                    const double s1 = c1 + fmk_dpp_iscan(d, 0.0, FmkOpAdd());
                    const double sx = cx + fmk_dpp_iscan((double)j * d, 0.0, FmkOpAdd());
                    const double s2 = c2 + fmk_dpp_iscan(d * d, 0.0, FmkOpAdd());
                    c1 = fmk_last_lane(s1);
                    cx = fmk_last_lane(sx);
                    c2 = fmk_last_lane(s2);
                    const int64_t L = j + 1;
                    if (L >= a.min_len && L <= a.max_len && (a.step == 1 || (uint64_t)(L - a.min_len) % (uint64_t)a.step == 0)) {
                        const double t = tr_tvalue(s1, sx, s2, L);
                        const double at = fabs(t);
                        if (at > best_abs) { best_abs = at; best_t = t; best_l = L; }
                    }
                    if (c2 != c2) break;              // every later span is NaN
                }
                m = fmk_wave_max(best_abs);           // no lane holds a NaN: a NaN |t| is never kept
                best_l = fmk_wave_min(best_abs == m ? best_l : INT64_MAX);
            }
            if (m < 0.0) {                            // no span fits, or all are NaN
                if (inside) ++skipped; else ++bad;
                continue;
            }
            const double t = tr_readlane(best_t, fmk_uniform((int)((best_l - 1) & 63)));
            if (lane == k) {
                o_label = t > 0.0 ? 1 : t < 0.0 ? -1 : 0;
                o_t = t;
                o_touch = t0 + best_l - 1;
                o_ret = w[best_l - 1] / y0 - 1.0;
            }
        }
        if (lane < cnt) { a.labels[e0 + lane] = o_label; a.t_value[e0 + lane] = o_t; a.touch[e0 + lane] = o_touch; a.ret[e0 + lane] = o_ret; }
    }
    if (lane == 0) {
        if (skipped) {
            atomicAdd((unsigned long long *)&a.mail->skipped, (unsigned long long)skipped);
            if (a.n_skipped) atomicAdd((unsigned long long *)a.n_skipped, (unsigned long long)skipped);
        }
        if (bad) atomicAdd((unsigned long long *)&a.mail->bad, (unsigned long long)bad);
    }
}

extern "C" int fmk_trend_scanning_dev(fmk_ctx *ctx, const double *d_y, int64_t n, const int64_t *d_event_idx, int64_t n_events,
                                      int64_t min_len, int64_t max_len, int64_t step, int8_t *d_labels, double *d_t_value,
                                      int64_t *d_touch_idx, double *d_ret, int64_t *d_n_skipped)
{
    FMK_TRY(fmk_rule_trend(ctx, min_len, max_len, step));
    if (n_events < 0 || n < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    if (n_events == 0) return FMK_OK;
    if (n == 0) return fmk_set_error(ctx, FMK_E_ARG, "trend_scanning: event indices outside the (empty) series");
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    fmk_mail::Trend *mail = &ctx->d_mail->trend;
    FMK_HIP(ctx, hipMemsetAsync(mail, 0, sizeof *mail, ctx->stream));
    TrArgs a;
    a.y = d_y; a.n = n; a.ev = d_event_idx; a.n_events = n_events; a.min_len = min_len; a.max_len = max_len; a.step = step;
    a.labels = d_labels; a.t_value = d_t_value; a.touch = d_touch_idx; a.ret = d_ret; a.n_skipped = d_n_skipped; a.mail = mail;
    int64_t grid = (int64_t)ctx->n_cu * 8;                           // persistent: 32 waves per CU take batches from the counter
    if (grid > fmk_ceil_div(n_events, 4 * TR_BATCH * TR_CLAIMS)) grid = fmk_ceil_div(n_events, 4 * TR_BATCH * TR_CLAIMS);
    k_trend<<<(unsigned)grid, 256, 0, ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    fmk_mail::Trend m;                                               // the call's one wait: the index check
    FMK_TRY(fmk_read_back(ctx, &m, mail, sizeof m));
    if (m.bad) return fmk_set_error(ctx, FMK_E_ARG, "trend_scanning: %lld event indices outside [0, %lld)", m.bad, (long long)n);
    return FMK_OK;
}
