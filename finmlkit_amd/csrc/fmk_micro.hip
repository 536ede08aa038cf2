// fmk_micro.hip -- comp_bar_microstructure_features on gfx950: Kyle's, Amihud's and Hasbrouck's lambda with their t-values and the
// Roll serial covariance / spread of every bar, from one read of price, amount and side (the arithmetic that decides
// bits is fmk_micro_rule.h).  Two schedules of fmk_bars.h, chosen by the bar's tick count alone, so a bar's bits never depend on its
// neighbours or on the tape around it:
//   * a lane per bar (k_micro_lanes) for bars of at most MC_LANE_MAX ticks: groups of 64 bars, the ticks of the longest run of bars
//     that fits staged in the wave's LDS tile by coalesced loads, every lane then walks its own bar in tick order with the tick
//     before in registers.  A wave per such bar would leave most lanes idle and pay nine 64-lane reductions per bar;
//   * a wave per bar (k_micro_waves, list mode) for the rest: the lane kernel appends those bars to a bar list as it meets them;
//     64 ticks a step, lane l takes tick 64 k + l, p_{t-1} and d_{t-1} come from lane l - 1 by a DPP shift (lane 0: lane 63 of the
//     step before, carried in SGPRs), each lane keeps nine running sums, one DPP reduction per sum at the end of the bar.
// A term at the bar's first tick and a product at its second do not exist: they are skipped by the tick's place in the bar, never
// multiplied by zero.
#include <math.h>

#include <type_traits>

#include "fmk_bars.h"
#include "fmk_dpp.h"
#include "fmk_micro_rule.h"

#define MC_LANE_MAX 32                     // ticks: the longest bar a lane takes
#define MC_TILE 1024                       // ticks of a wave's LDS tile (13 or 17 B each)

namespace {

struct McOut { double *col[FMK_MICRO_COLS]; };

__device__ __forceinline__ void mc_store(const McOut &o, int64_t b, const double (&r)[FMK_MICRO_COLS])
{
#pragma unroll
    for (int k = 0; k < FMK_MICRO_COLS; ++k) o.col[k][b] = r[k];
}
__device__ __forceinline__ void mc_store_nan(const McOut &o, int64_t b)
{
#pragma unroll
    for (int k = 0; k < FMK_MICRO_COLS; ++k) o.col[k][b] = NAN;
}

// Bars of at most MC_LANE_MAX ticks, a lane each; longer ones go to `longs`.  A bar whose close indices leave the tape ([-1, n)) is
// not read: NaN row, *bad raised (the call fails).  A bar that ends before it starts is an empty bar.
template <bool AF64>
__global__ __launch_bounds__(128) void k_micro_lanes(const double *__restrict__ price, const void *__restrict__ amount,
                                                     const int8_t *__restrict__ side, const int64_t *__restrict__ ci, int64_t nb,
                                                     int64_t n, unsigned long long *__restrict__ longs, int *__restrict__ bad, McOut o)
{
    typedef typename std::conditional<AF64, double, float>::type A;
    __shared__ double s_p[2][MC_TILE];
    __shared__ A s_a[2][MC_TILE];
    __shared__ int8_t s_s[2][MC_TILE];
    __shared__ int64_t s_ci[2][66];
    __shared__ uint8_t s_long[2][64];                                   // the group's bars for the wave schedule (their place in the group)
    const int lane = fmk_lane();
    const int w = fmk_uniform((int)(threadIdx.x >> 6));
    double *tp = s_p[w];
    A *ta = s_a[w];
    int8_t *ts = s_s[w];
    const int64_t ngroups = (nb + 63) >> 6;
    const int64_t nwaves = (int64_t)gridDim.x * 2;
    for (int64_t g = (int64_t)blockIdx.x * 2 + w; g < ngroups; g += nwaves) {
        const int64_t B0 = g * 64;
        const int nbg = fmk_lane_group_load(s_ci[w], ci, nb, B0, lane);
        int bl = 0, nlong = 0;
        while (bl < nbg) {
            const int64_t s0 = s_ci[w][bl];
            const int idx = bl + 1 + lane;
            const bool valid = idx <= nbg;
            const int64_t e_l = valid ? s_ci[w][idx] : 0;
            const int64_t s_l = valid ? s_ci[w][idx - 1] : 0;
            // the run: the leading bars that lie, one after the other, inside (s0, s0 + MC_TILE] and inside the tape
            const bool fit = valid && s0 >= -1 && s_l >= s0 && e_l >= s_l && e_l - s0 <= MC_TILE && e_l <= n - 1;
            const unsigned long long nofit = ~__builtin_amdgcn_ballot_w64(fit);
            const int m = nofit ? fmk_uniform((int)__builtin_ctzll(nofit)) : 64;
            if (m == 0) {                                               // bar bl alone: longer than the tile, or irregular
                int is_long = 0;
                if (lane == 0) {
                    const int64_t b = B0 + bl;
                    if (s_l < -1 || s_l > n - 1 || e_l < -1 || e_l > n - 1) { fmk_raise(bad); mc_store_nan(o, b); }
                    else if (e_l < s_l) mc_store_nan(o, b);
                    else { s_long[w][nlong] = (uint8_t)bl; is_long = 1; }
                }
                nlong += fmk_uniform(is_long);
                bl += 1;
                continue;
            }
            const bool owner = lane < m;
            const int L = owner ? (int)(e_l - s_l) : 0;
            const bool mine = owner && L <= MC_LANE_MAX;
            // ---- the longer bars of the run wait for the group's one append (an append per step put 10^5 atomics on the counter at
            // 250-tick bars: 1.3 of the call's 2.1 ms per 10^8 ticks)
            const unsigned long long lm = __builtin_amdgcn_ballot_w64(owner && !mine);
            if (lm) {
                const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(lm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)lm, 0u));
                if (owner && !mine) s_long[w][nlong + pos] = (uint8_t)(bl + lane);
                nlong += (int)__builtin_popcountll(lm);
            }
            // ---- fill the tile: one contiguous range, coalesced (a run without a bar of two ticks or more has nothing to read)
            const int Lw = mine ? L : 0;
            const int Lmax = fmk_dpp_reduce(Lw, 0, FmkOpMax());
            if (Lmax >= 2) {
                const int ntick = (int)(s_ci[w][bl + m] - s0);          // ticks of the m bars: (s0, s0 + ntick], ntick <= MC_TILE
                __builtin_amdgcn_wave_barrier();
                const double *gp = price + s0 + 1;
                const A *ga = (const A *)amount + s0 + 1;
                const int8_t *gs = side + s0 + 1;
#pragma unroll 4
                for (int j = lane; j < ntick; j += 64) {
                    tp[j] = gp[j];
                    ta[j] = ga[j];
                    ts[j] = gs[j];
                }
                __builtin_amdgcn_wave_barrier();
            }
            // ---- one lane per bar, in tick order
            FmkMicroSums acc;
            fmk_micro_zero(acc);
            if (Lmax >= 2) {
                const int off = Lw >= 2 ? (int)(s_l - s0) : 0;
                double pm = Lw >= 2 ? tp[off] : 0.0, dm = 0.0;
                for (int i = 1; i < Lmax; ++i) {
                    if (i < Lw) {
                        const double p = tp[off + i];
                        const FmkMicroTerm t = fmk_micro_term(p, pm, (double)ta[off + i], (double)ts[off + i]);
                        fmk_micro_add(acc, t, dm, i >= 2);
                        dm = t.d;
                        pm = p;
                    }
                }
            }
            if (mine) {
                double r[FMK_MICRO_COLS];
                fmk_micro_finish(L, acc, r);
                mc_store(o, B0 + bl + lane, r);
            }
            bl += m;
        }
        // ---- the group's bars for the wave schedule: one append (nlong <= nbg <= 64: a bar is listed once)
        if (nlong) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(longs, (unsigned long long)nlong);
            base = (unsigned long long)fmk_uniform((int64_t)base);
            __builtin_amdgcn_wave_barrier();
            if (lane < nlong) longs[FMK_BAR_LIST_HEAD + base + lane] = (unsigned long long)(B0 + s_long[w][lane]);
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// The bars of `longs` (regular, more than MC_LANE_MAX ticks), a wave each.
template <bool AF64>
__global__ __launch_bounds__(256) void k_micro_waves(const double *__restrict__ price, const void *__restrict__ amount,
                                                     const int8_t *__restrict__ side, const int64_t *__restrict__ ci,
                                                     const unsigned long long *__restrict__ longs, McOut o)
{
    const int lane = fmk_lane();
    const int wib = fmk_uniform((int)(threadIdx.x >> 6));
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + wib;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t todo = fmk_list_count(longs, 0);
    for (int64_t it = wave0; it < todo; it += nwaves) {
        const int64_t b = fmk_list_bar(longs, it);
        const int64_t s = fmk_uniform(ci[b]) + 1;                       // the bar's first tick
        const int64_t L = fmk_uniform(ci[b + 1]) - s + 1;
        const double *gp = price + s;
        const int8_t *gs = side + s;
        FmkMicroSums acc;
        fmk_micro_zero(acc);
        double cp = 0.0, cd = 0.0;                                      // p and d of lane 63 in the step before
        // the next step's ticks are in flight while this one's are worked on
        double p = 0.0, v = 0.0, sd = 0.0;
        if (lane < L) { p = gp[lane]; v = fmk_amt<AF64>(amount, s + lane); sd = (double)gs[lane]; }
        for (int64_t j0 = 0; j0 < L; j0 += 64) {
            const int64_t j = j0 + lane, jn = j + 64;
            double pn = 0.0, vn = 0.0, sn = 0.0;
            if (jn < L) { pn = gp[jn]; vn = fmk_amt<AF64>(amount, s + jn); sn = (double)gs[jn]; }
            // the look-back: every lane takes part in the shifts, whether its tick has the term or not
            const double pm = fmk_dpp_shift_up1(p, cp);
            const double d = p - pm;
            const double dm = fmk_dpp_shift_up1(d, cd);
            cp = fmk_last_lane(p);
            cd = fmk_last_lane(d);
            if (j >= 1 && j < L) {                                      // the bar's first tick has no term, its second no product
                const FmkMicroTerm t = fmk_micro_term(p, pm, v, sd);
                fmk_micro_add(acc, t, dm, j >= 2);
            }
            p = pn; v = vn; sd = sn;
        }
        acc.kxx = fmk_dpp_reduce(acc.kxx, 0.0, FmkOpAdd());
        acc.kxy = fmk_dpp_reduce(acc.kxy, 0.0, FmkOpAdd());
        acc.kyy = fmk_dpp_reduce(acc.kyy, 0.0, FmkOpAdd());
        acc.axx = fmk_dpp_reduce(acc.axx, 0.0, FmkOpAdd());
        acc.axy = fmk_dpp_reduce(acc.axy, 0.0, FmkOpAdd());
        acc.ryy = fmk_dpp_reduce(acc.ryy, 0.0, FmkOpAdd());
        acc.hxx = fmk_dpp_reduce(acc.hxx, 0.0, FmkOpAdd());
        acc.hxy = fmk_dpp_reduce(acc.hxy, 0.0, FmkOpAdd());
        acc.q = fmk_dpp_reduce(acc.q, 0.0, FmkOpAdd());
        double r[FMK_MICRO_COLS];
        fmk_micro_finish(L, acc, r);
        if (lane == 0) mc_store(o, b, r);
    }
}

}  // namespace

extern "C" int fmk_comp_bar_microstructure_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount, int amount_is_f64, int64_t n,
                                               const int64_t *d_close_idx, int64_t n_idx, const int8_t *d_side,
                                               const fmk_microstructure_out *d_out)
{
    FMK_TRY(fmk_rule_micro(ctx, d_price, d_amount, amount_is_f64, n, d_close_idx, n_idx, d_side, d_out));
    if (n_idx == 1) return FMK_OK;
    const int64_t nb = n_idx - 1;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    fmk_mail::Micro *mail = &ctx->d_mail->micro;
    FMK_HIP(ctx, hipMemsetAsync(mail, 0, sizeof *mail, ctx->stream));
    void *lp;
    FMK_TRY(fmk_alloc(ctx, sizeof(unsigned long long) * fmk_bar_list_words(nb), &lp));
    unsigned long long *longs = (unsigned long long *)lp;
    McOut o;
    double *const cols[FMK_MICRO_COLS] = {d_out->kyle_lambda, d_out->kyle_t, d_out->amihud_lambda, d_out->amihud_t,
                                          d_out->hasbrouck_lambda, d_out->hasbrouck_t, d_out->serial_cov, d_out->roll_spread};
    for (int k = 0; k < FMK_MICRO_COLS; ++k) o.col[k] = cols[k];
    int rc = FMK_OK;
    do {
        if (hipMemsetAsync(longs, 0, FMK_BAR_LIST_CLEAR, ctx->stream) != hipSuccess) { rc = fmk_set_error(ctx, FMK_E_HIP, "comp_bar_microstructure: memset"); break; }
        int64_t g1 = fmk_ceil_div(fmk_ceil_div(nb, 64), 2), g2 = fmk_ceil_div(nb, 4);
        if (g1 > (int64_t)ctx->n_cu * 16) g1 = (int64_t)ctx->n_cu * 16;
        if (g2 > (int64_t)ctx->n_cu * 8) g2 = (int64_t)ctx->n_cu * 8;
        if (amount_is_f64) {
            k_micro_lanes<true><<<(unsigned)g1, 128, 0, ctx->stream>>>(d_price, d_amount, d_side, d_close_idx, nb, n, longs, &mail->bad, o);
            k_micro_waves<true><<<(unsigned)g2, 256, 0, ctx->stream>>>(d_price, d_amount, d_side, d_close_idx, longs, o);
        } else {
            k_micro_lanes<false><<<(unsigned)g1, 128, 0, ctx->stream>>>(d_price, d_amount, d_side, d_close_idx, nb, n, longs, &mail->bad, o);
            k_micro_waves<false><<<(unsigned)g2, 256, 0, ctx->stream>>>(d_price, d_amount, d_side, d_close_idx, longs, o);
        }
        if (hipGetLastError() != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "comp_bar_microstructure: launch");
    } while (0);
    (void)fmk_free(ctx, lp);                                            // stream-ordered: the kernels above are queued before it
    FMK_TRY(rc);
    fmk_mail::Micro m;                                                  // the call's one wait: the index check
    FMK_TRY(fmk_read_back(ctx, &m, mail, sizeof m));
    if (m.bad) return fmk_set_error(ctx, FMK_E_ARG, "comp_bar_microstructure: a close index outside [-1, %lld)", (long long)n);
    return FMK_OK;
}
