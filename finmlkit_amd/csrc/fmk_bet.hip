// fmk_bet.hip -- bet sizing (Lopez de Prado, Advances in Financial Machine Learning, ch. 10) on label spans: the average of the
// active signals per tick of a resident tape, discretised, and the budget approach's position (the arithmetic that
// decides a bit is fmk_bet_rule.h).  The same kind of loop as label_concurrency (fmk_label.hip): a difference array over the tape
// and one device-wide scan.
//   k_bet_mark       one thread per event: checks the span and the signal BEFORE it touches the arrays, then integer atomics
//                    +q / -q (int64) and +1 / -1 (int32) at ev and tc.  Integer sums: the result does not depend on arrival order
//   k_bet_tile_sums  one workgroup per tile of BET_TILE ticks: the tile's (sum, count)
//   k_fmk_agg_scan   (fmk_wgscan.h) one workgroup, BET_AGG_UNIT tile totals per trip
//   k_bet_apply      scans the tile again with its carry, forms the quotient, discretises, stores float64 (and the int16 count)
// A thread owns BET_VEC = 4 consecutive ticks of a row of BET_ROW = 1024: one 16-byte load of counts, two of sums, two 16-byte
// stores of values.  The difference arrays are padded to whole tiles and zeroed, so the loads need no bounds; the stores check n.
// The two arrays (12 B/tick per pass) rather than one shared 64-bit word (8 B/tick): see DESIGN.md §7q, "Layout".
// The budget approach runs the same mark and scan on the two side counts; k_bud_scan<false> only reduces the two maxima,
// k_bud_scan<true> forms the quotients.  k_bet_gather: out[k] = path[idx[k]].
#include "fmk_wgscan.h"
#include "fmk_bet_rule.h"

#define BET_TILE 4096
#define BET_VEC 4
#define BET_ROW (256 * BET_VEC)
#define BET_ROWS (BET_TILE / BET_ROW)
#define BET_AGG_UNIT 1024

namespace {

struct BetSum {
    using T = FmkBetAcc;
    static __device__ __forceinline__ T identity() { return T{0, 0, 0}; }
    static __device__ __forceinline__ T combine(const T &first, const T &then) { return fmk_bet_combine(first, then); }
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ T dpp(const T &v)
    {
        T r;
        r.s = fmk_dpp<CTRL, ROW_MASK>((int64_t)0, v.s);
        r.c = fmk_dpp<CTRL, ROW_MASK>(0, (int)v.c);
        r.pad = 0;
        return r;
    }
};

struct BudSum {
    using T = FmkBetSides;
    static __device__ __forceinline__ T identity() { return T{0, 0}; }
    static __device__ __forceinline__ T combine(const T &first, const T &then) { return fmk_bet_sides_combine(first, then); }
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ T dpp(const T &v)
    {
        T r;
        r.l = fmk_dpp<CTRL, ROW_MASK>(0, (int)v.l);
        r.s = fmk_dpp<CTRL, ROW_MASK>(0, (int)v.s);
        return r;
    }
};

__device__ __forceinline__ int bet_wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

}  // namespace

__global__ __launch_bounds__(256) void k_bet_mark(const int64_t *__restrict__ ev, const int64_t *__restrict__ touch,
                                                  const double *__restrict__ signal, int64_t n_events, int64_t n,
                                                  int64_t *__restrict__ ds, int *__restrict__ dc, fmk_mail::Bet *mail)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_events) return;
    const int64_t s = ev[i], t = touch[i];
    if (s < 0 || t < s || t >= n) { atomicAdd((unsigned long long *)&mail->bad, 1ull); return; }
    int64_t q;
    if (!fmk_bet_quantise(signal[i], &q)) { atomicAdd((unsigned long long *)&mail->bad_signal, 1ull); return; }
    if (t == s) return;                            // open on ev <= tick < tc: never open
    if (q) {
        atomicAdd((unsigned long long *)&ds[s], (unsigned long long)q);
        atomicAdd((unsigned long long *)&ds[t], (unsigned long long)(-q));
    }
    atomicAdd(&dc[s], 1);
    atomicAdd(&dc[t], -1);
}

__global__ __launch_bounds__(256) void k_bet_tile_sums(const int64_t *__restrict__ ds, const int *__restrict__ dc,
                                                       FmkBetAcc *__restrict__ tile_sum)
{
    __shared__ int64_t ss[4];
    __shared__ int sc[4];
    const int64_t base = (int64_t)blockIdx.x * BET_TILE;
    uint64_t s = 0;
    unsigned c = 0;
#pragma unroll
    for (int r = 0; r < BET_ROWS; ++r) {
        const int64_t j = base + r * BET_ROW + threadIdx.x * BET_VEC;
        const int4 c4 = *reinterpret_cast<const int4 *>(dc + j);
        const longlong2 a = *reinterpret_cast<const longlong2 *>(ds + j);
        const longlong2 b = *reinterpret_cast<const longlong2 *>(ds + j + 2);
        c += (unsigned)c4.x + (unsigned)c4.y + (unsigned)c4.z + (unsigned)c4.w;
        s += (uint64_t)a.x + (uint64_t)a.y + (uint64_t)b.x + (uint64_t)b.y;
    }
    s = fmk_wave_sum(s);
    c = fmk_wave_sum(c);
    if (fmk_lane() == 0) { ss[threadIdx.x >> 6] = (int64_t)s; sc[threadIdx.x >> 6] = (int)c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        FmkBetAcc t;
        t.s = (int64_t)((uint64_t)ss[0] + (uint64_t)ss[1] + (uint64_t)ss[2] + (uint64_t)ss[3]);
        t.c = (int32_t)((unsigned)sc[0] + (unsigned)sc[1] + (unsigned)sc[2] + (unsigned)sc[3]);
        t.pad = 0;
        tile_sum[blockIdx.x] = t;
    }
}

// value[j] = discretise(value(S[j], c[j])), count[j] = int16(c[j]); the largest count above the bound goes to the mailbox
template <bool COUNT>
__global__ __launch_bounds__(256) void k_bet_apply(const int64_t *__restrict__ ds, const int *__restrict__ dc, int64_t n,
                                                   const FmkBetAcc *__restrict__ tile_off, double step, double *__restrict__ out,
                                                   int16_t *__restrict__ cnt, int vec_ok, fmk_mail::Bet *mail)
{
    __shared__ FmkBetAcc ws[4];
    const int64_t base = (int64_t)blockIdx.x * BET_TILE;
    FmkBetAcc run = tile_off[blockIdx.x];
    int cmax = 0;
    for (int r = 0; r < BET_ROWS; ++r) {
        const int64_t row = base + (int64_t)r * BET_ROW;
        if (row >= n) break;                       // the same for the whole workgroup
        const int64_t j = row + threadIdx.x * BET_VEC;
        const int4 c4 = *reinterpret_cast<const int4 *>(dc + j);
        const longlong2 a = *reinterpret_cast<const longlong2 *>(ds + j);
        const longlong2 b = *reinterpret_cast<const longlong2 *>(ds + j + 2);
        FmkBetAcc p[BET_VEC];
        p[0] = FmkBetAcc{a.x, c4.x, 0};
        p[1] = fmk_bet_combine(p[0], FmkBetAcc{a.y, c4.y, 0});
        p[2] = fmk_bet_combine(p[1], FmkBetAcc{b.x, c4.z, 0});
        p[3] = fmk_bet_combine(p[2], FmkBetAcc{b.y, c4.w, 0});
        FmkBetAcc tot;
        const FmkBetAcc ex = fmk_wg_exclusive<BetSum, 4>(p[3], ws, &tot);
        const FmkBetAcc before = fmk_bet_combine(run, ex);
        double v[BET_VEC];
        int c[BET_VEC];
#pragma unroll
        for (int k = 0; k < BET_VEC; ++k) {
            const FmkBetAcc at = fmk_bet_combine(before, p[k]);
            c[k] = at.c;
            v[k] = fmk_bet_discretise(fmk_bet_value(at.s, at.c), step);
            if (j + k < n) cmax = c[k] > cmax ? c[k] : cmax;
        }
        if (vec_ok && j + BET_VEC <= n) {
            *reinterpret_cast<double2 *>(out + j) = double2{v[0], v[1]};
            *reinterpret_cast<double2 *>(out + j + 2) = double2{v[2], v[3]};
            if (COUNT) *reinterpret_cast<short4 *>(cnt + j) = short4{(short)c[0], (short)c[1], (short)c[2], (short)c[3]};
        } else {
#pragma unroll
            for (int k = 0; k < BET_VEC; ++k)
                if (j + k < n) {
                    out[j + k] = v[k];
                    if (COUNT) cnt[j + k] = (int16_t)c[k];
                }
        }
        run = fmk_bet_combine(run, tot);
    }
    cmax = bet_wave_max(cmax);
    if (fmk_lane() == 0 && cmax > FMK_BET_MAX_CONC) atomicMax(&mail->max_c, cmax);
}

// ---- the budget approach
__global__ __launch_bounds__(256) void k_bud_mark(const int64_t *__restrict__ ev, const int64_t *__restrict__ touch,
                                                  const int8_t *__restrict__ side, int64_t n_events, int64_t n, int *__restrict__ dl,
                                                  int *__restrict__ dsh, fmk_mail::Bet *mail)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_events) return;
    const int64_t s = ev[i], t = touch[i];
    if (s < 0 || t < s || t >= n) { atomicAdd((unsigned long long *)&mail->bad, 1ull); return; }
    const int sd = side[i];
    if (t == s || sd == 0) return;
    int *d = sd > 0 ? dl : dsh;
    atomicAdd(&d[s], 1);
    atomicAdd(&d[t], -1);
}

__global__ __launch_bounds__(256) void k_bud_tile_sums(const int *__restrict__ dl, const int *__restrict__ dsh,
                                                       FmkBetSides *__restrict__ tile_sum)
{
    __shared__ int sl[4], ss[4];
    const int64_t base = (int64_t)blockIdx.x * BET_TILE;
    unsigned l = 0, s = 0;
#pragma unroll
    for (int r = 0; r < BET_ROWS; ++r) {
        const int64_t j = base + r * BET_ROW + threadIdx.x * BET_VEC;
        const int4 a = *reinterpret_cast<const int4 *>(dl + j);
        const int4 b = *reinterpret_cast<const int4 *>(dsh + j);
        l += (unsigned)a.x + (unsigned)a.y + (unsigned)a.z + (unsigned)a.w;
        s += (unsigned)b.x + (unsigned)b.y + (unsigned)b.z + (unsigned)b.w;
    }
    l = fmk_wave_sum(l);
    s = fmk_wave_sum(s);
    if (fmk_lane() == 0) { sl[threadIdx.x >> 6] = (int)l; ss[threadIdx.x >> 6] = (int)s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        FmkBetSides t;
        t.l = (int32_t)((unsigned)sl[0] + (unsigned)sl[1] + (unsigned)sl[2] + (unsigned)sl[3]);
        t.s = (int32_t)((unsigned)ss[0] + (unsigned)ss[1] + (unsigned)ss[2] + (unsigned)ss[3]);
        tile_sum[blockIdx.x] = t;
    }
}

// APPLY false: the two maxima over the tape into the mailbox; true: m[j] from the counts and the maxima found before
template <bool APPLY>
__global__ __launch_bounds__(256) void k_bud_scan(const int *__restrict__ dl, const int *__restrict__ dsh, int64_t n,
                                                  const FmkBetSides *__restrict__ tile_off, double *__restrict__ out,
                                                  int64_t *__restrict__ out_max2, int vec_ok, fmk_mail::Bet *mail)
{
    __shared__ FmkBetSides ws[4];
    const int64_t base = (int64_t)blockIdx.x * BET_TILE;
    FmkBetSides run = tile_off[blockIdx.x];
    int ml = 0, ms = 0;
    if (APPLY) {
        ml = mail->max2[0];
        ms = mail->max2[1];
        if (blockIdx.x == 0 && threadIdx.x == 0 && out_max2) { out_max2[0] = ml; out_max2[1] = ms; }
    }
    int top_l = 0, top_s = 0;
    for (int r = 0; r < BET_ROWS; ++r) {
        const int64_t row = base + (int64_t)r * BET_ROW;
        if (row >= n) break;
        const int64_t j = row + threadIdx.x * BET_VEC;
        const int4 a = *reinterpret_cast<const int4 *>(dl + j);
        const int4 b = *reinterpret_cast<const int4 *>(dsh + j);
        FmkBetSides p[BET_VEC];
        p[0] = FmkBetSides{a.x, b.x};
        p[1] = fmk_bet_sides_combine(p[0], FmkBetSides{a.y, b.y});
        p[2] = fmk_bet_sides_combine(p[1], FmkBetSides{a.z, b.z});
        p[3] = fmk_bet_sides_combine(p[2], FmkBetSides{a.w, b.w});
        FmkBetSides tot;
        const FmkBetSides ex = fmk_wg_exclusive<BudSum, 4>(p[3], ws, &tot);
        const FmkBetSides before = fmk_bet_sides_combine(run, ex);
        double v[BET_VEC];
#pragma unroll
        for (int k = 0; k < BET_VEC; ++k) {
            const FmkBetSides at = fmk_bet_sides_combine(before, p[k]);
            if (APPLY) v[k] = fmk_bet_budget_value(at.l, at.s, ml, ms);
            else if (j + k < n) {
                top_l = at.l > top_l ? at.l : top_l;
                top_s = at.s > top_s ? at.s : top_s;
            }
        }
        if (APPLY) {
            if (vec_ok && j + BET_VEC <= n) {
                *reinterpret_cast<double2 *>(out + j) = double2{v[0], v[1]};
                *reinterpret_cast<double2 *>(out + j + 2) = double2{v[2], v[3]};
            } else {
#pragma unroll
                for (int k = 0; k < BET_VEC; ++k)
                    if (j + k < n) out[j + k] = v[k];
            }
        }
        run = fmk_bet_sides_combine(run, tot);
    }
    if (!APPLY) {
        // one atomic per workgroup, and only where it would raise the maximum: the value only grows, so a stale read costs an atomic
        // too many, never one too few (an atomic per wave on the one address was 20 of the call's 28 ms at 10^9 ticks)
        __shared__ int tl[4], ts[4];
        top_l = bet_wave_max(top_l);
        top_s = bet_wave_max(top_s);
        if (fmk_lane() == 0) { tl[threadIdx.x >> 6] = top_l; ts[threadIdx.x >> 6] = top_s; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < 4; ++k) {
                top_l = tl[k] > top_l ? tl[k] : top_l;
                top_s = ts[k] > top_s ? ts[k] : top_s;
            }
            if (top_l > *(volatile int *)&mail->max2[0]) atomicMax(&mail->max2[0], top_l);
            if (top_s > *(volatile int *)&mail->max2[1]) atomicMax(&mail->max2[1], top_s);
        }
    }
}

__global__ __launch_bounds__(256) void k_bet_gather(const double *__restrict__ path, int64_t n, const int64_t *__restrict__ idx,
                                                    int64_t n_idx, double *__restrict__ out, fmk_mail::Bet *mail)
{
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n_idx; k += (int64_t)gridDim.x * 256) {
        const int64_t i = idx[k];
        if (i < 0 || i >= n) { atomicAdd((unsigned long long *)&mail->bad_idx, 1ull); continue; }
        out[k] = path[i];
    }
}

// ---------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------
static int bet_check_mail(fmk_ctx *ctx, const char *what, int64_t n)
{
    fmk_mail::Bet m;
    FMK_TRY(fmk_read_back(ctx, &m, &ctx->d_mail->bet, sizeof m));
    if (m.bad)
        return fmk_set_error(ctx, FMK_E_ARG, "%s: %lld events outside 0 <= event_idx <= touch_idx < %lld", what, m.bad, (long long)n);
    if (m.bad_signal)
        return fmk_set_error(ctx, FMK_E_ARG, "%s: %lld signals are NaN or outside [-1, 1]", what, m.bad_signal);
    if (m.max_c > FMK_BET_MAX_CONC)
        return fmk_set_error(ctx, FMK_E_ARG, "%s: a concurrency of %d passes int16 (32767)", what, m.max_c);
    if (m.max2[0] > FMK_BET_MAX_CONC || m.max2[1] > FMK_BET_MAX_CONC)
        return fmk_set_error(ctx, FMK_E_ARG, "%s: a concurrency of %d on one side passes int16 (32767)", what,
                             m.max2[0] > m.max2[1] ? m.max2[0] : m.max2[1]);
    if (m.bad_idx)
        return fmk_set_error(ctx, FMK_E_ARG, "%s: %lld indices outside [0, %lld)", what, m.bad_idx, (long long)n);
    return FMK_OK;
}

// the launches of the path; the caller reads the mailbox
static int bet_path_launch(fmk_ctx *ctx, const int64_t *d_ev, const int64_t *d_tc, const double *d_signal, int64_t n_events,
                           int64_t n, double step, double *d_out, int16_t *d_cnt)
{
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    fmk_mail::Bet *mail = &ctx->d_mail->bet;
    FMK_HIP(ctx, hipMemsetAsync(mail, 0, sizeof *mail, ctx->stream));
    const int64_t tiles = fmk_ceil_div(n, BET_TILE), padded = tiles * BET_TILE;
    const size_t diff_bytes = (size_t)padded * (sizeof(int64_t) + sizeof(int));
    void *blk;
    FMK_TRY(fmk_alloc(ctx, diff_bytes + (size_t)tiles * sizeof(FmkBetAcc), &blk));
    int64_t *ds = (int64_t *)blk;
    int *dc = (int *)(ds + padded);
    FmkBetAcc *tile = (FmkBetAcc *)(dc + padded);                  // padded is a multiple of 4096: 16-byte aligned
    hipError_t le = hipMemsetAsync(blk, 0, diff_bytes, ctx->stream);
    if (le == hipSuccess) {
        const int vec_ok = ((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_cnt & 7) == 0;
        k_bet_mark<<<(unsigned)fmk_ceil_div(n_events, 256), 256, 0, ctx->stream>>>(d_ev, d_tc, d_signal, n_events, n, ds, dc, mail);
        k_bet_tile_sums<<<(unsigned)tiles, 256, 0, ctx->stream>>>(ds, dc, tile);
        k_fmk_agg_scan<BetSum, BET_AGG_UNIT><<<1, BET_AGG_UNIT, 0, ctx->stream>>>(tile, tiles, nullptr);
        if (d_cnt) k_bet_apply<true><<<(unsigned)tiles, 256, 0, ctx->stream>>>(ds, dc, n, tile, step, d_out, d_cnt, vec_ok, mail);
        else k_bet_apply<false><<<(unsigned)tiles, 256, 0, ctx->stream>>>(ds, dc, n, tile, step, d_out, nullptr, vec_ok, mail);
        le = hipGetLastError();
    }
    FMK_TRY(fmk_free(ctx, blk));
    FMK_HIP(ctx, le);
    return FMK_OK;
}

extern "C" int fmk_bet_size_path_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, const double *d_signal,
                                     int64_t n_events, int64_t n, double step, double *d_out_value, int16_t *d_out_count)
{
    FMK_TRY(fmk_rule_bet(ctx, "bet_size_path", n_events, n, step));
    FMK_TRY(bet_path_launch(ctx, d_event_idx, d_touch_idx, d_signal, n_events, n, step, d_out_value, d_out_count));
    return bet_check_mail(ctx, "bet_size_path", n);
}

extern "C" int fmk_bet_size_at_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, const double *d_signal,
                                   int64_t n_events, int64_t n, double step, const int64_t *d_idx, int64_t n_idx, double *d_out)
{
    FMK_TRY(fmk_rule_bet(ctx, "bet_size_at", n_events, n, step));
    if (n_idx < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    void *path;
    FMK_TRY(fmk_alloc(ctx, (size_t)n * sizeof(double), &path));
    int rc = bet_path_launch(ctx, d_event_idx, d_touch_idx, d_signal, n_events, n, step, (double *)path, nullptr);
    hipError_t le = hipSuccess;
    if (rc == FMK_OK && n_idx) {
        k_bet_gather<<<fmk_grid_blocks(ctx, n_idx), 256, 0, ctx->stream>>>((const double *)path, n, d_idx, n_idx, d_out,
                                                                          &ctx->d_mail->bet);
        le = hipGetLastError();
    }
    FMK_TRY(fmk_free(ctx, path));                                  // stream-ordered: the next user comes after the gather
    FMK_TRY(rc);
    FMK_HIP(ctx, le);
    return bet_check_mail(ctx, "bet_size_at", n);
}

extern "C" int fmk_bet_size_budget_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, const int8_t *d_side,
                                       int64_t n_events, int64_t n, double *d_out_m, int64_t *d_out_max2)
{
    FMK_TRY(fmk_rule_bet(ctx, "bet_size_budget", n_events, n, 0.0));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    fmk_mail::Bet *mail = &ctx->d_mail->bet;
    FMK_HIP(ctx, hipMemsetAsync(mail, 0, sizeof *mail, ctx->stream));
    const int64_t tiles = fmk_ceil_div(n, BET_TILE), padded = tiles * BET_TILE;
    const size_t diff_bytes = (size_t)padded * 2 * sizeof(int);
    void *blk;
    FMK_TRY(fmk_alloc(ctx, diff_bytes + (size_t)tiles * sizeof(FmkBetSides), &blk));
    int *dl = (int *)blk, *dsh = dl + padded;
    FmkBetSides *tile = (FmkBetSides *)(dsh + padded);
    hipError_t le = hipMemsetAsync(blk, 0, diff_bytes, ctx->stream);
    if (le == hipSuccess) {
        const int vec_ok = ((uintptr_t)d_out_m & 15) == 0;
        k_bud_mark<<<(unsigned)fmk_ceil_div(n_events, 256), 256, 0, ctx->stream>>>(d_event_idx, d_touch_idx, d_side, n_events, n, dl,
                                                                                  dsh, mail);
        k_bud_tile_sums<<<(unsigned)tiles, 256, 0, ctx->stream>>>(dl, dsh, tile);
        k_fmk_agg_scan<BudSum, BET_AGG_UNIT><<<1, BET_AGG_UNIT, 0, ctx->stream>>>(tile, tiles, nullptr);
        k_bud_scan<false><<<(unsigned)tiles, 256, 0, ctx->stream>>>(dl, dsh, n, tile, nullptr, nullptr, 0, mail);
        k_bud_scan<true><<<(unsigned)tiles, 256, 0, ctx->stream>>>(dl, dsh, n, tile, d_out_m, d_out_max2, vec_ok, mail);
        le = hipGetLastError();
    }
    FMK_TRY(fmk_free(ctx, blk));
    FMK_HIP(ctx, le);
    return bet_check_mail(ctx, "bet_size_budget", n);
}

extern "C" int fmk_bet_geometry(int64_t *out3)
{
    if (!out3) return FMK_E_ARG;
    out3[0] = BET_TILE;
    out3[1] = BET_ROW;
    out3[2] = BET_AGG_UNIT;
    return FMK_OK;
}
