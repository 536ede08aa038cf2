// fmk_label.hip -- triple-barrier labels and sample weights on the raw tick tape (finmlkit/label/tbm.py, label/weights.py).
//
// triple_barrier (tbm.py:11-158): one wave per event over a persistent grid with a work counter.  The reference's loop, restated:
//   t1_idx   = last tick with float64(ts[j]) <= float64(t0) + vertical_barrier * 1e9 (searchsorted on a float64 key, tbm.py:95-96);
//   the ticks skipped by min_close_time are a prefix of the window (timestamps are sorted): the first open tick is found by a
//   search, the walk then reads `close` only (8 B/tick);
//   ret_j    = (log(close[j]) - log(close[t0])) * side with the host's log (fmk_log.h), first touch = first j with
//   ret_j >= upper || ret_j <= lower: one ballot per 64 ticks;
//   max_urbr / max_lrbr are maxima of correctly rounded quotients ret / barrier: fl(x / U) is monotone in x, so they follow from
//   the max and the min of ret over the walked ticks.
// Two schedules:
//   direct -- every tick of [first open tick, touch] is walked;
//   long   -- (min, max) of log(close) per block of LB_BLOCK ticks and per LB_FAN blocks, built once per call (16 B per block).
//             ret is monotone in log(close[j]), so the extrema of ret over a block are the images of the block's extrema: a block
//             whose extrema reach neither barrier holds no touch and still gives its exact extrema to the two ratios, and the first
//             block whose extrema reach a barrier HOLDS the first touch (the extrema are attained).  Only that block is opened.
//
// average_uniqueness / return_attribution (weights.py:7-103): concurrency = a difference array (int32 atomics) and one scan over the
// tape, cast to int16 (the reference's int16 additions wrap mod 2^16: the same value).  The weights share one pass over close +
// concurrency (10 B/tick) that leaves per-block sums of 1 / c and of log(close[j] / close[j-1]) / c; an event of L ticks then
// costs O(L / LW_BLOCK + LW_BLOCK).  Sums are re-associated: DESIGN.md section 5's 1e-9 contract.
#include <math.h>
#include <stdlib.h>

#include "fmk_common.h"
#include "fmk_log.h"
#include "fmk_wgscan.h"

#define LB_BLOCK 1024            // ticks per level-1 table entry
#define LB_FAN 64                // level-1 entries per level-2 entry (one lane each)
#define LB_LONG_MIN 65536.0      // expected ticks per window from which the long schedule serves the call
#define LW_BLOCK 1024            // ticks per partial sum of the weights pass

struct LbMinMax { double mn, mx; };

struct TbArgs {
    const int64_t *ts;
    const double *close;
    int64_t n;
    const int64_t *ev;
    const double *tgt;
    const int8_t *side;          // NULL: side labels (all +1)
    int64_t n_events;
    double bottom, top, vb_ns, mc_ns, min_ret;
    int8_t *labels;
    int64_t *touch;
    double *ret, *ratio;
    int64_t *n_skipped;          // may be NULL
    const LbMinMax *t1, *t2;     // the long schedule's tables
    fmk_mail::Label *mail;
};

__device__ __forceinline__ double lb_readlane(double v, int src)
{
    return __longlong_as_double(fmk_readlane((int64_t)__double_as_longlong(v), src));
}

// largest j in [lo0, n) with float64(ts[j]) <= key; the caller knows that lo0 qualifies.  Gallop, then bisect (wave-uniform).
__device__ __forceinline__ int64_t lb_last_le(const int64_t *__restrict__ ts, int64_t lo0, int64_t n, double key)
{
    if (key == INFINITY) return n - 1;
    int64_t lo = lo0, hi = n, step = 64;
    for (;;) {
        const int64_t p = lo + step;
        if (p >= n) break;
        if ((double)ts[p] <= key) { lo = p; step <<= 1; } else { hi = p; break; }
    }
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((double)ts[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

// first j in (i0, t1] with float64(ts[j] - t0) >= mc_ns (tbm.py:111-114), t1 + 1 when there is none
__device__ __forceinline__ int64_t lb_first_open(const int64_t *__restrict__ ts, int64_t i0, int64_t t1, int64_t t0, double mc_ns)
{
    int64_t lo = i0, hi = t1 + 1, step = 1;
    for (;;) {
        const int64_t p = lo + step;
        if (p > t1) break;
        if ((double)(ts[p] - t0) >= mc_ns) { hi = p; break; }
        lo = p;
        step <<= 1;
    }
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((double)(ts[mid] - t0) >= mc_ns) hi = mid; else lo = mid;
    }
    return hi;
}

// The ticks [j0, j1] in order, 256 per step (four loads in flight per lane).  -> true at the first touch (touch, ret set);
// mx / mn: per-lane extrema of ret over the ticks up to the touch.
__device__ __forceinline__ bool tb_walk(const double *__restrict__ close, int64_t j0, int64_t j1, double base, double s, double U,
                                        double L, double &mx, double &mn, double &ret, int64_t &touch, long long &walked)
{
    const int lane = fmk_lane();
    for (int64_t j = j0; j <= j1; j += 256) {
        double p[4], r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t jj = j + k * 64 + lane;
            p[k] = jj <= j1 ? close[jj] : 1.0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (fmk_log_host(p[k]) - base) * s;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t c0 = j + k * 64;
            if (c0 > j1) break;
            const bool valid = c0 + lane <= j1;
            const uint64_t hit = __ballot(valid && (r[k] >= U || r[k] <= L));
            if (hit) {
                const int f = __ffsll((unsigned long long)hit) - 1;
                if (lane <= f) { mx = r[k] > mx ? r[k] : mx; mn = r[k] < mn ? r[k] : mn; }
                ret = lb_readlane(r[k], fmk_uniform(f));
                touch = c0 + f;
                walked += touch - j0 + 1;
                return true;
            }
            if (valid) { mx = r[k] > mx ? r[k] : mx; mn = r[k] < mn ? r[k] : mn; }
        }
    }
    walked += j1 - j0 + 1;
    return false;
}

// extrema of ret over a table entry: ret is monotone in log(close) for every side (side 0: +-0.0 everywhere).  An image that is
// NaN (inf - inf with an infinite base, +-inf * 0) is left out like the walk leaves out a NaN tick: every non-NaN ret of the
// entry is then the other image, so fmax / fmin give the entry's extrema (both NaN: no tick of it can touch).  Side 0 over a
// finite base: +-0.0 at every finite tick and NaN elsewhere, which (-inf, +inf) extrema cannot tell from "NaN everywhere"; the entry
// says 0 and the walk of the block decides (0 touches only a barrier that is <= 0 / >= 0, and 0 changes neither ratio).
__device__ __forceinline__ void lb_entry(const LbMinMax e, double base, double s, double &hi, double &lo)
{
    if (s == 0.0 && isfinite(base)) { hi = lo = 0.0; return; }
    const double r1 = (e.mx - base) * s, r2 = (e.mn - base) * s;
    hi = fmax(r1, r2);
    lo = fmin(r1, r2);
}

template <bool TABLE>
__global__ __launch_bounds__(256) void k_tb(const TbArgs a)
{
    const int lane = fmk_lane();
    long long walked = 0, opened = 0, skipped = 0;
    for (;;) {
        unsigned long long ew = 0;
        if (lane == 0) ew = atomicAdd(&a.mail->work, 1ull);
        const int64_t e = fmk_uniform((int64_t)ew);
        if (e >= a.n_events) break;
        const int64_t i0 = a.ev[e];
        bool live = i0 >= 0 && i0 < a.n;          // an index outside the tape was counted by k_lb_precheck: the call fails
        int64_t t1 = 0, t0 = 0;
        if (live) {
            t0 = a.ts[i0];
            t1 = lb_last_le(a.ts, i0, a.n, (double)t0 + a.vb_ns);
            if (t1 <= i0) { live = false; ++skipped; }
        }
        if (!live) {                              // tbm.py:97-100: label 0, NaN; the touch index is the event's own tick
            if (lane == 0) { a.labels[e] = 0; a.touch[e] = i0; a.ret[e] = NAN; a.ratio[e] = NAN; }
            continue;
        }
        const double tgt = a.tgt[e];
        const double U = tgt * a.top, L = -tgt * a.bottom;
        const bool uv = isfinite(U) && U != 0.0, lv = isfinite(L) && L != 0.0;
        const double s = a.side ? (double)a.side[e] : 1.0;
        const double base = fmk_log_host(a.close[i0]);
        const int64_t js = lb_first_open(a.ts, i0, t1, t0, a.mc_ns);
        double mx = -INFINITY, mn = INFINITY, ret = 0.0;
        int64_t touch = t1;
        if (js <= t1) {
            bool hit = false;
            int64_t b = (js + LB_BLOCK - 1) / LB_BLOCK;            // the blocks [b, bB) lie inside [js, t1]
            const int64_t bB = (t1 + 1) / LB_BLOCK;
            if (!TABLE || b >= bB) {
                hit = tb_walk(a.close, js, t1, base, s, U, L, mx, mn, ret, touch, walked);
            } else {
                if (js < b * LB_BLOCK) hit = tb_walk(a.close, js, b * LB_BLOCK - 1, base, s, U, L, mx, mn, ret, touch, walked);
                while (!hit && b < bB) {
                    double hi, lo;
                    if ((b & (LB_FAN - 1)) == 0 && b + LB_FAN <= bB) {               // one lane per LB_FAN blocks
                        const int64_t left = (bB - b) / LB_FAN;
                        const int cnt = left < 64 ? (int)left : 64;
                        const bool valid = lane < cnt;
                        LbMinMax en = {0.0, 0.0};
                        if (valid) en = a.t2[b / LB_FAN + lane];
                        lb_entry(en, base, s, hi, lo);
                        const uint64_t may = __ballot(valid && (hi >= U || lo <= L));
                        const int f = may ? __ffsll((unsigned long long)may) - 1 : cnt;
                        if (lane < f) { mx = hi > mx ? hi : mx; mn = lo < mn ? lo : mn; }
                        b += (int64_t)f * LB_FAN;
                        if (!may) continue;
                    }
                    const int64_t to_fan = LB_FAN - (b & (LB_FAN - 1)), left = bB - b;
                    const int cnt = (int)(left < to_fan ? left : to_fan);
                    const bool valid = lane < cnt;
                    LbMinMax en = {0.0, 0.0};
                    if (valid) en = a.t1[b + lane];
                    lb_entry(en, base, s, hi, lo);
                    const uint64_t may = __ballot(valid && (hi >= U || lo <= L));
                    const int f = may ? __ffsll((unsigned long long)may) - 1 : cnt;
                    if (lane < f) { mx = hi > mx ? hi : mx; mn = lo < mn ? lo : mn; }
                    b += f;
                    if (!may) continue;
                    ++opened;                                                        // the block that holds the first touch
                    hit = tb_walk(a.close, b * LB_BLOCK, b * LB_BLOCK + LB_BLOCK - 1, base, s, U, L, mx, mn, ret, touch, walked);
                    ++b;
                }
                if (!hit && bB * LB_BLOCK <= t1)
                    hit = tb_walk(a.close, bB * LB_BLOCK, t1, base, s, U, L, mx, mn, ret, touch, walked);
            }
            if (!hit) ret = (fmk_log_host(a.close[t1]) - base) * s;                  // the last evaluated tick
        }
        int8_t label;
        if (a.side) label = ret >= a.min_ret ? 1 : 0;                                // tbm.py:139-143
        else label = ret < 0.0 ? -1 : 1;
        double ratio = 1.0;
        if (touch == t1) {                                                           // tbm.py:146-154
            mx = fmk_wave_max(mx);
            mn = fmk_wave_min(mn);
            double ur = 0.0, lr = 0.0;
            if (uv && mx > 0.0) { const double q = mx / U; ur = q > 0.0 ? q : 0.0; }
            if (lv && mn < 0.0) { const double q = mn / L; lr = q > 0.0 ? q : 0.0; }
            double rb;
            if (ret > 0.0) { rb = ur / (1 + lr); if (!uv) rb = NAN; }
            else { rb = lr / (1 + ur); if (!lv) rb = NAN; }
            ratio = 1.0 < rb ? 1.0 : rb;
        }
        if (lane == 0) { a.labels[e] = label; a.touch[e] = touch; a.ret[e] = ret; a.ratio[e] = ratio; }
    }
    if (lane == 0) {
        if (skipped) {
            atomicAdd((unsigned long long *)&a.mail->skipped, (unsigned long long)skipped);
            if (a.n_skipped) atomicAdd((unsigned long long *)a.n_skipped, (unsigned long long)skipped);
        }
        if (opened) atomicAdd((unsigned long long *)&a.mail->opened, (unsigned long long)opened);
        if (walked) atomicAdd((unsigned long long *)&a.mail->walked, (unsigned long long)walked);
    }
}

// event indices outside the tape (the call fails with FMK_E_ARG) and the two timestamps the tick rate is made from
__global__ __launch_bounds__(256) void k_lb_precheck(const int64_t *__restrict__ ev, int64_t n_events, const int64_t *__restrict__ ts,
                                                     int64_t n, fmk_mail::Label *mail)
{
    long long bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_events; i += (int64_t)gridDim.x * 256) {
        const int64_t v = ev[i];
        bad += v < 0 || v >= n;
    }
    bad = fmk_wave_sum(bad);
    if (fmk_lane() == 0 && bad) atomicAdd((unsigned long long *)&mail->bad, (unsigned long long)bad);
    if (blockIdx.x == 0 && threadIdx.x == 0 && n > 0) { mail->ts_ends[0] = ts[0]; mail->ts_ends[1] = ts[n - 1]; }
}

// level 1: (min, max) of log(close) over each block of LB_BLOCK ticks
__global__ __launch_bounds__(256) void k_lb_table1(const double *__restrict__ close, int64_t n, LbMinMax *__restrict__ t1)
{
    __shared__ double s_mn[4], s_mx[4];
    const int64_t base = (int64_t)blockIdx.x * LB_BLOCK;
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < LB_BLOCK / 256; ++k) {
        const int64_t j = base + k * 256 + threadIdx.x;
        if (j < n) {
            const double v = fmk_log_host(close[j]);
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
    }
    mn = fmk_wave_min(mn);
    mx = fmk_wave_max(mx);
    if (fmk_lane() == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        LbMinMax o;
        o.mn = fmin(fmin(s_mn[0], s_mn[1]), fmin(s_mn[2], s_mn[3]));
        o.mx = fmax(fmax(s_mx[0], s_mx[1]), fmax(s_mx[2], s_mx[3]));
        t1[blockIdx.x] = o;
    }
}

// level 2: one wave per LB_FAN level-1 entries
__global__ __launch_bounds__(256) void k_lb_table2(const LbMinMax *__restrict__ t1, int64_t nb1, LbMinMax *__restrict__ t2, int64_t nb2)
{
    const int64_t sb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sb >= nb2) return;
    const int64_t b = sb * LB_FAN + fmk_lane();
    double mn = INFINITY, mx = -INFINITY;
    if (b < nb1) { const LbMinMax e = t1[b]; mn = e.mn; mx = e.mx; }
    mn = fmk_wave_min(mn);
    mx = fmk_wave_max(mx);
    if (fmk_lane() == 0) { LbMinMax o; o.mn = mn; o.mx = mx; t2[sb] = o; }
}

extern "C" int fmk_diag_label_last(fmk_ctx *ctx, int64_t *out5)
{
    fmk_mail::Label m;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    FMK_TRY(fmk_read_back(ctx, &m, &ctx->d_mail->label, sizeof m));
    out5[0] = ctx->h_mail->label.last[0];
    out5[1] = ctx->h_mail->label.last[1];
    out5[2] = m.skipped;
    out5[3] = m.opened;
    out5[4] = m.walked;
    return FMK_OK;
}

extern "C" int fmk_triple_barrier_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_close, int64_t n,
                                      const int64_t *d_event_idx, const double *d_targets, const int8_t *d_side, int64_t n_events,
                                      double bottom_mult, double top_mult, double vertical_barrier_sec,
                                      double min_close_time_sec, double min_ret, int8_t *d_labels, int64_t *d_touch_idx,
                                      double *d_ret, double *d_max_rb_ratio, int64_t *d_n_skipped)
{
    if (!(vertical_barrier_sec > 0)) return fmk_set_error(ctx, FMK_E_ARG, "The vertical barrier must be greater than zero.");
    if (min_ret < 0) return fmk_set_error(ctx, FMK_E_ARG, "The minimum return must be non-negative.");
    if (n_events <= 0) return fmk_set_error(ctx, FMK_E_ARG, "The event_idxs array must not be empty.");
    if (n <= 0) return fmk_set_error(ctx, FMK_E_ARG, "triple_barrier: event indices outside the (empty) tape");
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    fmk_mail::Label *mail = &ctx->d_mail->label;
    FMK_HIP(ctx, hipMemsetAsync(mail, 0, sizeof *mail, ctx->stream));
    int64_t pre_blocks = fmk_ceil_div(n_events, 256);
    if (pre_blocks > 1024) pre_blocks = 1024;
    k_lb_precheck<<<(unsigned)pre_blocks, 256, 0, ctx->stream>>>(d_event_idx, n_events, d_ts, n, mail);
    FMK_LAUNCH_CHECK(ctx);
    fmk_mail::Label m;
    FMK_TRY(fmk_read_back(ctx, &m, mail, sizeof m));
    if (m.bad) return fmk_set_error(ctx, FMK_E_ARG, "triple_barrier: %lld event indices outside [0, %lld)", m.bad, (long long)n);

    // the schedule, from what the call can observe: the ticks a vertical barrier spans at the tape's mean tick rate
    const double vb_ns = vertical_barrier_sec * 1e9;
    const double span = (double)(m.ts_ends[1] - m.ts_ends[0]);
    const double window_ticks = span > 0 ? vb_ns * ((double)(n - 1) / span) : INFINITY;
    bool use_table = !(window_ticks < LB_LONG_MIN);
    const char *v = getenv("FMK_LABEL_SCHEDULE");                   // tests only: "direct" / "long"
    if (v && v[0] == 'd') use_table = false;
    if (v && v[0] == 'l') use_table = true;
    ctx->h_mail->label.last[0] = use_table;
    ctx->h_mail->label.last[1] = n_events;

    TbArgs a;
    a.ts = d_ts; a.close = d_close; a.n = n; a.ev = d_event_idx; a.tgt = d_targets; a.side = d_side; a.n_events = n_events;
    a.bottom = bottom_mult; a.top = top_mult; a.vb_ns = vb_ns; a.mc_ns = min_close_time_sec * 1e9; a.min_ret = min_ret;
    a.labels = d_labels; a.touch = d_touch_idx; a.ret = d_ret; a.ratio = d_max_rb_ratio; a.n_skipped = d_n_skipped;
    a.t1 = a.t2 = nullptr; a.mail = mail;
    int64_t grid = (int64_t)ctx->n_cu * 8;                           // persistent: 32 waves per CU take events from the counter
    if (grid > fmk_ceil_div(n_events, 4)) grid = fmk_ceil_div(n_events, 4);
    if (!use_table) {
        k_tb<false><<<(unsigned)grid, 256, 0, ctx->stream>>>(a);
        FMK_LAUNCH_CHECK(ctx);
        return FMK_OK;
    }
    const int64_t nb1 = fmk_ceil_div(n, LB_BLOCK), nb2 = fmk_ceil_div(nb1, LB_FAN);
    void *tab;
    FMK_TRY(fmk_alloc(ctx, (size_t)(nb1 + nb2) * sizeof(LbMinMax), &tab));
    LbMinMax *t1 = (LbMinMax *)tab, *t2 = t1 + nb1;
    k_lb_table1<<<(unsigned)nb1, 256, 0, ctx->stream>>>(d_close, n, t1);
    k_lb_table2<<<(unsigned)fmk_ceil_div(nb2, 4), 256, 0, ctx->stream>>>(t1, nb1, t2, nb2);
    a.t1 = t1;
    a.t2 = t2;
    k_tb<true><<<(unsigned)grid, 256, 0, ctx->stream>>>(a);
    const hipError_t le = hipGetLastError();
    FMK_TRY(fmk_free(ctx, tab));                                     // stream-ordered: the next user comes after k_tb
    FMK_HIP(ctx, le);
    return FMK_OK;
}

// ---------------------------------------------------------------------------------------
// concurrency (weights.py:31-38)
// ---------------------------------------------------------------------------------------
#define LC_TILE 4096

__global__ __launch_bounds__(256) void k_lc_mark(const int64_t *__restrict__ ev, const int64_t *__restrict__ touch, int64_t n_events,
                                                 int64_t n, int *__restrict__ diff, fmk_mail::Label *mail)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_events) return;
    const int64_t s = ev[i], t = touch[i];
    if (s < 0 || t < s || t >= n) { atomicAdd((unsigned long long *)&mail->bad, 1ull); return; }
    atomicAdd(&diff[s], 1);
    atomicAdd(&diff[t + 1], -1);                   // diff has n + 1 entries
}

__global__ __launch_bounds__(256) void k_lc_tile_sums(const int *__restrict__ diff, int64_t n, unsigned *__restrict__ tile_sum)
{
    __shared__ unsigned sw[4];
    const int64_t base = (int64_t)blockIdx.x * LC_TILE;
    unsigned s = 0;
#pragma unroll 4
    for (int r = 0; r < LC_TILE / 256; ++r) {
        const int64_t j = base + r * 256 + threadIdx.x;
        if (j < n) s += (unsigned)diff[j];
    }
    s = fmk_wave_sum(s);
    if (fmk_lane() == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

// the uint32 sum as a monoid of fmk_wgscan.h: the exclusive scan of the tile sums (one workgroup, LC_AGG_UNIT per trip) and the
// workgroup scan of k_lc_apply come from there
#define LC_AGG_UNIT 1024
namespace {
struct LcSum : FmkScalarDpp<LcSum, unsigned, int> {
    using T = unsigned;
    static __device__ __forceinline__ unsigned identity() { return 0; }
    static __device__ __forceinline__ unsigned combine(unsigned first, unsigned then) { return first + then; }
};
}  // namespace

// concurrency[j] = int16(inclusive prefix of diff), one workgroup scan per row of 256 ticks
__global__ __launch_bounds__(256) void k_lc_apply(const int *__restrict__ diff, int64_t n, const unsigned *__restrict__ tile_off,
                                                  int16_t *__restrict__ out)
{
    __shared__ unsigned ws[4];
    const int64_t base = (int64_t)blockIdx.x * LC_TILE;
    unsigned run = tile_off[blockIdx.x];
    for (int r = 0; r < LC_TILE / 256; ++r) {
        const int64_t j = base + r * 256 + threadIdx.x;
        const unsigned v = j < n ? (unsigned)diff[j] : 0;
        unsigned tot;
        const unsigned ex = fmk_wg_exclusive<LcSum, 4>(v, ws, &tot);
        if (j < n) out[j] = (int16_t)(uint16_t)(run + LcSum::combine(ex, v));
        run += tot;
    }
}

static int lb_check_bad(fmk_ctx *ctx, const char *what, int64_t n)
{
    fmk_mail::Label m;
    FMK_TRY(fmk_read_back(ctx, &m, &ctx->d_mail->label, sizeof m));
    if (m.bad)
        return fmk_set_error(ctx, FMK_E_ARG, "%s: %lld events outside 0 <= event_idx <= touch_idx < %lld", what, m.bad, (long long)n);
    return FMK_OK;
}

extern "C" int fmk_label_concurrency_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, int64_t n_events,
                                         int64_t n, int16_t *d_concurrency)
{
    if (n_events < 0 || n < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    if (n == 0) {
        if (n_events) return fmk_set_error(ctx, FMK_E_ARG, "label_concurrency: events on an empty tape");
        return FMK_OK;
    }
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n_events == 0) {                          // weights.py: an empty event list is legal -- a zero column
        FMK_HIP(ctx, hipMemsetAsync(d_concurrency, 0, (size_t)n * sizeof(int16_t), ctx->stream));
        return FMK_OK;
    }
    fmk_mail::Label *mail = &ctx->d_mail->label;
    FMK_HIP(ctx, hipMemsetAsync(&mail->bad, 0, sizeof mail->bad, ctx->stream));
    const int64_t tiles = fmk_ceil_div(n, LC_TILE);
    void *blk;
    FMK_TRY(fmk_alloc(ctx, (size_t)(n + 1) * sizeof(int) + (size_t)tiles * sizeof(unsigned) + 16, &blk));
    int *diff = (int *)blk;
    unsigned *tile = (unsigned *)(diff + ((n + 1 + 3) & ~(int64_t)3));
    hipError_t le = hipMemsetAsync(diff, 0, (size_t)(n + 1) * sizeof(int), ctx->stream);
    if (le == hipSuccess) {
        k_lc_mark<<<(unsigned)fmk_ceil_div(n_events, 256), 256, 0, ctx->stream>>>(d_event_idx, d_touch_idx, n_events, n, diff, mail);
        k_lc_tile_sums<<<(unsigned)tiles, 256, 0, ctx->stream>>>(diff, n, tile);
        k_fmk_agg_scan<LcSum, LC_AGG_UNIT><<<1, LC_AGG_UNIT, 0, ctx->stream>>>(tile, tiles, nullptr);
        k_lc_apply<<<(unsigned)tiles, 256, 0, ctx->stream>>>(diff, n, tile, d_concurrency);
        le = hipGetLastError();
    }
    FMK_TRY(fmk_free(ctx, blk));
    FMK_HIP(ctx, le);
    return lb_check_bad(ctx, "label_concurrency", n);
}

// ---------------------------------------------------------------------------------------
// average uniqueness + return attribution (weights.py:41-47, 76-94)
// ---------------------------------------------------------------------------------------
// the attribution term of tick j: log(close[j] / close[j-1]) / c, 0 where the reference adds nothing
__device__ __forceinline__ double lw_term(const double *__restrict__ close, int16_t c, int64_t j)
{
    if (c <= 0 || j == 0) return 0.0;
    const double pm = close[j - 1];
    if (pm == 0.0) return 0.0;
    const double lr = fmk_log_ratio(close[j], pm);
    if (lr != lr) return 0.0;
    return lr / (double)c;
}

// per block of LW_BLOCK ticks: sum of 1 / c and of the attribution terms (fixed tree order)
template <bool ATTR>
__global__ __launch_bounds__(256) void k_lw_blocks(const double *__restrict__ close, const int16_t *__restrict__ conc, int64_t n,
                                                   double *__restrict__ sum_u, double *__restrict__ sum_a)
{
    __shared__ double s_u[4], s_a[4];
    const int64_t base = (int64_t)blockIdx.x * LW_BLOCK;
    double u = 0.0, at = 0.0;
#pragma unroll
    for (int k = 0; k < LW_BLOCK / 256; ++k) {
        const int64_t j = base + k * 256 + threadIdx.x;
        if (j < n) {
            const int16_t c = conc[j];
            u += 1.0 / (double)c;
            if (ATTR) at += lw_term(close, c, j);
        }
    }
    u = fmk_wave_sum(u);
    if (ATTR) at = fmk_wave_sum(at);
    if (fmk_lane() == 0) { s_u[threadIdx.x >> 6] = u; s_a[threadIdx.x >> 6] = at; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sum_u[blockIdx.x] = (s_u[0] + s_u[1]) + (s_u[2] + s_u[3]);
        if (ATTR) sum_a[blockIdx.x] = (s_a[0] + s_a[1]) + (s_a[2] + s_a[3]);
    }
}

// one wave per event: the ticks in front of the first whole block, the whole blocks' sums, the ticks behind the last one
template <bool ATTR>
__global__ __launch_bounds__(256) void k_lw_events(const double *__restrict__ close, const int16_t *__restrict__ conc, int64_t n,
                                                   const int64_t *__restrict__ ev, const int64_t *__restrict__ touch,
                                                   int64_t n_events, const double *__restrict__ sum_u,
                                                   const double *__restrict__ sum_a, double *__restrict__ avg_u,
                                                   double *__restrict__ attr, fmk_mail::Label *mail)
{
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_events) return;
    const int lane = fmk_lane();
    const int64_t s = ev[e], t = touch[e];
    if (s < 0 || t < s || t >= n) {
        if (lane == 0) {
            atomicAdd((unsigned long long *)&mail->bad, 1ull);
            if (avg_u) avg_u[e] = NAN;
            if (ATTR) attr[e] = NAN;
        }
        return;
    }
    const int64_t b0 = (s + LW_BLOCK - 1) / LW_BLOCK, b1 = (t + 1) / LW_BLOCK;      // whole blocks [b0, b1)
    double u = 0.0, at = 0.0;
    const int64_t head_end = b0 < b1 ? b0 * LW_BLOCK - 1 : t;
    for (int64_t j = s + lane; j <= head_end; j += 64) {
        const int16_t c = conc[j];
        u += 1.0 / (double)c;
        if (ATTR) at += lw_term(close, c, j);
    }
    if (b0 < b1) {
        for (int64_t b = b0 + lane; b < b1; b += 64) {
            u += sum_u[b];
            if (ATTR) at += sum_a[b];
        }
        for (int64_t j = b1 * LW_BLOCK + lane; j <= t; j += 64) {
            const int16_t c = conc[j];
            u += 1.0 / (double)c;
            if (ATTR) at += lw_term(close, c, j);
        }
    }
    u = fmk_wave_sum(u);
    if (ATTR) at = fmk_wave_sum(at);
    if (lane == 0) {
        if (avg_u) avg_u[e] = u / (double)(t - s + 1);
        if (ATTR) attr[e] = fabs(at);
    }
}

extern "C" int fmk_label_weights_dev(fmk_ctx *ctx, const double *d_close, const int16_t *d_concurrency, int64_t n,
                                     const int64_t *d_event_idx, const int64_t *d_touch_idx, int64_t n_events,
                                     double *d_avg_uniqueness, double *d_return_attribution)
{
    if (n_events < 0 || n < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    if (d_return_attribution && !d_close) return fmk_set_error(ctx, FMK_E_ARG, "label_weights: return attribution needs the close column");
    if (n_events == 0 || (!d_avg_uniqueness && !d_return_attribution)) return FMK_OK;
    if (n == 0) return fmk_set_error(ctx, FMK_E_ARG, "label_weights: events on an empty tape");
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    fmk_mail::Label *mail = &ctx->d_mail->label;
    FMK_HIP(ctx, hipMemsetAsync(&mail->bad, 0, sizeof mail->bad, ctx->stream));
    const int64_t nb = fmk_ceil_div(n, LW_BLOCK);
    void *blk;
    FMK_TRY(fmk_alloc(ctx, (size_t)nb * 2 * sizeof(double), &blk));
    double *su = (double *)blk, *sa = su + nb;
    const unsigned eg = (unsigned)fmk_ceil_div(n_events, 4);
    if (d_return_attribution) {
        k_lw_blocks<true><<<(unsigned)nb, 256, 0, ctx->stream>>>(d_close, d_concurrency, n, su, sa);
        k_lw_events<true><<<eg, 256, 0, ctx->stream>>>(d_close, d_concurrency, n, d_event_idx, d_touch_idx, n_events, su, sa,
                                                       d_avg_uniqueness, d_return_attribution, mail);
    } else {
        k_lw_blocks<false><<<(unsigned)nb, 256, 0, ctx->stream>>>(d_close, d_concurrency, n, su, sa);
        k_lw_events<false><<<eg, 256, 0, ctx->stream>>>(d_close, d_concurrency, n, d_event_idx, d_touch_idx, n_events, su, sa,
                                                        d_avg_uniqueness, d_return_attribution, mail);
    }
    const hipError_t le = hipGetLastError();
    FMK_TRY(fmk_free(ctx, blk));
    FMK_HIP(ctx, le);
    return lb_check_bad(ctx, "label_weights", n);
}
