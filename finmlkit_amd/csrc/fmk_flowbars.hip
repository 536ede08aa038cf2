// fmk_flowbars.hip -- imbalance and run bars with a fixed threshold (AFML 2.3.2; the reference has stubs only, logic.py:224-261).
//
// The loops that define them (DESIGN.md section 6 "Imbalance and run bars"; fb_step in fmk_flowbars_search.h is their one step):
//   imbalance   theta += side * size;                    close at the first |theta| >= thr, then theta = 0
//   run         side > 0: up += size, side < 0: dn += size;  close at the first up >= thr or dn >= thr, then up = dn = 0
// tick 0 is counted but cannot close, the result starts with index 0.  After a close only its position matters, so both are reset
// chains: nxt(j) = the close of the bar that starts behind tick j, and the answer is root, nxt(root), nxt(nxt(root)), ...  The
// one-pass CUSUM scheme does not apply: two walks that start from different states stay a constant apart until one closes.
//
// Two rungs.
//   tables (rung 0)   for 0 < thr < inf, n < 2^31 - 4096, finite sizes >= 0, and a tape that CERTIFIES: all increments are multiples
//       of one power of two q and sum |x| + thr stays below 2^53 q (fb_certificate), so every sum is exact in float64 in any order
//       and a prefix difference is the loop's theta.  No margins, no replay.
//         k_fb_prefix   one pass over the columns: block-local inclusive prefixes of the increments (U; run: U and V), per block
//                       (total, max, min, sum |x|), the tape's quantum, the bad-amount flag
//         k_fb_scan     block totals -> block bases; (max, min) per block become absolute; sum |x| of the tape
//         [host wait: the certificate; T = thr rounded up to q]
//         k_fb_links    nxt(j) for every tick: the first-exit search of fmk_flowbars_search.h in the tick's own block (LDS pyramid),
//                       then over block summaries 64 at a time, then in the block that fires.  k_fb_root: the first close.
//         [host wait: the longest link -> table span S = 2^ls]
//         k_fb_level0, the tree of fmk_voltree.h (one host wait: the count), k_fb_emit
//   serial (rung 1)   one lane walks the loops.  Everything else, and everything with FMK_FLOWBARS_SERIAL set (tests).
// Nothing is kept between calls: the work buffers come from the context's pool and go back to it, the result is the caller's.
#include <limits.h>
#include <math.h>
#include <stdlib.h>

#include "fmk_common.h"
#include "fmk_voltree.h"
#include "fmk_flowbars_search.h"

#define FB_DEND 0x7FFFFFFF              // destination block of a tick whose bar never closes (or closes in its own block)
#define FB_TOO_LONG 0x7FFFFFFFu         // "longest link" of a tick that ran out of look-ahead

typedef fmk_mail::Fb::Tape FbTape;

static struct FbDiag { int64_t rung, code, longest, ls; } g_fb_diag = {-1, 0, 0, 0};

extern "C" int fmk_diag_flowbars_last(int64_t *rung, int64_t *code, int64_t *longest, int64_t *ls)
{
    *rung = g_fb_diag.rung;
    *code = g_fb_diag.code;
    *longest = g_fb_diag.longest;
    *ls = g_fb_diag.ls;
    return FMK_OK;
}

// side and size of tick i (i < n)
template <int KIND, bool AF64>
__device__ __forceinline__ void fb_tick(const double *__restrict__ price, const void *__restrict__ amount,
                                        const int8_t *__restrict__ side, int64_t i, int &b, double &q, bool &bad)
{
    b = side[i];
    q = 1.0;
    if constexpr (KIND >= 1) {
        const double a = fmk_amt<AF64>(amount, i);
        bad |= !(a >= 0.0 && a < INFINITY);
        q = a;
        if constexpr (KIND == 2) {
            const double p = price[i];
            bad |= !(p >= 0.0 && p < INFINITY);
            q = p * a;                                              // one rounded product (-ffp-contract=off)
            bad |= !(q < INFINITY);
        }
    }
}

// ---- pass 1: one wave per 512-tick block, lane l owns ticks 8 l .. 8 l + 7
template <bool RUN, int KIND, bool AF64>
__global__ __launch_bounds__(256) void k_fb_prefix(const double *__restrict__ price, const void *__restrict__ amount,
                                                   const int8_t *__restrict__ side, int64_t n, int64_t nblk,
                                                   double *__restrict__ LU, double *__restrict__ LV, double *__restrict__ tU,
                                                   double *__restrict__ tV, double *__restrict__ bmx, double *__restrict__ bmn,
                                                   double *__restrict__ bsa, FbTape *__restrict__ tape)
{
    const int lane = fmk_lane(), w = threadIdx.x >> 6;
    const int64_t blk = (int64_t)blockIdx.x * 4 + w;
    if (blk >= nblk) return;
    const int64_t j0 = blk * FB_BLOCK + (int64_t)lane * 8;
    double u[8], v[8], sa = 0.0;
    bool bad = false;
    int qe = INT_MAX;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double xu = 0.0, xv = 0.0;
        if (j0 + k < n) {
            int b;
            double q;
            fb_tick<KIND, AF64>(price, amount, side, j0 + k, b, q, bad);
            if constexpr (RUN) { xu = b > 0 ? q : 0.0; xv = b < 0 ? -q : 0.0; }
            else xu = (double)b * q;
            const int e1 = fb_low_bit_exp(xu), e2 = RUN ? fb_low_bit_exp(xv) : INT_MAX;
            qe = e1 < qe ? e1 : qe;
            qe = e2 < qe ? e2 : qe;
            sa += fabs(xu) + fabs(xv);
        }
        u[k] = k ? u[k - 1] + xu : xu;                              // inclusive inside the lane
        v[k] = k ? v[k - 1] + xv : xv;
    }
    const double iu = fmk_wave_iscan(u[7]), iv = RUN ? fmk_wave_iscan(v[7]) : 0.0;
    double eu = __shfl_up(iu, 1, 64), ev = __shfl_up(iv, 1, 64);   // the lanes before this one
    if (lane == 0) eu = ev = 0.0;
    double mx = -INFINITY, mn = INFINITY;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        u[k] += eu;                                                 // ticks past the end repeat the last prefix: neutral for max / min
        v[k] = RUN ? v[k] + ev : u[k];
        mx = fmax(mx, u[k]);
        mn = fmin(mn, v[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (j0 + k < n) {
            LU[j0 + k] = u[k];
            if constexpr (RUN) LV[j0 + k] = v[k];
        }
    mx = fmk_wave_max(mx);
    mn = fmk_wave_min(mn);
    sa = fmk_wave_sum(sa);
    qe = (int)fmk_wave_min((int64_t)qe);
    const double totu = __shfl(iu, 63, 64), totv = __shfl(iv, 63, 64);
    if (__ballot(bad) != 0 && lane == 0) vol_flag(&tape->status, VOL_ST_BAD);
    if (lane == 0) {
        tU[blk] = totu;
        if constexpr (RUN) tV[blk] = totv;
        bmx[blk] = mx;
        bmn[blk] = mn;
        bsa[blk] = sa;                                              // summed by k_fb_scan, not by a float64 atomic per wave on one address
        if (qe < __atomic_load_n(&tape->qexp, __ATOMIC_RELAXED)) atomicMin(&tape->qexp, qe);
    }
}

// ---- pass 2: one workgroup.  Block totals -> exclusive bases (in place); the blocks' local (max, min) become absolute; the
// blocks' sums of |x| add up to the tape's.
template <bool RUN>
__global__ __launch_bounds__(1024) void k_fb_scan(int64_t nblk, double *__restrict__ tU, double *__restrict__ tV,
                                                  double *__restrict__ bmx, double *__restrict__ bmn,
                                                  const double *__restrict__ bsa, FbTape *__restrict__ tape)
{
    __shared__ double s_u[16], s_v[16], s_a[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t per = (nblk + 1023) / 1024;
    const int64_t b0 = (int64_t)tid * per < nblk ? (int64_t)tid * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
    double su = 0.0, sv = 0.0;
    double sa = 0.0;
    for (int64_t b = b0; b < b1; ++b) { su += tU[b]; sa += bsa[b]; if constexpr (RUN) sv += tV[b]; }
    const double iu = fmk_wave_iscan(su), iv = fmk_wave_iscan(sv);
    sa = fmk_wave_sum(sa);
    if (lane == 63) { s_u[w] = iu; s_v[w] = iv; s_a[w] = sa; }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += s_a[q];
        tape->sum_abs = t;
    }
    double ru = __shfl_up(iu, 1, 64), rv = __shfl_up(iv, 1, 64);
    if (lane == 0) ru = rv = 0.0;
    for (int q = 0; q < w; ++q) { ru += s_u[q]; rv += s_v[q]; }
    for (int64_t b = b0; b < b1; ++b) {
        const double t = tU[b];
        tU[b] = ru;
        bmx[b] += ru;
        if constexpr (RUN) {
            const double t2 = tV[b];
            tV[b] = rv;
            bmn[b] += rv;
            rv += t2;
        } else bmn[b] += ru;
        ru += t;
    }
}

// ---- pass 3: the links
struct FbTile {
    double U[FB_BLOCK], V[FB_BLOCK];                               // absolute prefixes of the staged block (imbalance: V unused)
    double mx8[FB_BLOCK / 8], mn8[FB_BLOCK / 8], mx64[FB_BLOCK / 64], mn64[FB_BLOCK / 64];
    double smx[64], smn[64];                                       // summaries of 64 following blocks
};

// the wave stages block blk (absolute prefixes, short blocks padded with their last tick) and its pyramid -> valid ticks
template <bool RUN>
__device__ __forceinline__ int fb_stage(FbTile &t, const double *__restrict__ LU, const double *__restrict__ LV,
                                        const double *__restrict__ baseU, const double *__restrict__ baseV, int64_t blk, int64_t n)
{
    const int lane = fmk_lane();
    const int64_t ds = blk * FB_BLOCK;
    const int nv = (int)(n - ds < FB_BLOCK ? n - ds : FB_BLOCK);
    const double bu = baseU[blk], bv = RUN ? baseV[blk] : 0.0;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < FB_BLOCK / 64; ++q) {
        const int i = 64 * q + lane, src = i < nv ? i : nv - 1;
        t.U[i] = bu + LU[ds + src];
        if constexpr (RUN) t.V[i] = bv + LV[ds + src];
    }
    __builtin_amdgcn_wave_barrier();
    const double *V = RUN ? t.V : t.U;
    double a = t.U[8 * lane], b = V[8 * lane];
#pragma unroll
    for (int i = 1; i < 8; ++i) { a = fmax(a, t.U[8 * lane + i]); b = fmin(b, V[8 * lane + i]); }
    t.mx8[lane] = a;
    t.mn8[lane] = b;
    __builtin_amdgcn_wave_barrier();
    if (lane < FB_BLOCK / 64) {
        double c = t.mx8[8 * lane], d = t.mn8[8 * lane];
#pragma unroll
        for (int i = 1; i < 8; ++i) { c = fmax(c, t.mx8[8 * lane + i]); d = fmin(d, t.mn8[8 * lane + i]); }
        t.mx64[lane] = c;
        t.mn64[lane] = d;
    }
    __builtin_amdgcn_wave_barrier();
    return nv;
}

template <bool RUN>
__global__ __launch_bounds__(256) void k_fb_links(const double *__restrict__ LU, const double *__restrict__ LV,
                                                  const double *__restrict__ baseU, const double *__restrict__ baseV,
                                                  const double *__restrict__ gmx, const double *__restrict__ gmn, int64_t n,
                                                  int64_t nblk, double T, uint32_t *__restrict__ nxt, FbTape *__restrict__ tape)
{
    __shared__ FbTile s_tile[4];
    const int lane = fmk_lane(), w = threadIdx.x >> 6;
    FbTile &t = s_tile[w];
    const double *tV = RUN ? t.V : t.U;
    const int64_t blk = (int64_t)blockIdx.x * 4 + w;
    if (blk >= nblk) return;                                        // waves are independent: wave barriers only
    const int64_t bs = blk * FB_BLOCK;
    const int nv = fb_stage<RUN>(t, LU, LV, baseU, baseV, blk, n);
    double hi[8], lo[8];
    int dblk[8];
    uint32_t res[8];
    bool odd = false;                                               // the pyramid or a summary contradicted its ticks
    // ---- the tick's own block
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int jl = lane * 8 + k;
        res[k] = VOL_END;
        dblk[k] = FB_DEND;
        hi[k] = lo[k] = 0.0;
        if (jl < nv) {
            hi[k] = t.U[jl] + T;
            lo[k] = tV[jl] - T;
            const int r = fb_first_exit(t.U, tV, t.mx8, t.mn8, t.mx64, t.mn64, jl + 1, hi[k], lo[k]);
            if (r < nv) res[k] = (uint32_t)(bs + r);
            else dblk[k] = -1;                                      // pending
        }
    }
    // ---- the block it closes in: summaries of the following blocks, 64 per load
    bool too_long = false;
    for (int r = 0;; ++r) {
        const int64_t b0 = blk + 1 + 64 * (int64_t)r;
        const int nvb = (int)(nblk - b0 < 64 ? nblk - b0 : 64);
        if (nvb <= 0) break;
        __builtin_amdgcn_wave_barrier();
        const double mymx = lane < nvb ? gmx[b0 + lane] : -INFINITY, mymn = lane < nvb ? gmn[b0 + lane] : INFINITY;
        t.smx[lane] = mymx;
        t.smn[lane] = mymn;
        __builtin_amdgcn_wave_barrier();
        const double rmx = fmk_wave_max(mymx), rmn = fmk_wave_min(mymn);
        bool pending = false;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (dblk[k] != -1) continue;
            if (fb_out(rmx, rmn, hi[k], lo[k])) {
                const int i = fb_first_block(t.smx, t.smn, nvb, hi[k], lo[k]);
                if (i < nvb) dblk[k] = 1 + 64 * r + i;
                else { dblk[k] = FB_DEND; odd = true; }
            } else pending = true;
        }
        if (__ballot(pending) == 0) break;
        if (r + 1 == FB_MAX_ROUNDS) { too_long = b0 + 64 < nblk; break; }
    }
    int64_t wmax = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (dblk[k] == -1) {                                        // no close before the tape (or the look-ahead) ends
            dblk[k] = FB_DEND;
            if (too_long) wmax = FB_TOO_LONG;
        }
    // ---- inside the destination blocks, in ascending order, only those some tick needs
    int cur = 0;
    for (;;) {
        int mine = FB_DEND;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (dblk[k] > cur && dblk[k] < mine) mine = dblk[k];
        cur = (int)fmk_wave_min((int64_t)mine);
        if (cur == FB_DEND) break;
        const int64_t ds = (blk + cur) * FB_BLOCK;
        const int nvd = fb_stage<RUN>(t, LU, LV, baseU, baseV, blk + cur, n);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (dblk[k] != cur) continue;
            const int r = fb_first_exit(t.U, tV, t.mx8, t.mn8, t.mx64, t.mn64, 0, hi[k], lo[k]);
            if (r < nvd) res[k] = (uint32_t)(ds + r);
            else odd = true;
        }
    }
    const int64_t j0 = bs + (int64_t)lane * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (res[k] != VOL_END && (int64_t)res[k] - (j0 + k) > wmax) wmax = (int64_t)res[k] - (j0 + k);
    if (j0 + 7 < n) {
        uint4 *o = (uint4 *)(nxt + j0);
        o[0] = make_uint4(res[0], res[1], res[2], res[3]);
        o[1] = make_uint4(res[4], res[5], res[6], res[7]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (j0 + k < n) nxt[j0 + k] = res[k];
    }
    wmax = fmk_wave_max(wmax);
    if (lane == 0 && (unsigned)wmax > __atomic_load_n(&tape->maxlen, __ATOMIC_RELAXED)) atomicMax(&tape->maxlen, (unsigned)wmax);
    if (__ballot(odd) != 0 && lane == 0) vol_flag(&tape->status, VOL_ST_INEXACT);
}

// the first close: tick 0 is counted but cannot close -> the first m >= 1 that exits from a prefix of zero
template <bool RUN>
__global__ __launch_bounds__(64) void k_fb_root(const double *__restrict__ LU, const double *__restrict__ LV,
                                                const double *__restrict__ baseU, const double *__restrict__ baseV,
                                                const double *__restrict__ gmx, const double *__restrict__ gmn, int64_t n,
                                                int64_t nblk, double T, FbTape *__restrict__ tape)
{
    __shared__ FbTile t;
    const double *tV = RUN ? t.V : t.U;
    const int lane = fmk_lane();
    const double hi = T, lo = -T;
    int64_t m = -1;                                                 // -1 none, -2 a summary contradicted its ticks
    const int nv = fb_stage<RUN>(t, LU, LV, baseU, baseV, 0, n);
    const int r = fb_first_exit(t.U, tV, t.mx8, t.mn8, t.mx64, t.mn64, 1, hi, lo);
    if (r < nv) m = r;
    else
        for (int64_t b0 = 1; b0 < nblk && m == -1; b0 += 64) {
            const int64_t b = b0 + lane;
            const bool hit = b < nblk && fb_out(gmx[b < nblk ? b : 0], gmn[b < nblk ? b : 0], hi, lo);
            const uint64_t mk = __ballot(hit);
            if (mk == 0) continue;
            const int64_t bstar = b0 + __ffsll((unsigned long long)mk) - 1;
            const int nvd = fb_stage<RUN>(t, LU, LV, baseU, baseV, bstar, n);
            const int r2 = fb_first_exit(t.U, tV, t.mx8, t.mn8, t.mx64, t.mn64, 0, hi, lo);
            m = r2 < nvd ? bstar * FB_BLOCK + r2 : -2;
        }
    if (lane != 0) return;
    tape->root = m >= 0 ? (uint32_t)m : VOL_END;
    if (m >= 0) atomicMax(&tape->maxlen, (unsigned)m);              // the tables must span the first bar too
    if (m == -2) vol_flag(&tape->status, VOL_ST_INEXACT);
}

// ---- the tree's level 0 from the links, and the emit pass (the shapes of k_vg_level0 / k_vol_emit without fragile lists)
__global__ __launch_bounds__(256) void k_fb_level0(const uint32_t *__restrict__ nxt, int64_t n, int ls, int64_t total,
                                                   uint32_t *__restrict__ E0, uint32_t *__restrict__ C0)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    if (j >= n) { E0[j] = VOL_END; C0[j] = 0; return; }
    const uint64_t bend = (uint64_t)((j >> ls) + 1) << ls;
    uint32_t e = nxt[j], c = 1;
    while (e != VOL_END && (uint64_t)e < bend && (int64_t)e < n) { e = nxt[e]; ++c; }
    E0[j] = e;
    C0[j] = c;
}

__global__ __launch_bounds__(256) void k_fb_emit(int ls, const uint32_t *__restrict__ ent0, const int64_t *__restrict__ off0,
                                                 int64_t nblk0, const uint32_t *__restrict__ nxt, int64_t n,
                                                 int64_t *__restrict__ out, int64_t cap)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0 && cap > 0) out[0] = 0;
    if (b >= nblk0) return;
    uint32_t j = ent0[b];
    int64_t o = off0[b];
    const uint64_t bend = (uint64_t)(b + 1) << ls;
    while (j != VOL_END && (uint64_t)j < bend && (int64_t)j < n) {
        if (o >= 0 && o < cap) out[o] = (int64_t)j;
        ++o;
        j = nxt[j];
    }
}

// ---- the serial rung: the loops themselves.  The lanes fetch 64 ticks (the next 64 are in flight meanwhile), lane 0 walks them.
template <bool RUN, int KIND, bool AF64>
__global__ __launch_bounds__(64) void k_fb_serial(const double *__restrict__ price, const void *__restrict__ amount,
                                                  const int8_t *__restrict__ side, int64_t n, double thr,
                                                  int64_t *__restrict__ out, int64_t cap, int64_t *__restrict__ count)
{
    __shared__ double s_q[64];
    __shared__ int s_b[64];
    const int lane = fmk_lane();
    int64_t m = 1;
    if (lane == 0 && cap > 0) out[0] = 0;
    auto load = [&](int64_t i, int &b, double &q) {
        b = 0;
        q = 0.0;
        bool bad = false;
        if (i < n) fb_tick<KIND, AF64>(price, amount, side, i, b, q, bad);
    };
    FbState st = {0.0, 0.0, 0.0};
    int cb, nb;
    double cq, nq;
    load(lane, cb, cq);
    for (int64_t base = 0; base < n; base += 64) {
        load(base + 64 + lane, nb, nq);
        s_q[lane] = cq;
        s_b[lane] = cb;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            const int lim = (int)(n - base < 64 ? n - base : 64);
            for (int q = 0; q < lim; ++q)
                if (fb_step(st, RUN, s_b[q], s_q[q], thr, base + q > 0)) {
                    if (m < cap) out[m] = base + q;
                    ++m;
                }
        }
        __builtin_amdgcn_wave_barrier();
        cb = nb;
        cq = nq;
    }
    if (lane == 0) *count = m;
}

// ---- host side
struct FbBuf {                                                      // a block of the context's pool for the length of a scope
    fmk_ctx *ctx;
    void *p;
    explicit FbBuf(fmk_ctx *c) : ctx(c), p(nullptr) {}
    FbBuf(const FbBuf &) = delete;
    FbBuf &operator=(const FbBuf &) = delete;
    ~FbBuf() { if (p) (void)fmk_free(ctx, p); }
    int get(size_t bytes) { return fmk_alloc(ctx, bytes, &p); }
    void *release() { void *q = p; p = nullptr; return q; }
};

static size_t fb_round(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// -> FMK_OK (answered), 1 / 2 / 4 (declined: fmk_diag_flowbars_last), < 0 an error
template <bool RUN, int KIND, bool AF64>
static int fb_tables(fmk_ctx *ctx, const double *d_price, const void *d_amount, const int8_t *d_side, int64_t n, double thr,
                     int64_t **d_out, int64_t *n_idx)
{
    const int64_t nblk = fmk_ceil_div(n, FB_BLOCK);
    FbTape *d_tape = &ctx->d_mail->fb.tape, *h_tape = &ctx->h_mail->fb.tape, tape;
    memset(h_tape, 0, sizeof *h_tape);                              // the pinned copy holds the start values until the copy has run
    h_tape->qexp = INT_MAX;
    FMK_HIP(ctx, hipMemcpyAsync(d_tape, h_tape, sizeof *h_tape, hipMemcpyHostToDevice, ctx->stream));
    // prefixes (run: two), the per-block arrays, the links
    const size_t col = fb_round((size_t)n * 8), bcol = fb_round((size_t)nblk * 8);
    FbBuf pre(ctx), blocks(ctx), links(ctx);
    FMK_TRY(pre.get(col * (RUN ? 2 : 1)));
    FMK_TRY(blocks.get(bcol * 5));
    double *LU = (double *)pre.p, *LV = RUN ? (double *)((char *)pre.p + col) : LU;
    double *tU = (double *)blocks.p, *tV = (double *)((char *)blocks.p + bcol), *bmx = (double *)((char *)blocks.p + 2 * bcol),
           *bmn = (double *)((char *)blocks.p + 3 * bcol), *bsa = (double *)((char *)blocks.p + 4 * bcol);
    const unsigned wgrid = (unsigned)fmk_ceil_div(nblk, 4);
    k_fb_prefix<RUN, KIND, AF64><<<wgrid, 256, 0, ctx->stream>>>(d_price, d_amount, d_side, n, nblk, LU, LV, tU, tV, bmx, bmn, bsa, d_tape);
    k_fb_scan<RUN><<<1, 1024, 0, ctx->stream>>>(nblk, tU, tV, bmx, bmn, bsa, d_tape);
    FMK_LAUNCH_CHECK(ctx);
    FMK_TRY(fmk_read_back(ctx, &tape, d_tape, sizeof tape));
    if (tape.status & VOL_ST_BAD) return 2;
    double T;
    if (!fb_certificate(tape.sum_abs, tape.qexp, thr, &T)) return 4;
    const double *baseU = tU, *baseV = RUN ? tV : tU;
    FMK_TRY(links.get((size_t)n * 4));
    uint32_t *nxt = (uint32_t *)links.p;
    k_fb_links<RUN><<<wgrid, 256, 0, ctx->stream>>>(LU, LV, baseU, baseV, bmx, bmn, n, nblk, T, nxt, d_tape);
    k_fb_root<RUN><<<1, 64, 0, ctx->stream>>>(LU, LV, baseU, baseV, bmx, bmn, n, nblk, T, d_tape);
    FMK_LAUNCH_CHECK(ctx);
    FMK_TRY(fmk_read_back(ctx, &tape, d_tape, sizeof tape));
    if (tape.status & VOL_ST_INEXACT) return 4;
    const uint32_t root = tape.root;
    const int64_t longest = tape.maxlen;
    g_fb_diag.longest = longest;
    FbBuf out(ctx);
    if (root == VOL_END) {                                          // no close at all: [0]
        FMK_TRY(out.get(8));
        FMK_HIP(ctx, hipMemsetAsync(out.p, 0, 8, ctx->stream));
        *n_idx = 1;
        *d_out = (int64_t *)out.release();
        return FMK_OK;
    }
    int ls = 12;
    while (ls <= FB_MAX_LS && ((int64_t)1 << ls) < longest) ++ls;
    if (ls > FB_MAX_LS) return 1;
    g_fb_diag.ls = ls;
    const int64_t S = (int64_t)1 << ls, nblk0 = fmk_ceil_div(n, S);
    VolTree t = vol_tree_plan(nblk0, S, S, VOL_RADIX);
    FbBuf tree(ctx);
    FMK_TRY(tree.get(vol_tree_bytes(t) + 256));
    vol_tree_bind(t, tree.p);
    int *d_status = &d_tape->tree_status;                           // cleared with the tape
    k_fb_level0<<<(unsigned)fmk_ceil_div(nblk0 * S, 256), 256, 0, ctx->stream>>>(nxt, n, ls, nblk0 * S, t.E[0], t.C[0]);
    FMK_LAUNCH_CHECK(ctx);
    FMK_TRY(vol_tree_up(ctx, t, d_status));
    int64_t closes = 0;
    int status = 0;
    const int rc = vol_tree_closes(ctx, t, root, &closes, d_status, &status);
    if (rc < 0) return rc;
    if (rc == 1 || (status & VOL_ST_OVERFLOW)) return 1;            // cannot happen with S >= the longest link; the serial rung answers
    const int64_t count = closes + 1;
    FMK_TRY(out.get((size_t)count * 8));
    FMK_TRY(vol_tree_down(ctx, t, root));
    k_fb_emit<<<(unsigned)fmk_ceil_div(nblk0, 256), 256, 0, ctx->stream>>>(ls, t.ent[0], t.off[0], nblk0, nxt, n, (int64_t *)out.p, count);
    FMK_LAUNCH_CHECK(ctx);
    *n_idx = count;
    *d_out = (int64_t *)out.release();
    return FMK_OK;
}

template <bool RUN, int KIND, bool AF64>
static int fb_serial(fmk_ctx *ctx, const double *d_price, const void *d_amount, const int8_t *d_side, int64_t n, double thr,
                     int64_t **d_out, int64_t *n_idx)
{
    FbBuf all(ctx), out(ctx);                                       // at most one close per tick; the closes then move to their own buffer
    FMK_TRY(all.get((size_t)n * 8));
    int64_t *d_count = &ctx->d_mail->fb.serial_count, count = 0;
    k_fb_serial<RUN, KIND, AF64><<<1, 64, 0, ctx->stream>>>(d_price, d_amount, d_side, n, thr, (int64_t *)all.p, n, d_count);
    FMK_LAUNCH_CHECK(ctx);
    FMK_TRY(fmk_read_back(ctx, &count, d_count, 8));
    if (count < 1 || count > n) return fmk_set_error(ctx, FMK_E_HIP, "flow bar indexer: the serial walk counted %lld closes", (long long)count);
    FMK_TRY(out.get((size_t)count * 8));
    FMK_HIP(ctx, hipMemcpyAsync(out.p, all.p, (size_t)count * 8, hipMemcpyDeviceToDevice, ctx->stream));
    *n_idx = count;
    *d_out = (int64_t *)out.release();
    return FMK_OK;
}

template <bool RUN, int KIND, bool AF64>
static int fb_run(fmk_ctx *ctx, const double *d_price, const void *d_amount, const int8_t *d_side, int64_t n, double thr,
                  int64_t **d_out, int64_t *n_idx)
{
    g_fb_diag = FbDiag{-1, 0, 0, 0};
    if (!getenv("FMK_FLOWBARS_SERIAL") && n < ((int64_t)1 << 31) - 4096) {
        int rc = 2;
        if (thr > 0.0 && thr < INFINITY) rc = fb_tables<RUN, KIND, AF64>(ctx, d_price, d_amount, d_side, n, thr, d_out, n_idx);
        if (rc < 0) return rc;
        if (rc == FMK_OK) { g_fb_diag.rung = 0; return FMK_OK; }
        g_fb_diag.code = rc;
    }
    FMK_TRY((fb_serial<RUN, KIND, AF64>(ctx, d_price, d_amount, d_side, n, thr, d_out, n_idx)));
    g_fb_diag.rung = 1;
    return FMK_OK;
}

extern "C" int fmk_flow_bar_indexer_dev(fmk_ctx *ctx, int rule, int kind, const double *d_price, const void *d_amount,
                                        int amount_is_f64, const int8_t *d_side, int64_t n, double threshold,
                                        int64_t **d_close_idx, int64_t *n_idx)
{
    if (rule != 0 && rule != 1) return fmk_set_error(ctx, FMK_E_ARG, "flow bar indexer: rule must be 0 (imbalance) or 1 (run)");
    if (kind < 0 || kind > 2) return fmk_set_error(ctx, FMK_E_ARG, "flow bar indexer: kind must be 0 (tick), 1 (volume) or 2 (dollar)");
    if (n <= 0) return fmk_set_error(ctx, FMK_E_ARG, "flow bar indexer: empty input");
    if (!d_side || (kind >= 1 && !d_amount) || (kind == 2 && !d_price) || !d_close_idx || !n_idx)
        return fmk_set_error(ctx, FMK_E_ARG, "flow bar indexer: a column or result pointer is missing");
    *d_close_idx = nullptr;
    *n_idx = 0;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    const bool f64 = kind >= 1 && amount_is_f64;
#define FB_GO(R, K, F) return fb_run<R, K, F>(ctx, d_price, d_amount, d_side, n, threshold, d_close_idx, n_idx)
    if (rule == 0) {
        if (kind == 0) FB_GO(false, 0, false);
        if (kind == 1) { if (f64) FB_GO(false, 1, true); FB_GO(false, 1, false); }
        if (f64) FB_GO(false, 2, true);
        FB_GO(false, 2, false);
    }
    if (kind == 0) FB_GO(true, 0, false);
    if (kind == 1) { if (f64) FB_GO(true, 1, true); FB_GO(true, 1, false); }
    if (f64) FB_GO(true, 2, true);
    FB_GO(true, 2, false);
#undef FB_GO
}
