// fmk_cusum_filter.h -- the symmetric CUSUM event filter (finmlkit/sampling/filters.py:7-70) on gfx950.
// Included by fmk_cusum.hip after fmk_cusum_onepass.h.  The rule below is cf_tick of fmk_cusum_rule.h (CsState, cs_same and cs_lane
// live there too).  From fmk_cusum_onepass.h come the CS1_* geometry, the fix-up's lockstep walk (cs1_fix_body: k_cf_fix is that body
// on the source CfSrc), Cs1Fix, the scratch layout Cs1Work, the counts / emit kernels and their host tail cs1_emit_all.  Pass A and the
// re-walk are this file's own: sharing the walker's tile with k_cs1_pass reorders that kernel's listing.
//
// The rule, for i = 1 .. n-1 (tick i sits at offset t = i - 1 of the chunked stream, m = n - 1 ticks):
//     ret   = log(x[i] / x[i-1])                     (fmk_log_ratio: the host's log of the rounded quotient)
//     s_pos = max(0.0, s_pos + ret);  s_neg = min(0.0, s_neg + ret)          (NaN -> 0.0, never -0.0)
//     if   s_neg < -thr[i]: s_neg = 0.0, event i     (the NEGATIVE side first, strict comparisons)
//     elif s_pos >  thr[i]: s_pos = 0.0, event i
// thr is one constant (n_thr == 1) or one value per element.  What differs from _cusum_bar_indexer: strict comparisons, the negative
// side first, no same-timestamp block rule, no floor / multiplier / forward fill, any float64 series.  A NaN threshold never fires, a
// negative one fires the negative side on every tick, non-positive or NaN x gives NaN returns that clamp to 0.0: all of it falls out of
// the selects of cf_tick, there is no special code.
//
// The state is again two float64 that are never NaN and never -0.0, so the scheme of fmk_cusum_onepass.h carries over:
//   pass A  (k_cf_pass<PER, false>) : 32 chunks of CS1_L ticks per workgroup, 64-tick tiles through LDS, 32 walker lanes that start
//                                     from (0, 0) CS1_W ticks in front of their chunk; closes as 16-bit offsets in the chunk's staging
//                                     row, entry state E, exit state S0.  PER = false (constant threshold): x only, 8 B/tick, no
//                                     threshold tile in LDS; PER = true: x and thr, 16 B/tick.
//   fix-up  (k_cf_fix<PER>)         : a wave per chunk whose true entry state is not the one its record was made from: lane 0 walks from
//                                     the true state, lane 1 from E, and they merge on bitwise-equal states (cs1_fix_body).
//   re-walk (k_cf_pass<PER, true>)  : the loop of pass A without the warm-up, a LANE per chunk, from the exit state of the chunk before:
//                                     the staging row, E and S0 are made anew from that entry state.  For tapes that do not forget
//                                     within a chunk (wide thresholds), where a wave per chunk would walk every chunk over its whole
//                                     length with one lane.
// Both schedules are the same fixed point -- chunk 0 is exact from the start, every launch makes at least one more chunk exact, stop
// when no exit state changes -- and both are exact on every input; "more than a quarter of the chunks pending after the first fix-up
// launch" and the launch cap only switch from the wave-per-chunk fix-up to the lane-per-chunk re-walk.
#pragma once

#define CF_MAX_FIX_LAUNCHES 24     // fix-up launches after which the default schedule goes over to the re-walk

// PER: one threshold per element (thr[i]); otherwise the constant thr[0].
// REWALK = false: pass A.  Every chunk is walked from (0, 0), CS1_W ticks in front of it -> E, S0, C0, staged.
// REWALK = true : chunk k >= 1 whose record was not made from S_read[k - 1] is walked again from exactly that state, without a warm-up
//                 -> E = last_in = that state, S0 = S = the exit state, C0, staged, fix = {0, 0}; `changed` counts exit states that
//                 differ from S_read[k].  A workgroup none of whose chunks needs it returns at once.
template <bool PER, bool REWALK>
__global__ __launch_bounds__(256) void k_cf_pass(const double *__restrict__ x, const double *__restrict__ thr, int64_t n, int64_t m,
                                                 int64_t chunks, CsState *__restrict__ E, CsState *__restrict__ S0,
                                                 int *__restrict__ C0, unsigned short *__restrict__ staged,
                                                 const CsState *__restrict__ S_read, CsState *__restrict__ S,
                                                 CsState *__restrict__ last_in, Cs1Fix *__restrict__ fix, unsigned long long *changed)
{
    __shared__ double s_r[CS1_TK][CS1_TJ + 1];
    __shared__ double s_l[PER ? CS1_TK : 1][CS1_TJ + 1];
    __shared__ unsigned s_need;
    const int64_t k0 = (int64_t)blockIdx.x * CS1_TK;
    const int col = threadIdx.x & (CS1_TJ - 1), row4 = threadIdx.x / CS1_TJ;
    constexpr int RP = 256 / CS1_TJ;                                     // rows per pass of the load phase
    constexpr int NR = CS1_TK / RP;                                      // rows per thread and tile
    const int64_t kw = k0 + threadIdx.x;                                 // the walker's chunk
    const bool mine = threadIdx.x < CS1_TK && kw < chunks;
    const double lam = PER ? 0.0 : thr[0];
    double sp = 0.0, sn = 0.0;
    int cnt = 0;
    CsState in;
    in.sp = 0.0; in.sn = 0.0;
    bool walk = mine;
    unsigned need = ~0u;                                                 // rows (chunks of this workgroup) whose inputs are wanted
    if (REWALK) {
        walk = false;
        if (mine && kw > 0) {
            in = S_read[kw - 1];
            walk = !cs_same(in, last_in[kw]);
        }
        if (threadIdx.x < 64) {                                          // the walkers are lanes 0 .. 31 of the first wave
            const unsigned long long b = __builtin_amdgcn_ballot_w64(walk);
            if (threadIdx.x == 0) s_need = (unsigned)b;
        }
        __syncthreads();
        need = s_need;
        if (need == 0) return;
        sp = in.sp; sn = in.sn;
    }
    const int len_w = mine ? (int)(m - kw * CS1_L < CS1_L ? m - kw * CS1_L : CS1_L) : 0;
    unsigned short *my = staged + (mine ? kw : 0) * (int64_t)CS1_L;
    for (int j0 = REWALK ? 0 : -CS1_W; j0 < CS1_L; j0 += CS1_TJ) {
        // raw inputs of the tile: all loads first, then the arithmetic.  x[i - 1] is the neighbouring lane's own load except at
        // lane 0 of the 64-tick row, which fetches it as a halo word
        double p[NR], th[NR], halo[NR];
        unsigned okm = 0;
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int row = rr * RP + row4;
            const int64_t t = (k0 + row) * CS1_L + j0 + col;
            const bool ok = k0 + row < chunks && t >= 0 && t < m && ((need >> row) & 1u);
            okm |= (ok ? 1u : 0u) << rr;
            const int64_t i = 1 + (ok ? t : 0);                          // (n >= 2: x[1] and x[0] exist)
            p[rr] = x[i];
            th[rr] = PER ? thr[i] : 0.0;
            halo[rr] = 0.0;
            if (col == 0) halo[rr] = x[i - 1];
        }
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int row = rr * RP + row4;
            const double up = __shfl_up(p[rr], 1, 64);
            const double pm = col == 0 ? halo[rr] : up;
            double r = 0.0, l = NAN;                                     // outside the stream: never read by a walker
            if ((okm >> rr) & 1u) {
                r = fmk_log_ratio(p[rr], pm);
                l = th[rr];
            }
            s_r[row][col] = r;
            if (PER) s_l[row][col] = l;
        }
        __syncthreads();
        if (walk) {
            if (!REWALK && j0 == 0) { E[kw].sp = sp; E[kw].sn = sn; }
            // ticks of this tile that belong to the stream: the warm-up of chunk 0 lies in front of it, the last chunk may end inside
            // a tile (that one tile is walked tick by tick); the ticks behind are not walked at all
            const int nv = j0 < 0 ? (kw > 0 ? CS1_TJ : 0) : len_w - j0;
            unsigned long long mask = 0;
            if (nv >= CS1_TJ) {
                // the rule as selects, one basic block per 8 ticks; the events go into a bit mask and are stored after the tile
#pragma unroll
                for (int j8 = 0; j8 < CS1_TJ; j8 += 8) {
                    double r8[8], l8[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        r8[q] = s_r[threadIdx.x][j8 + q];
                        l8[q] = PER ? s_l[PER ? threadIdx.x : 0][j8 + q] : lam;
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) mask |= (unsigned long long)cf_tick(sp, sn, r8[q], l8[q]) << (j8 + q);
                }
            } else {
                for (int q = 0; q < nv; ++q) {
                    const double l = PER ? s_l[PER ? threadIdx.x : 0][q] : lam;
                    mask |= (unsigned long long)cf_tick(sp, sn, s_r[threadIdx.x][q], l) << q;
                }
            }
            if (j0 >= 0)
                while (mask) {
                    my[cnt++] = (unsigned short)(j0 + __builtin_ctzll(mask));
                    mask &= mask - 1;
                }
        }
        __syncthreads();
    }
    if (walk) {
        CsState out;
        out.sp = sp; out.sn = sn;
        S0[kw] = out;
        C0[kw] = cnt;
        if (REWALK) {
            E[kw] = in;
            last_in[kw] = in;
            fix[kw].pfx_a = 0; fix[kw].pfx_t = 0;
            if (!cs_same(S_read[kw], out)) atomicAdd(changed, 1ULL);
            S[kw] = out;
        }
    }
}

// the filter's ticks for cs1_fix_body: tick t of the stream is element 1 + t of x (and of thr when there is one per element)
template <bool PER>
struct CfSrc {
    const double *__restrict__ x, *__restrict__ thr;
    int64_t n;
    double lam;                                                          // the constant threshold, read once
    __device__ __forceinline__ CfSrc(const double *x_, const double *thr_, int64_t n_) : x(x_), thr(thr_), n(n_), lam(PER ? 0.0 : thr_[0]) {}
    struct Raw { double p, pm, th; };
    static __device__ __forceinline__ Raw idle() { return Raw{1.0, 1.0, NAN}; }
    __device__ __forceinline__ Raw load(int64_t t) const
    {
        int64_t i = 1 + t;
        if (i > n - 1) i = n - 1;                                        // lanes past the chunk: any valid address
        return Raw{x[i], x[i - 1], PER ? thr[i] : lam};
    }
    __device__ __forceinline__ void eval(const Raw &c, int64_t, double &r, double &l) const
    {
        r = fmk_log_ratio(c.p, c.pm);                                    // the expressions of k_cf_pass
        l = c.th;
    }
    static __device__ __forceinline__ unsigned tick(double &sp, double &sn, double r, double l) { return cf_tick(sp, sn, r, l); }
};

// One wave per chunk k >= 1 whose true entry state S_read[k - 1] is not the one its staging row was made from (cs1_fix_body)
template <bool PER>
__global__ __launch_bounds__(256) void k_cf_fix(const double *__restrict__ x, const double *__restrict__ thr, int64_t n, int64_t m,
                                                int64_t chunks, const CsState *__restrict__ E, const CsState *__restrict__ S0,
                                                const CsState *__restrict__ S_read, CsState *__restrict__ S,
                                                CsState *__restrict__ last_in, Cs1Fix *__restrict__ fix,
                                                unsigned short *__restrict__ patch, int limit, unsigned long long *changed,
                                                unsigned long long *pending)
{
    cs1_fix_body(CfSrc<PER>(x, thr, n), m, chunks, E, S0, S_read, S, last_in, fix, patch, limit, changed, pending);
}

static int64_t g_cf_last[4];            // last call: form that answered (0 one pass + fix-up, 1 re-walk), launches, pending after the first, chunks
extern "C" int fmk_diag_cusum_filter_last(int64_t *form, int64_t *fix_launches, int64_t *pending_first, int64_t *chunks)
{
    if (form) *form = g_cf_last[0];
    if (fix_launches) *fix_launches = g_cf_last[1];
    if (pending_first) *pending_first = g_cf_last[2];
    if (chunks) *chunks = g_cf_last[3];
    return FMK_OK;
}

template <bool PER>
static int cf_run(fmk_ctx *ctx, const double *d_x, int64_t n, const double *d_thr, int64_t *d_out, int64_t capacity, int64_t *n_out,
                  int64_t *n_rounds)
{
    const int64_t m = n - 1;
    const int64_t chunks = fmk_ceil_div(m, (int64_t)CS1_L);
    g_cf_last[0] = 0; g_cf_last[1] = 0; g_cf_last[2] = 0; g_cf_last[3] = chunks;
    int force = 0;                                                       // FMK_CUSUM_FILTER_FORM (tests): 1 the fix-up only, 2 the re-walk only
    if (const char *v = getenv("FMK_CUSUM_FILTER_FORM")) {
        if (!strcmp(v, "onepass")) force = 1;
        else if (!strcmp(v, "fixed")) force = 2;
        else if (*v) return fmk_set_error(ctx, FMK_E_ARG, "FMK_CUSUM_FILTER_FORM must be onepass or fixed");
    }
    Cs1Work w;
    FMK_TRY(cs1_work(ctx, chunks, &w));
    fmk_mail::Cusum::Round *d_round = w.d_round, r;
    const unsigned pass_grid = (unsigned)fmk_ceil_div(chunks, (int64_t)CS1_TK);
    k_cf_pass<PER, false><<<pass_grid, 256, 0, ctx->stream>>>(d_x, d_thr, n, m, chunks, w.E, w.S0, w.C0, w.staged, nullptr, nullptr,
                                                            nullptr, nullptr, nullptr);
    FMK_LAUNCH_CHECK(ctx);
    FMK_TRY(cs1_after_pass(ctx, w));
    int64_t rounds = 1, launches = 0;
    int limit = CS1_FIRST_LIMIT;
    bool rewalk = force == 2;
    while (chunks > 1) {
        FMK_TRY(cs1_round_begin(ctx, w));
        FMK_HIP(ctx, hipMemsetAsync(d_round, 0, sizeof *d_round, ctx->stream));
        if (rewalk)
            k_cf_pass<PER, true><<<pass_grid, 256, 0, ctx->stream>>>(d_x, d_thr, n, m, chunks, w.E, w.S0, w.C0, w.staged, w.S_read, w.S,
                                                                   w.last_in, w.fix, &d_round->changed);
        else
            k_cf_fix<PER><<<(unsigned)fmk_ceil_div(chunks - 1, (int64_t)4), 256, 0, ctx->stream>>>(
                d_x, d_thr, n, m, chunks, w.E, w.S0, w.S_read, w.S, w.last_in, w.fix, w.patch, limit, &d_round->changed, &d_round->pending);
        FMK_LAUNCH_CHECK(ctx);
        ++launches; ++rounds;
        FMK_TRY(fmk_read_back(ctx, &r, d_round, sizeof r));
        const int64_t changed = (int64_t)r.changed, pending = (int64_t)r.pending;
        g_cf_last[1] = launches;
        if (launches == 1 && !rewalk) g_cf_last[2] = pending;
        limit = CS1_L;
        if (changed == 0 && pending == 0) break;                          // every record was made from, or patched to, its true entry state
        if (rounds > chunks + 2) return fmk_set_error(ctx, FMK_E_HIP, "cusum_filter: fixed point did not converge");
        // the tape does not forget within CS1_FIRST_LIMIT ticks, or the fix-up drags on: the same fixed point, a lane per chunk
        if (!rewalk && force != 1 && ((launches == 1 && pending > chunks / 4 + 1) || launches >= CF_MAX_FIX_LAUNCHES)) rewalk = true;
    }
    g_cf_last[0] = rewalk ? 1 : 0;
    // tick t of chunk k is element 1 + k * CS1_L + t of the series (k_cs1_emit's `first` = 0); no opening entry
    int64_t total = -1;
    const int rc = cs1_emit_all(ctx, w, chunks, 0, d_out, 0, capacity, "cusum_filter: %lld event indices, capacity %lld", &total);
    if (total >= 0) {                                                    // the count was read: also reported with "capacity" (the caller asks again)
        if (n_out) *n_out = total;
        if (n_rounds) *n_rounds = rounds;
    }
    return rc;
}

extern "C" int fmk_cusum_filter_dev(fmk_ctx *ctx, const double *d_x, int64_t n, const double *d_thr, int64_t n_thr, int64_t *d_out,
                                    int64_t capacity, int64_t *n_out, int64_t *n_rounds)
{
    if (n <= 1) return fmk_set_error(ctx, FMK_E_ARG, "Input time series must have at least 2 elements.");
    if (n_thr != 1 && n_thr != n)
        return fmk_set_error(ctx, FMK_E_ARG, "Threshold array must either contain 1 const. element or len(raw_time_series) elements.");
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    return n_thr == 1 ? cf_run<false>(ctx, d_x, n, d_thr, d_out, capacity, n_out, n_rounds)
                      : cf_run<true>(ctx, d_x, n, d_thr, d_out, capacity, n_out, n_rounds);
}
