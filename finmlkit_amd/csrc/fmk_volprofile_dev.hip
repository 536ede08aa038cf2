// fmk_volprofile_dev.hip -- volume_profile_developing (finmlkit/feature/core/volume.py:493-569) on gfx950: the session-anchored
// profile.  For a range [s, e) of bars the profile of bar t is the profile of bar t - 1 plus one footprint, in float32, in bar order;
// POC / HVA / LVA of every bar's profile come out.  Many ranges (one per trading day) in one call; the contract is in include/fmk.h.
//
// The bars of a range are cut into chunks of chunk_bars bars.  Two phases:
//   1 snapshots  one wave per range and slab of VPD_SLAB levels walks the range's bars in order (vp_add_bars: the rolling kernel's
//                aggregation loop) and stores its float32 buy / sell sums at every chunk boundary.  Levels never interact, and every
//                level sees its adds in bar order from zero: a snapshot holds the very bits the sequential loop has at that bar.
//   2 replay     one wave per chunk loads the chunk's snapshot and replays the chunk's bars; after every bar: total = buy + sell,
//                (bucketing: np.round(total, 8), trim of the zero ends, bucket_price_levels on what is left,) NumPy-pairwise total,
//                first argmax, the value-area walk by one lane -- the rolling kernel's device code paths (fmk_vp.h).
// A chunk's outputs depend on the bars in front of it only through the snapshot, so the results do not depend on chunk_bars.
#include <vector>

#include "fmk_vp.h"

#define VPD_SLAB 4096                       // levels one phase-1 wave keeps in LDS (buy + sell: 32 KiB)
#define VPD_SNAP_BUDGET ((size_t)512 << 20) // automatic chunk_bars: the most bytes the snapshots of a call may take
#define VPD_MIN_CHUNK 16                    // ... and the shortest chunk (a replay loads L levels and then serves >= 16 bars)
#define VPD_RI 8                            // int64 per range in the range table:
enum { RI_S, RI_E, RI_OUT, RI_MINL, RI_MAXL, RI_SNAP, RI_CHUNKS, RI_NAN };   // (RI_SNAP: the range's first float in the snapshots)

// Level range of every range: int(round(min(lows) / tick)) .. int(round(max(highs) / tick)) over ALL its bars (it looks ahead, as the
// reference does), half-even.  One workgroup per range.  np.min / np.max hand a NaN on (fmin / fmax would skip it): RI_NAN.
__global__ __launch_bounds__(256) void k_vpd_ranges(const double *__restrict__ highs, const double *__restrict__ lows, double tick,
                                                    int64_t *__restrict__ ri)
{
    __shared__ double smn[4], smx[4];
    __shared__ int snan[4];
    int64_t *w = ri + VPD_RI * (int64_t)blockIdx.x;
    const int64_t s = w[RI_S], e = w[RI_E];
    double mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    for (int64_t t = s + threadIdx.x; t < e; t += 256) {
        const double lo = lows[t], hi = highs[t];
        nan |= (lo != lo) | (hi != hi);
        mn = fmin(mn, lo); mx = fmax(mx, hi);
    }
    mn = fmk_wave_min(mn); mx = fmk_wave_max(mx);
    const bool wnan = __ballot(nan) != 0;
    if (fmk_lane() == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; snan[threadIdx.x >> 6] = wnan; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < 4; ++k) { mn = fmin(mn, smn[k]); mx = fmax(mx, smx[k]); nan |= snan[k] != 0; }
    nan |= snan[0] != 0;
    const double qlo = mn / tick, qhi = mx / tick;
    if (nan || !(fabs(qlo) < 0x1p61) || !(fabs(qhi) < 0x1p61)) { w[RI_MINL] = 0; w[RI_MAXL] = -1; w[RI_NAN] = 1; return; }
    w[RI_MINL] = (int64_t)rint(qlo); w[RI_MAXL] = (int64_t)rint(qhi); w[RI_NAN] = 0;
}

// Phase 1.  jobs[2 j] = range, jobs[2 j + 1] = first level (offset from the range's lowest) of the slab; only ranges of more than one
// chunk have jobs, and the bars of a range's last chunk are not walked: nobody needs the sums behind them.
// snap: per range, per chunk boundary c = 1 .. chunks - 1: buy[L] then sell[L], the sums in front of bar s + c * cb.
__global__ __launch_bounds__(64) void k_vpd_snapshots(const int64_t *__restrict__ off, const int32_t *__restrict__ levels,
                                                      const float *__restrict__ buy, const float *__restrict__ sell,
                                                      const int64_t *__restrict__ ri, const int64_t *__restrict__ jobs, int64_t cb,
                                                      float *__restrict__ snap)
{
    __shared__ float ab[VPD_SLAB], as[VPD_SLAB];
    const int lane = fmk_lane();
    const int64_t r = fmk_uniform(jobs[2 * (int64_t)blockIdx.x]), k0 = fmk_uniform(jobs[2 * (int64_t)blockIdx.x + 1]);
    const int64_t *w = ri + VPD_RI * r;
    const int64_t s = fmk_uniform(w[RI_S]), minl = fmk_uniform(w[RI_MINL]), Lr = fmk_uniform(w[RI_MAXL]) - minl + 1;
    const int64_t snap0 = fmk_uniform(w[RI_SNAP]), chunks = fmk_uniform(w[RI_CHUNKS]);
    const int L = (int)(Lr - k0 < VPD_SLAB ? Lr - k0 : VPD_SLAB);
    for (int k = lane; k < L; k += 64) { ab[k] = 0.f; as[k] = 0.f; }
    __builtin_amdgcn_wave_barrier();
    int64_t left = cb, c = 1;
    // (a level outside the slab belongs to another wave or is refused by the replay: not looked at here)
    (void)vp_add_bars(off, levels, buy, sell, s, s + (chunks - 1) * cb, minl + k0, L, ab, as, lane, [&](int64_t) {
        if (--left != 0) return;
        float *dst = snap + snap0 + (c - 1) * 2 * Lr + k0;
        for (int k = lane; k < L; k += 64) { dst[k] = ab[k]; dst[Lr + k] = as[k]; }
        __builtin_amdgcn_wave_barrier();
        left = cb; ++c;
    });
}

// per-wave working set of the replay: buy sums, sell sums, the bar's totals and -- when bucketing -- the bins, [cap + 8] floats each,
// then the tables of the pairwise sum (the tree routine fmk_np_sum).  cap: the call's widest range rounded up to 64 levels, not the
// class's capacity -- the value-area walk is one lane chasing LDS latency, and what hides it is more waves per CU (2 800 unbucketed
// levels: 35 KiB a wave instead of the 4 096 class's 67)
__host__ __device__ static inline size_t vpd_per_wave(int cap, bool binned) { return (size_t)(cap + 8) * (binned ? 16 : 12) + FMK_PW_PAR_STK * 4; }

template <bool GLOBAL>
__device__ __forceinline__ void vpd_visible()                      // what the lanes wrote, before other lanes read it
{
    if constexpr (GLOBAL) __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

// Phase 2.  cjobs[2 j] = range, cjobs[2 j + 1] = chunk of the range; one wave per chunk, waves stride over the chunks.
template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_vpd_replay(const int64_t *__restrict__ off, const int32_t *__restrict__ levels,
                                                    const float *__restrict__ buy, const float *__restrict__ sell,
                                                    const int64_t *__restrict__ ri, const int64_t *__restrict__ cjobs, int64_t n_chunks,
                                                    int64_t cb, int64_t n_bins, double va_pct, int cap, const float *__restrict__ snap,
                                                    int32_t *__restrict__ poc, int32_t *__restrict__ hva, int32_t *__restrict__ lva,
                                                    fmk_mail::Vpd *mail, unsigned char *gscratch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = fmk_lane();
    const int wib = fmk_uniform((int)(threadIdx.x >> 6));
    const int wpb = blockDim.x >> 6;
    const size_t per_wave = vpd_per_wave(cap, n_bins >= 0);
    unsigned char *mine;
    if constexpr (GLOBAL) mine = gscratch + ((size_t)blockIdx.x * wpb + wib) * per_wave;
    else mine = smem + (size_t)wib * per_wave;
    float *ab = (float *)mine;                                    // [cap + 8] buy sums
    float *as = ab + (cap + 8);                                   // [cap + 8] sell sums
    float *tot = as + (cap + 8);                                  // [cap + 8] the bar's totals (rounded when bucketing)
    float *bins = tot + (cap + 8);                                // [cap + 8] binned volumes (bucketing only)
    int *stk = (int *)(bins + (n_bins >= 0 ? cap + 8 : 0));       // FMK_PW_PAR_STK ints
    const int64_t nwaves = (int64_t)gridDim.x * wpb;
    for (int64_t j = (int64_t)blockIdx.x * wpb + wib; j < n_chunks; j += nwaves) {
        const int64_t r = fmk_uniform(cjobs[2 * j]), c = fmk_uniform(cjobs[2 * j + 1]);
        const int64_t *w = ri + VPD_RI * r;
        const int64_t s = fmk_uniform(w[RI_S]), e = fmk_uniform(w[RI_E]), out0 = fmk_uniform(w[RI_OUT]);
        const int64_t minl = fmk_uniform(w[RI_MINL]), maxl = fmk_uniform(w[RI_MAXL]), snap0 = fmk_uniform(w[RI_SNAP]);
        const int64_t Lr = maxl - minl + 1;
        if (Lr < 1 || Lr > cap) { if (lane == 0) atomicOr(&mail->status, VP_BAD_LEVEL); continue; }   // (the host refuses both before)
        const int L = (int)Lr;
        const int64_t t0 = s + c * cb, t1 = t0 + cb < e ? t0 + cb : e;
        if (c == 0) {
            for (int k = lane; k < L; k += 64) { ab[k] = 0.f; as[k] = 0.f; }
        } else {
            const float *src = snap + snap0 + (c - 1) * 2 * Lr;
            for (int k = lane; k < L; k += 64) { ab[k] = src[k]; as[k] = src[Lr + k]; }
        }
        vpd_visible<GLOBAL>();
        const bool bad = vp_add_bars(off, levels, buy, sell, t0, t1, minl, L, ab, as, lane, [&](int64_t t) {
            if constexpr (GLOBAL) __threadfence_block();
            // ---- developing_total_volumes = buy + sell (float32); bucketing: np.round(total, 8) in float32 = rint(v * 1e8) / 1e8, both
            //      operations rounded to float32 (1e8 is a float32), and the first / last entry that does not compare == 0
            int first = 0x7FFFFFFF, last = -1;
            for (int k = lane; k < L; k += 64) {
                float v = ab[k] + as[k];
                if (n_bins >= 0) {
                    v = __fdiv_rn(rintf(__fmul_rn(v, 1e8f)), 1e8f);
                    if (!(v == 0.f)) { first = k < first ? k : first; last = k; }       // (a NaN or a negative entry stops the trim)
                }
                tot[k] = v;
            }
            vpd_visible<GLOBAL>();
            const float *vol = tot;
            int np_ = L;
            VpPrices pl{minl, maxl, 1, 0, false};
            if (n_bins >= 0) {
                first = fmk_dpp_reduce(first, 0x7FFFFFFF, FmkOpMin());
                last = fmk_dpp_reduce(last, -1, FmkOpMax());
                if (last < 0) {                                   // trimmed to nothing: the reference's np.min of an empty array raises
                    if (lane == 0) {
                        atomicMax(&mail->zero_at, ~(((unsigned long long)r << 40) | (unsigned long long)(t - s)));
                        atomicOr(&mail->status, VP_ALL_ZERO);
                    }
                    return;
                }
                np_ = vp_bucket(tot + first, minl + first, minl + last, n_bins, true, bins, lane, pl);
                vpd_visible<GLOBAL>();
                vol = bins;
            }
            // ---- comp_poc_hva_lva
            const float total = fmk_np_sum([vol](int i) { return vol[i]; }, np_, lane, stk);   // np.sum of the float32 array
            const int pi = vp_argmax(vol, np_, lane);
            if (lane == 0) {
                int32_t p, hv, lv;
                vp_walk(vol, np_, pi, total, va_pct, pl, p, hv, lv);
                poc[out0 + (t - s)] = p; hva[out0 + (t - s)] = hv; lva[out0 + (t - s)] = lv;
            }
            __builtin_amdgcn_wave_barrier();
        });
        if (__ballot(bad) != 0 && lane == 0) atomicOr(&mail->status, VP_BAD_LEVEL);
        __builtin_amdgcn_wave_barrier();
    }
}

// chunk_bars of a call that leaves it to the entry: enough chunks for n_cu * 32 waves, no chunk shorter than
// VPD_MIN_CHUNK bars, doubled until the snapshots fit VPD_SNAP_BUDGET.  ri: the range table with the level ranges filled in.
static int64_t vpd_snapshot_floats(const std::vector<int64_t> &ri, int64_t cb)
{
    int64_t f = 0;
    for (size_t r = 0; r * VPD_RI < ri.size(); ++r) {
        const int64_t *w = &ri[r * VPD_RI];
        f += (fmk_ceil_div(w[RI_E] - w[RI_S], cb) - 1) * 2 * (w[RI_MAXL] - w[RI_MINL] + 1);
    }
    return f;
}
static int64_t vpd_auto_chunk(const std::vector<int64_t> &ri, int64_t total_bars, int n_cu)
{
    int64_t cb = fmk_ceil_div(total_bars, (int64_t)n_cu * 32);
    if (cb < VPD_MIN_CHUNK) cb = VPD_MIN_CHUNK;
    while ((size_t)vpd_snapshot_floats(ri, cb) * 4 > VPD_SNAP_BUDGET) cb *= 2;
    return cb;
}

extern "C" int fmk_volume_profile_developing_dev(fmk_ctx *ctx, const double *d_highs, const double *d_lows,
                                                 const int64_t *d_level_offsets, const int32_t *d_price_levels,
                                                 const float *d_buy_volumes, const float *d_sell_volumes, int64_t n_bars,
                                                 const int64_t *range_starts, const int64_t *range_ends, const int64_t *out_offsets,
                                                 int64_t n_ranges, int64_t n_bins, double price_tick, double va_pct, int64_t chunk_bars,
                                                 int32_t *d_poc, int32_t *d_hva, int32_t *d_lva)
{
    if (n_bars <= 0) return fmk_set_error(ctx, FMK_E_ARG, "Input arrays should have the same length and be non-empty.");
    if (!(price_tick > 0)) return fmk_set_error(ctx, FMK_E_ARG, "price_tick must be > 0");
    if (n_bins == 0) return fmk_set_error(ctx, FMK_E_ZERODIV, "integer division or modulo by zero");   // range // n_bins
    if (chunk_bars < 0) return fmk_set_error(ctx, FMK_E_ARG, "volume_profile_developing: chunk_bars must not be negative");
    if (n_ranges < 0 || n_ranges >= (1 << 24)) return fmk_set_error(ctx, FMK_E_ARG, "volume_profile_developing: fewer than 2^24 ranges a call");
    if (n_ranges == 0) return FMK_OK;
    std::vector<int64_t> ri((size_t)n_ranges * VPD_RI, 0);
    int64_t total_bars = 0;
    for (int64_t r = 0; r < n_ranges; ++r) {
        const int64_t s = range_starts[r], e = range_ends[r];
        if (s < 0 || e > n_bars || out_offsets[r] < 0)
            return fmk_set_error(ctx, FMK_E_ARG, "volume_profile_developing: range %lld reaches outside the bars", (long long)r);
        if (s >= e)                                                // np.min of an empty slice
            return fmk_set_error(ctx, FMK_E_ARG, "volume_profile_developing: range %lld is empty (zero-size array to reduction "
                                 "operation minimum which has no identity)", (long long)r);
        ri[r * VPD_RI + RI_S] = s; ri[r * VPD_RI + RI_E] = e; ri[r * VPD_RI + RI_OUT] = out_offsets[r];
        total_bars += e - s;
    }
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    struct Blocks {                                                // pool blocks of the call, given back on every way out
        fmk_ctx *c; std::vector<void *> p;
        ~Blocks() { for (void *q : p) (void)fmk_free(c, q); }
        int get(size_t bytes, void **out) { int rc = fmk_alloc(c, bytes ? bytes : 8, out); if (rc == FMK_OK) p.push_back(*out); return rc; }
    } blocks{ctx, {}};
    void *v;
    FMK_TRY(blocks.get(ri.size() * 8, &v));
    int64_t *d_ri = (int64_t *)v;
    FMK_TRY(fmk_h2d(ctx, d_ri, ri.data(), ri.size() * 8));
    k_vpd_ranges<<<(unsigned)n_ranges, 256, 0, ctx->stream>>>(d_highs, d_lows, price_tick, d_ri);
    FMK_LAUNCH_CHECK(ctx);
    FMK_TRY(fmk_d2h(ctx, ri.data(), d_ri, ri.size() * 8));
    int64_t max_levels = 0;
    for (int64_t r = 0; r < n_ranges; ++r) {
        const int64_t *w = &ri[r * VPD_RI];
        if (w[RI_NAN])
            return fmk_set_error(ctx, FMK_E_ARG, "volume_profile_developing: range %lld holds a NaN low or high, or its lows / highs over "
                                 "price_tick are not finite: no level range (the reference's int(round(nan)) raises here)", (long long)r);
        const int64_t L = w[RI_MAXL] - w[RI_MINL] + 1;
        if (L < 1) return fmk_set_error(ctx, FMK_E_LEVEL, "volume_profile_developing: range %lld: its highest high is below its lowest low", (long long)r);
        max_levels = L > max_levels ? L : max_levels;
    }
    if (max_levels > VP_MAX_LEVELS_GLOBAL)
        return fmk_set_error(ctx, FMK_E_CAPACITY, "volume_profile_developing: a range spans %lld price levels; this build "
                             "supports <= %d", (long long)max_levels, VP_MAX_LEVELS_GLOBAL);
    // ---- chunks, snapshots
    const int64_t cb = chunk_bars > 0 ? chunk_bars : vpd_auto_chunk(ri, total_bars, ctx->n_cu);
    std::vector<int64_t> jobs, cjobs;
    int64_t snap_floats = 0;
    for (int64_t r = 0; r < n_ranges; ++r) {
        int64_t *w = &ri[r * VPD_RI];
        const int64_t L = w[RI_MAXL] - w[RI_MINL] + 1, chunks = fmk_ceil_div(w[RI_E] - w[RI_S], cb);
        w[RI_SNAP] = snap_floats; w[RI_CHUNKS] = chunks;
        snap_floats += (chunks - 1) * 2 * L;
        if (chunks > 1)
            for (int64_t k0 = 0; k0 < L; k0 += VPD_SLAB) { jobs.push_back(r); jobs.push_back(k0); }
        for (int64_t c = 0; c < chunks; ++c) { cjobs.push_back(r); cjobs.push_back(c); }
    }
    const int64_t n_jobs = (int64_t)jobs.size() / 2, n_chunks = (int64_t)cjobs.size() / 2;
    if (n_jobs >= ((int64_t)1 << 31)) return fmk_set_error(ctx, FMK_E_CAPACITY, "volume_profile_developing: %lld snapshot slabs", (long long)n_jobs);
    FMK_TRY(fmk_h2d(ctx, d_ri, ri.data(), ri.size() * 8));
    FMK_TRY(blocks.get(cjobs.size() * 8, &v));
    int64_t *d_cjobs = (int64_t *)v;
    FMK_TRY(fmk_h2d(ctx, d_cjobs, cjobs.data(), cjobs.size() * 8));
    FMK_TRY(blocks.get((size_t)snap_floats * 4, &v));
    float *d_snap = (float *)v;
    if (n_jobs > 0) {
        FMK_TRY(blocks.get(jobs.size() * 8, &v));
        int64_t *d_jobs = (int64_t *)v;
        FMK_TRY(fmk_h2d(ctx, d_jobs, jobs.data(), jobs.size() * 8));
        k_vpd_snapshots<<<(unsigned)n_jobs, 64, 0, ctx->stream>>>(d_level_offsets, d_price_levels, d_buy_volumes, d_sell_volumes, d_ri,
                                                                   d_jobs, cb, d_snap);
        FMK_LAUNCH_CHECK(ctx);
    }
    // ---- replay: the rolling kernel's capacity classes (four waves a workgroup up to 1 024 levels, one above; LDS up to 8 192 levels)
    fmk_mail::Vpd *d_vpd = &ctx->d_mail->vpd, m;
    FMK_HIP(ctx, hipMemsetAsync(d_vpd, 0, sizeof *d_vpd, ctx->stream));
    const int cap = (int)((max_levels + 63) / 64 * 64), wpb = max_levels > 1024 ? 1 : 4;
    size_t smem = (size_t)wpb * vpd_per_wave(cap, n_bins >= 0);
    int64_t nblocks = fmk_ceil_div(n_chunks, wpb);
    int64_t capb = (int64_t)ctx->n_cu * 32;
    unsigned char *gscratch = nullptr;
    if (max_levels > VP_MAX_LEVELS) {                             // working set in global scratch (<= 8 GB, >= 16 waves)
        const size_t per_wave = smem;
        capb = (int64_t)(((size_t)8 << 30) / per_wave);
        if (capb < 16) capb = 16;
        if (capb > (int64_t)ctx->n_cu * 8) capb = (int64_t)ctx->n_cu * 8;
        if (nblocks > capb) nblocks = capb;
        void *scr;
        FMK_TRY(fmk_scratch(ctx, per_wave * (size_t)nblocks + 256, &scr));
        gscratch = (unsigned char *)scr;
        smem = 0;
    }
    if (smem > 64 * 1024)
        FMK_HIP(ctx, hipFuncSetAttribute((const void *)k_vpd_replay<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    if (nblocks > capb) nblocks = capb;
    if (gscratch)
        k_vpd_replay<true><<<(unsigned)nblocks, wpb * 64, 0, ctx->stream>>>(
            d_level_offsets, d_price_levels, d_buy_volumes, d_sell_volumes, d_ri, d_cjobs, n_chunks, cb, n_bins, va_pct, cap, d_snap,
            d_poc, d_hva, d_lva, d_vpd, gscratch);
    else
        k_vpd_replay<false><<<(unsigned)nblocks, wpb * 64, smem, ctx->stream>>>(
            d_level_offsets, d_price_levels, d_buy_volumes, d_sell_volumes, d_ri, d_cjobs, n_chunks, cb, n_bins, va_pct, cap, d_snap,
            d_poc, d_hva, d_lva, d_vpd, nullptr);
    FMK_LAUNCH_CHECK(ctx);
    FMK_TRY(fmk_read_back(ctx, &m, d_vpd, sizeof m));
    if (m.status & VP_BAD_LEVEL) return fmk_set_error(ctx, FMK_E_LEVEL, "volume_profile_developing: footprint level outside its range");
    if (m.status & VP_ALL_ZERO) {
        const unsigned long long at = ~m.zero_at;
        return fmk_set_error(ctx, FMK_E_LEVEL, "volume_profile_developing: range %lld, bar %lld of the range: every total volume rounds "
                             "to 0, nothing is left to bucket (the reference: zero-size array to reduction operation minimum which has "
                             "no identity)", (long long)(at >> 40), (long long)(at & ((1ull << 40) - 1)));
    }
    return FMK_OK;
}
