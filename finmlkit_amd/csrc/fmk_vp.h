// fmk_vp.h -- the device code paths the rolling (fmk_volprofile.hip) and the developing (fmk_volprofile_dev.hip) volume profile
// share: footprints of a run of bars added to a dense level histogram in bar order, bucket_price_levels, np.argmax, the value-area
// walk of comp_poc_hva_lva (finmlkit/feature/core/volume.py:196-200, :206-275, :278-365).  One wave each; `lane` = fmk_lane().
#ifndef FMK_VP_H
#define FMK_VP_H
#include "fmk_footprint.h"

#define VP_MAX_LEVELS 8192                  // widest window whose histogram lives in LDS
#define VP_MAX_LEVELS_GLOBAL (1 << 24)      // wider windows: histogram in global scratch
#define VP_NO_RANGE (1ull << 62)            // in place of the widest window: a window without a level range (a NaN low or high)

// status bits
#define VP_BAD_LEVEL 1      // a footprint level outside its window's range
#define VP_ONE_LEVEL 2      // bucketing a window that spans a single level (the rolling entry refuses it)
#define VP_ALL_ZERO 4       // developing profile: bucketing a profile whose every rounded total is 0

// aggregate_footprint's loop: the bars [s, e) ONE AFTER THE OTHER, lanes across the (distinct) levels of a bar, level l -> slot
// l - base of ab / as[0 .. L): every level sees its float32 adds in the reference's order.  The CSR offsets of up to 63 bars come by
// one coalesced load, a bar's first 64 rows are fetched while the previous bar is added.  after(t) runs once per bar, by the whole
// wave, when the adds of bar t are visible to every lane.  -> true (on some lane) when a level fell outside [base, base + L).
template <class After>
__device__ __forceinline__ bool vp_add_bars(const int64_t *__restrict__ off, const int32_t *__restrict__ levels,
                                            const float *__restrict__ buy, const float *__restrict__ sell, int64_t s, int64_t e,
                                            int64_t base, int L, float *ab, float *as, int lane, After &&after)
{
    bool bad = false;
    for (int64_t t0 = s; t0 < e; t0 += 63) {
        const int nbar = (int)(e - t0 < 63 ? e - t0 : 63);
        const int64_t my_off = lane <= nbar ? off[t0 + lane] : 0;
        int64_t r0 = fmk_readlane(my_off, 0), r1 = fmk_readlane(my_off, 1);
        int lv = 0;
        float bv = 0.f, sv = 0.f;
        bool has = r0 + lane < r1;
        if (has) { lv = levels[r0 + lane]; bv = buy[r0 + lane]; sv = sell[r0 + lane]; }
        for (int q = 0; q < nbar; ++q) {
            const int64_t c0 = r0, c1 = r1;
            const int clv = lv;
            const float cbv = bv, csv = sv;
            const bool chas = has;
            if (q + 1 < nbar) {                               // the next bar's first rows, in flight during the adds below
                r0 = r1; r1 = fmk_readlane(my_off, q + 2);
                has = r0 + lane < r1;
                if (has) { lv = levels[r0 + lane]; bv = buy[r0 + lane]; sv = sell[r0 + lane]; }
            }
            if (chas) {
                const int64_t idx = (int64_t)clv - base;
                if (idx < 0 || idx >= L) bad = true;
                else { ab[idx] += cbv; as[idx] += csv; }      // float32 += float32, one add per level per bar
            }
            for (int64_t r = c0 + 64 + lane; r < c1; r += 64) {
                const int64_t idx = (int64_t)levels[r] - base;
                if (idx < 0 || idx >= L) { bad = true; continue; }
                ab[idx] += buy[r];
                as[idx] += sell[r];
            }
            __builtin_amdgcn_wave_barrier();
            after(t0 + q);
        }
    }
    return bad;
}

// The price of profile entry k: a level of the dense range [minl, maxl], or -- bucketed -- a bin's midpoint (e_k + e_k+1 - 1) // 2,
// the maximum for the leftover bin.
struct VpPrices {
    int64_t minl, maxl, bw, nbk;
    bool binned;
    __device__ __forceinline__ int32_t operator()(int k) const
    {
        if (!binned) return (int32_t)(minl + k);
        if (k < nbk) return (int32_t)(minl + (int64_t)k * bw + (bw - 1) / 2);
        return (int32_t)maxl;
    }
};

// bucket_price_levels on the dense levels minl .. maxl with the totals tot[0 .. maxl - minl]: width max(1, range // n_bins) made
// odd, edges = arange(min, max + width, width), one lane per bin adding its levels in level order (float32), the leftover bin iff
// the last level falls past the bins.  -> the number of entries written to bins[]; 0 and nothing written when the edges enclose
// no bin (one level) and !one_level_ok.  With one_level_ok that level comes back as the only (leftover) bin, as the interpreted
// reference hands it back behind its warning.
__device__ __forceinline__ int vp_bucket(const float *tot, int64_t minl, int64_t maxl, int64_t n_bins, bool one_level_ok, float *bins,
                                         int lane, VpPrices &pr)
{
    const int64_t range = maxl - minl;
    const int L = (int)(range + 1);
    int64_t bw = range / n_bins;
    if (bw < 1) bw = 1;
    if (bw % 2 == 0) bw += 1;
    const int64_t n_edges = (range + bw + bw - 1) / bw;   // len(arange(min, max + bw, bw))
    const int64_t nbk = n_edges - 1;
    pr.minl = minl; pr.maxl = maxl; pr.bw = bw; pr.nbk = nbk; pr.binned = true;
    if (n_edges < 2 && !one_level_ok) return 0;
    const int np_ = (int)(nbk + ((range / bw >= nbk) ? 1 : 0));     // + leftover bin iff the last level falls past the bins
    for (int b = lane; b < np_; b += 64) {
        const int64_t k0 = (int64_t)b * bw;
        const int64_t k1 = (b == nbk) ? L : (k0 + bw < L ? k0 + bw : L);
        float acc = 0.f;
        for (int64_t k = k0; k < k1; ++k) acc += tot[k];   // float32 adds in level order (volume.py:262-270)
        bins[b] = acc;
    }
    __builtin_amdgcn_wave_barrier();
    return np_;
}

// np.argmax of vol[0 .. n): the first maximum, the first NaN is the maximum; 0 for n == 0.  Uniform across the wave.
__device__ __forceinline__ int vp_argmax(const float *vol, int n, int lane)
{
    float best = -INFINITY;
    int best_i = 0x7FFFFFFF;
    for (int k = lane; k < n; k += 64) {
        const float v = vol[k];
        if (v > best || (v != v && best == best)) { best = v; best_i = k; }
    }
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
        const float ob = __shfl_xor(best, x, 64);
        const int oi = __shfl_xor(best_i, x, 64);
        const bool on = ob != ob, bn = best != best;
        const bool take = on ? (!bn || oi < best_i) : (!bn && (ob > best || (ob == best && oi < best_i)));
        if (take) { best = ob; best_i = oi; }
    }
    return best_i == 0x7FFFFFFF ? 0 : best_i;
}

// The value-area walk of comp_poc_hva_lva from the POC at entry pi, by ONE lane: float64 scalars (Numba-typed semantics), threshold
// float(total) * (va_pct / 100), two entries a step towards the heavier side, -1.0 for an exhausted side.
template <class Prices>
__device__ __forceinline__ void vp_walk(const float *vol, int n, int pi, float total, double va_pct, const Prices &pl, int32_t &poc_price,
                                        int32_t &hv, int32_t &lv)
{
    poc_price = pl(pi);
    const double va_thrs = (double)total * (va_pct / 100.0);
    double cum = vol[pi];
    hv = poc_price; lv = poc_price;
    int up = pi + 1, down = pi - 1;
    double cu = 0.0, cd = 0.0;
    if (up < n) { cu = vol[up]; if (up + 1 < n) cu += vol[up + 1]; }
    if (down >= 0) { cd = vol[down]; if (down - 1 >= 0) cd += vol[down - 1]; }
    while (cum < va_thrs) {
        if (cu > cd) {
            cum += cu;
            hv = pl(up + 1 < n - 1 ? up + 1 : n - 1);
            up += 2;
            cu = -1.0;
            if (up < n) { cu = vol[up]; if (up + 1 < n) cu += vol[up + 1]; }
        } else if (cu < cd) {
            cum += cd;
            lv = pl(down - 1 > 0 ? down - 1 : 0);
            down -= 2;
            cd = -1.0;
            if (down >= 0) { cd = vol[down]; if (down - 1 >= 0) cd += vol[down - 1]; }
        } else if (cu == cd && cd != -1.0) {
            cum += cu + cd;
            hv = pl(up + 1 < n - 1 ? up + 1 : n - 1);
            lv = pl(down - 1 > 0 ? down - 1 : 0);
            up += 2; down -= 2;
            cu = -1.0;
            if (up < n) { cu = vol[up]; if (up + 1 < n) cu += vol[up + 1]; }
            cd = -1.0;
            if (down >= 0) { cd = vol[down]; if (down - 1 >= 0) cd += vol[down - 1]; }
        } else break;                                      // the reference's "stuck in loop" exit
    }
}

#endif
