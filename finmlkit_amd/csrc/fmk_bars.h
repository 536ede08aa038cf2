// fmk_bars.h -- how a wave gets to its bars: what the per-bar kernels (fmk_ohlcv.hip, fmk_median.hip, fmk_tradesize.hip, fmk_barflow.hip,
// fmk_fused.h, fmk_footprint.hip) share.  None of it is the arithmetic of a bar.  DESIGN.md section 3.
// THE BAR LIST: 64-bit words, [0] = how many entries, entries from [FMK_BAR_LIST_HEAD] in any order (a 256-byte line away from the
// counter every appending wave hits).  An entry is a bar number; the redo lists put a column mask into bits 48 and up.  The host
// sizes it with fmk_bar_list_words(most entries) and clears FMK_BAR_LIST_CLEAR bytes.  Appends by a whole wave or workgroup
// (k_bar_dir_lanes, k_bar_trade_size_rows' flush, the scans behind the lane kernels) claim their slots themselves and write from
// FMK_BAR_LIST_HEAD + base: a shared wave-append moved registers in k_bar_dir_lanes' tick loop.  The lists of fmk_median.hip
// (k_long_bar_list[s]; read by k_bar_median_long and comp_bar_ohlcv's mid classes) are int64_t with the entries from [1]: several
// share one allocation, each with its own cap, and a workgroup claims the slots at once -- they keep that layout and their appends.
// THE THREE SCHEDULES by which a wave finds bars:
//  * list mode (fmk_list_count / fmk_list_bar): a wave per bar of an optional list `only`, or of all nb bars when there is none;
//  * the leftover pass (fmk_for_long_bars): 64 bars per step, one coalesced load of their close indices, a ballot of the bars of
//    more than min_cnt ticks, each of those then gets the whole wave;
//  * a lane per bar (fmk_lane_group_load): groups of 64 consecutive bars, their close indices in the wave's LDS row; per step the
//    longest run of the group's next bars whose ticks fit the wave's LDS tile, lane l taking bar l.  The steps stand in the two
//    kernels: as a shared function with the step as a callable they changed the order of the tile-fill loop's instructions.
// (k_bar_dir_lanes' 64 bars per wave without a tile is a fourth one and stays in fmk_barflow.hip.)
// The sorting network is plain C++17, so that a host program can check it (tools/lanesort_check.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <utility>

#ifdef __HIPCC__
#include "fmk_common.h"
#define FMK_HD __host__ __device__ __forceinline__
#else
#define FMK_HD static inline
#endif

// ---- bitonic sorting network on N registers of ONE lane; every index is a template constant, so the keys stay in VGPRs
template <int I, int J, int K, int N>
FMK_HD void fmk_lane_ce(uint32_t (&r)[N])
{
    constexpr int l = I ^ J;
    if constexpr (l > I) {
        const uint32_t a = r[I], b = r[l];
        const uint32_t mn = a < b ? a : b, mx = a < b ? b : a;
        if constexpr ((I & K) == 0) { r[I] = mn; r[l] = mx; }
        else { r[I] = mx; r[l] = mn; }
    }
}
template <int J, int K, int N, int... I>
FMK_HD void fmk_lane_stage(uint32_t (&r)[N], std::integer_sequence<int, I...>) { (fmk_lane_ce<I, J, K, N>(r), ...); }
template <int J, int K, int N>
FMK_HD void fmk_lane_js(uint32_t (&r)[N])
{
    fmk_lane_stage<J, K, N>(r, std::make_integer_sequence<int, N>{});
    if constexpr (J > 1) fmk_lane_js<J / 2, K, N>(r);
}
template <int K, int N>
FMK_HD void fmk_lane_ks(uint32_t (&r)[N])
{
    fmk_lane_js<K / 2, K, N>(r);
    if constexpr (K < N) fmk_lane_ks<K * 2, N>(r);
}
template <int N>
FMK_HD void fmk_lane_sort(uint32_t (&r)[N]) { fmk_lane_ks<2, N>(r); }
template <int N, int... I>
FMK_HD uint32_t fmk_lane_pick_seq(const uint32_t (&r)[N], int idx, std::integer_sequence<int, I...>)
{
    uint32_t v = r[0];
    ((v = idx == I ? r[I] : v), ...);
    return v;
}
// r[idx] for an index that is no constant (idx outside [0, N): r[0])
template <int N>
FMK_HD uint32_t fmk_lane_pick(const uint32_t (&r)[N], int idx) { return fmk_lane_pick_seq<N>(r, idx, std::make_integer_sequence<int, N>{}); }

// ---- the bar list: sizes (host and device)
#define FMK_BAR_LIST_HEAD 32             // words in front of the entries
#define FMK_BAR_LIST_CLEAR 8             // bytes the host clears before a kernel appends: the counter
FMK_HD size_t fmk_bar_list_words(int64_t cap) { return (size_t)(cap + FMK_BAR_LIST_HEAD); }

#ifdef __HIPCC__
// entry `it` as this lane reads it (the lanes may ask for different entries)
__device__ __forceinline__ int64_t fmk_list_entry(const unsigned long long *list, int64_t it) { return (int64_t)list[FMK_BAR_LIST_HEAD + it]; }
// one lane appends one entry
__device__ __forceinline__ void fmk_list_push(unsigned long long *list, unsigned long long entry) { list[FMK_BAR_LIST_HEAD + atomicAdd(list, 1ULL)] = entry; }

// ---- list mode: the bars of a wave-per-bar kernel with an optional list `only` (null: all nb bars)
__device__ __forceinline__ int64_t fmk_list_count(const unsigned long long *only, int64_t nb) { return only ? (int64_t)only[0] : nb; }
__device__ __forceinline__ int64_t fmk_list_bar(const unsigned long long *only, int64_t it) { return only ? fmk_uniform(fmk_list_entry(only, it)) : it; }

// ---- the raise-once flag: it only ever becomes 1 -- look first (shared reads do not serialise), store if still clear.  The
// caller picks the lane.
__device__ __forceinline__ void fmk_raise(int *flag)
{
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
        __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the leftover pass of a small-bar kernel: f(b, s, e), wave-uniform, for every bar of more than min_cnt ticks among the groups
// wave0, wave0 + nwaves, ... of 64 bars (walking the bars one by one cost a dependent load per bar: 2.3 ms per 2.5e7 bars of which
// a few per cent were long)
template <class F>
__device__ __forceinline__ void fmk_for_long_bars(const int64_t *__restrict__ ci, int64_t nb, int64_t min_cnt, int64_t wave0,
                                                  int64_t nwaves, int lane, F f)
{
    const int64_t ngroups = (nb + 63) >> 6;
    for (int64_t g = wave0; g < ngroups; g += nwaves) {
        const int64_t bl = g * 64 + lane;
        int64_t s_l = 0, e_l = 0;
        if (bl < nb) { s_l = ci[bl]; e_l = ci[bl + 1]; }
        unsigned long long todo = __builtin_amdgcn_ballot_w64(bl < nb && e_l - s_l > min_cnt);
        while (todo) {
            const int bit = fmk_uniform((int)__builtin_ctzll(todo));
            todo &= todo - 1;
            f(g * 64 + bit, fmk_readlane(s_l, bit), fmk_readlane(e_l, bit));
        }
    }
}

// ---- a lane per bar.  `row`: the wave's int64_t[66] in LDS.  The load puts the close indices of the group's bars B0 .. B0 + nbg - 1
// there (nbg + 1 of them) and returns nbg.
__device__ __forceinline__ int fmk_lane_group_load(int64_t *row, const int64_t *__restrict__ ci, int64_t nb, int64_t B0, int lane)
{
    const int nbg = (int)(nb - B0 < 64 ? nb - B0 : 64);
    __builtin_amdgcn_wave_barrier();
    if (lane <= nbg) row[lane] = ci[B0 + lane];
    if (lane == 0 && nbg == 64) row[64] = ci[B0 + 64];
    __builtin_amdgcn_wave_barrier();
    return nbg;
}
#endif  // __HIPCC__
