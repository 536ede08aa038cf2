// fmk_wgscan.h -- the two pieces every device-wide scan of this library is made of (reduce the tiles, scan the tile aggregates with
// ONE workgroup, scan the tiles again with their carries): the workgroup's exclusive scan and the aggregate-scan kernel, with the
// monoid as a parameter.  A new scan feature writes its monoid next to its own code and takes both pieces from here.
//
// A monoid M is a struct with
//   using T;                                      the element
//   static T identity();
//   static T combine(const T &first, const T &then);     ordered: `first` comes earlier in element order
//   template <int CTRL, int ROW_MASK> static T dpp(const T &);     every field through fmk_dpp, lanes without a source receive
//                                                 identity() (scalar monoids: the base FmkScalarDpp of fmk_dpp.h)
// The users: the integer sums of fmk_scan.h and fmk_label.hip, "last non-NaN" of fmk_cusum.hip, and the compositions of RcMap<K>
// (fmk_recur_core.h) and EwMap (fmk_ticklevel.hip).
//
// What deliberately stays out: k_dl_scan_dd and k_dl_scan_min (fmk_dollar.hip), k_vc_scan (fmk_volume.hip), fmk_threshold.hip,
// rv_block_carry (fmk_ticklevel.hip), the cusum chain and the cusum filter.  They are floating-point or double-double sums on a
// Kogge-Stone __shfl_up tree, or segmented scans; for a monoid that is not exact the tree IS the numerics, and the DPP tree below
// would move their bits.  k_synth_scan_tiles (it takes a carry-in and makes the benchmark's tape) and the hierarchical ew_scan_maps
// (its association is part of ewmst's bits) stay as they are too.  Two exact scans that could use these pieces keep their own, because
// they were measured slower on them (profiles/wgscan_refactor_timing.json): the running maximum of fmk_lasthead.h and "last non-zero"
// of the tick rule (fmk_preprocess.hip).
#pragma once
#include "fmk_common.h"
#include "fmk_dpp.h"

namespace {

// The values of the workgroup's NW * 64 threads in thread order: returns the ordered composition of the threads before this one
// (identity() for thread 0), *total = of all.  The lane scan is the tree of fmk_dpp_iscan; lanes without a source combine with the
// identity.  Two barriers: may be called again at once.
template <class M, int NW>
__device__ __forceinline__ typename M::T fmk_wg_exclusive(const typename M::T &mine, typename M::T *lds /* [NW] */, typename M::T *total)
{
    using T = typename M::T;
    const int lane = fmk_lane(), w = threadIdx.x >> 6;
    T inc = mine;
    inc = M::combine(M::template dpp<FMK_DPP_ROW_SHR(1), 0xF>(inc), inc);
    inc = M::combine(M::template dpp<FMK_DPP_ROW_SHR(2), 0xF>(inc), inc);
    inc = M::combine(M::template dpp<FMK_DPP_ROW_SHR(4), 0xF>(inc), inc);
    inc = M::combine(M::template dpp<FMK_DPP_ROW_SHR(8), 0xF>(inc), inc);
    inc = M::combine(M::template dpp<FMK_DPP_ROW_BCAST15, 0xA>(inc), inc);     // rows 1 and 3 take lane 15 of the row before
    inc = M::combine(M::template dpp<FMK_DPP_ROW_BCAST31, 0xC>(inc), inc);     // rows 2 and 3 take lane 31
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    T pre = M::identity();
    for (int k = 0; k < w; ++k) pre = M::combine(pre, lds[k]);
    T tot = lds[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) tot = M::combine(tot, lds[k]);
    *total = tot;
    const T prev = M::template dpp<FMK_DPP_WAVE_SHR1, 0xF>(inc);              // lane 0: the identity
    __syncthreads();
    return M::combine(pre, prev);
}

// The second launch, ONE workgroup: v[t] <- the ordered composition of v[0 .. t - 1] in place, THREADS aggregates per trip, the next
// trip's loaded ahead of the scan (a trip writes below the next one's values only); *total = the composition of all m when total is
// not null (it must not lie inside v[0 .. m - 1]).
template <class M, int THREADS>
__global__ __launch_bounds__(THREADS) void k_fmk_agg_scan(typename M::T *v, int64_t m, typename M::T *total /* may be null */)
{
    using T = typename M::T;
    __shared__ T wl[THREADS / 64];
    T run = M::identity();
    T nxt = (int64_t)threadIdx.x < m ? v[threadIdx.x] : M::identity();
    for (int64_t b = 0; b < m; b += THREADS) {
        const int64_t i = b + threadIdx.x;
        const T mine = nxt;
        nxt = i + THREADS < m ? v[i + THREADS] : M::identity();
        T tot;
        const T ex = fmk_wg_exclusive<M, THREADS / 64>(mine, wl, &tot);
        if (i < m) v[i] = M::combine(run, ex);
        run = M::combine(run, tot);
    }
    if (total && threadIdx.x == 0) *total = run;
}

}  // namespace
