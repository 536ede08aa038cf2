// fmk_lasthead.h -- the device-wide "index of the last head at or before me" scan: h(i) = the largest j <= i whose flag is set, or
// LH_NONE.  A running maximum over flagged indices (fmk_clock.hip: dir_run_len's run starts, orb_break's day starts; DESIGN.md
// section 7i).  Three launches on the context's stream in the manner of fmk_recur_core.h, no workgroup waits for another.  The workgroup
// scan and the aggregate scan are this file's own, not those of fmk_wgscan.h: on those, dir_run_len took 0.003 ms more per 1e8 elements
// (0.412 -> 0.415 ms, in k_lh_aggscan and k_lh_apply; profiles/wgscan_refactor_timing.json).
//   k_lh_tiles    every thread loads its LH_ITEMS consecutive elements and keeps the last flagged index among them; the workgroup's
//                 maximum goes to one int per tile (LH_NONE: no head in the whole tile).
//   k_lh_aggscan  one workgroup: the tile values become the running maximum over the tiles before each (exclusive), LH_AGG_UNIT
//                 tiles per trip.
//   k_lh_apply    loads the elements again, takes the running maximum over the threads before it in the workgroup and the tile's
//                 carry, then walks its elements: a flagged element becomes the head, emit() is handed the head.
// Indices are 32-bit: the callers refuse series of 2^31 elements and more (fmk_series_check).
//
// A functor F gives: In (the thread's elements), load(i0, n, whole, in), flag(in, j, i) for element j of the thread (index i < n),
// emit(in, j, i, h) for the same, and finish(in, i0, n, whole) after the thread's last emit(), which stores what the emits left in `in`.
#pragma once
#include "fmk_common.h"

#define LH_THREADS 256
#define LH_ITEMS 8                   // consecutive elements per thread
#define LH_TILE (LH_THREADS * LH_ITEMS)
#define LH_AGG_UNIT LH_THREADS       // tile values per trip of the aggregate scan
#define LH_NONE (-1)

namespace {

__device__ __forceinline__ bool lh_whole(int64_t tile, int64_t n) { return tile > 0 && (tile + 1) * LH_TILE <= n; }

// The values of the workgroup's 256 threads in thread order: returns the maximum over the threads before this one (LH_NONE for
// thread 0), *total = over all.  Two barriers: may be called again at once.
__device__ __forceinline__ int lh_block_exclusive(int mine, int *lds /* [LH_THREADS / 64] */, int *total)
{
    const int lane = fmk_lane(), w = threadIdx.x >> 6;
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc = up > inc ? up : inc;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int pre = LH_NONE, tot = LH_NONE;
#pragma unroll
    for (int k = 0; k < LH_THREADS / 64; ++k) {
        const int v = lds[k];
        if (k < w) pre = v > pre ? v : pre;
        tot = v > tot ? v : tot;
    }
    *total = tot;
    int prev = __shfl_up(inc, 1, 64);
    if (lane == 0) prev = LH_NONE;
    __syncthreads();
    return prev > pre ? prev : pre;
}

// the last flagged index among the thread's elements of tile `tile`
template <class F>
__device__ __forceinline__ int lh_thread_last(const F &f, int64_t tile, int64_t n, typename F::In &in)
{
    const int64_t i0 = tile * LH_TILE + (int64_t)threadIdx.x * LH_ITEMS;
    f.load(i0, n, lh_whole(tile, n), in);
    int last = LH_NONE;
#pragma unroll
    for (int j = 0; j < LH_ITEMS; ++j) {
        const int64_t i = i0 + j;
        if (i < n && f.flag(in, j, i)) last = (int)i;
    }
    return last;
}

template <class F>
__global__ __launch_bounds__(LH_THREADS) void k_lh_tiles(F f, int64_t n, int *__restrict__ tile_last)
{
    __shared__ int wl[LH_THREADS / 64];
    typename F::In in;
    const int last = lh_thread_last(f, blockIdx.x, n, in);
    int tot;
    (void)lh_block_exclusive(last, wl, &tot);
    if (threadIdx.x == 0) tile_last[blockIdx.x] = tot;
}

// one workgroup: v[t] <- max(v[0 .. t - 1]) (LH_NONE for t == 0), LH_AGG_UNIT values per trip; a trip reads its values before it
// writes them and no trip touches another's
__global__ __launch_bounds__(LH_THREADS) void k_lh_aggscan(int *v, int64_t m)
{
    __shared__ int wl[LH_THREADS / 64];
    int run = LH_NONE;
    for (int64_t b = 0; b < m; b += LH_AGG_UNIT) {
        const int64_t i = b + threadIdx.x;
        const int mine = i < m ? v[i] : LH_NONE;
        int tot;
        const int ex = lh_block_exclusive(mine, wl, &tot);
        if (i < m) v[i] = ex > run ? ex : run;
        run = tot > run ? tot : run;
    }
}

template <class F>
__global__ __launch_bounds__(LH_THREADS) void k_lh_apply(F f, int64_t n, const int *__restrict__ tile_pre)
{
    __shared__ int wl[LH_THREADS / 64];
    typename F::In in;
    const int last = lh_thread_last(f, blockIdx.x, n, in);
    int tot;
    const int ex = lh_block_exclusive(last, wl, &tot);
    const int carry = tile_pre[blockIdx.x];
    int h = ex > carry ? ex : carry;
    const int64_t i0 = (int64_t)blockIdx.x * LH_TILE + (int64_t)threadIdx.x * LH_ITEMS;
#pragma unroll
    for (int j = 0; j < LH_ITEMS; ++j) {
        const int64_t i = i0 + j;
        if (i >= n) break;
        if (f.flag(in, j, i)) h = (int)i;
        f.emit(in, j, i, h);
    }
    f.finish(in, i0, n, lh_whole(blockIdx.x, n));
}

// the scan over n > 0 elements (n < 2^31) on the context's stream
template <class F>
int lh_scan(fmk_ctx *ctx, const F &f, int64_t n)
{
    const int64_t tiles = fmk_ceil_div(n, LH_TILE);
    void *scr;
    FMK_TRY(fmk_scratch(ctx, (size_t)tiles * sizeof(int), &scr));
    int *tile_last = (int *)scr;
    k_lh_tiles<F><<<(unsigned)tiles, LH_THREADS, 0, ctx->stream>>>(f, n, tile_last);
    FMK_LAUNCH_CHECK(ctx);
    k_lh_aggscan<<<1, LH_THREADS, 0, ctx->stream>>>(tile_last, tiles);
    FMK_LAUNCH_CHECK(ctx);
    k_lh_apply<F><<<(unsigned)tiles, LH_THREADS, 0, ctx->stream>>>(f, n, tile_last);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

}  // namespace
