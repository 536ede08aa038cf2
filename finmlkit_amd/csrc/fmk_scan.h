// fmk_scan.h -- device-wide exclusive scan of int64 (reduce-then-scan, three launches).
//   k_scan_tile_sums : one 256-thread block per 4096-element tile -> tile total
//   k_fmk_agg_scan   : ONE 1024-thread block scans the tile totals in place (B/4096 elements), FMK_SCAN_AGG_UNIT per trip
//   k_scan_apply     : per tile: block scan of the elements + tile offset, in place
// The workgroup scan and the second launch are those of fmk_wgscan.h with the monoid ScanSum.
// Used for CSR offsets of the footprint output (B elements) -- tiny next to the tick streams.
#pragma once

#include "fmk_common.h"
#include "fmk_wgscan.h"

#define FMK_SCAN_THREADS 256
#define FMK_SCAN_ROWS 16
#define FMK_SCAN_TILE (FMK_SCAN_THREADS * FMK_SCAN_ROWS)
#define FMK_SCAN_AGG_UNIT 1024       // tile totals per trip of the aggregate scan

namespace {
struct ScanSum : FmkScalarDpp<ScanSum, int64_t> {
    using T = int64_t;
    static __device__ __forceinline__ int64_t identity() { return 0; }
    static __device__ __forceinline__ int64_t combine(int64_t first, int64_t then) { return first + then; }
};
}  // namespace

static __global__ __launch_bounds__(FMK_SCAN_THREADS) void k_scan_tile_sums(const int64_t *__restrict__ in, int64_t n,
                                                                     int64_t *__restrict__ tile_sum)
{
    __shared__ int64_t sw[4];
    const int64_t base = (int64_t)blockIdx.x * FMK_SCAN_TILE;
    int64_t s = 0;
#pragma unroll 4
    for (int r = 0; r < FMK_SCAN_ROWS; ++r) {
        int64_t j = base + r * FMK_SCAN_THREADS + threadIdx.x;
        if (j < n) s += in[j];
    }
    s = fmk_wave_sum(s);
    if (fmk_lane() == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

// out[j] = tile_off[tile] + exclusive prefix within the tile, one workgroup scan per row of FMK_SCAN_THREADS elements
static __global__ __launch_bounds__(FMK_SCAN_THREADS) void k_scan_apply(const int64_t *__restrict__ in, int64_t n,
                                                                 const int64_t *__restrict__ tile_off,
                                                                 int64_t *__restrict__ out)
{
    __shared__ int64_t ws[FMK_SCAN_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * FMK_SCAN_TILE;
    int64_t run = tile_off[blockIdx.x];
    for (int r = 0; r < FMK_SCAN_ROWS; ++r) {
        const int64_t j = base + r * FMK_SCAN_THREADS + threadIdx.x;
        int64_t tot;
        const int64_t ex = fmk_wg_exclusive<ScanSum, FMK_SCAN_THREADS / 64>(j < n ? in[j] : 0, ws, &tot);
        if (j < n) out[j] = run + ex;
        run += tot;
    }
}

// Exclusive scan of d_in[0..n) into d_out[0..n) (may alias); d_out[n] receives the total when
// `write_total_at_n` is set.  Enqueued on the context stream.
static inline int fmk_exclusive_scan_i64(fmk_ctx *ctx, const int64_t *d_in, int64_t *d_out, int64_t n,
                                         bool write_total_at_n)
{
    if (n <= 0) {
        if (write_total_at_n) FMK_HIP(ctx, hipMemsetAsync(d_out, 0, 8, ctx->stream));
        return FMK_OK;
    }
    const int64_t tiles = fmk_ceil_div(n, FMK_SCAN_TILE);
    void *scr;
    FMK_TRY(fmk_scratch(ctx, (size_t)tiles * 8, &scr));
    int64_t *tile = (int64_t *)scr;
    k_scan_tile_sums<<<(unsigned)tiles, FMK_SCAN_THREADS, 0, ctx->stream>>>(d_in, n, tile);
    FMK_LAUNCH_CHECK(ctx);
    k_fmk_agg_scan<ScanSum, FMK_SCAN_AGG_UNIT><<<1, FMK_SCAN_AGG_UNIT, 0, ctx->stream>>>(tile, tiles, write_total_at_n ? d_out + n : nullptr);
    FMK_LAUNCH_CHECK(ctx);
    k_scan_apply<<<(unsigned)tiles, FMK_SCAN_THREADS, 0, ctx->stream>>>(d_in, n, tile, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}
