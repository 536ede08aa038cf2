// fmk_recur_core.h -- the scan core of the first-order recurrences s[t] = a * s[t-1] + b[t] with one constant a on K channels
// (fmk_recur.hip, fmk_runsum.hip; DESIGN.md sections 7e and 7f): the maps and their composition (a monoid of fmk_wgscan.h, where the
// workgroup scan and the second launch, RC_AGG_UNIT tile maps per trip, come from), the 8-element loads and stores, the seed sum and
// the three launches.  A specification (see fmk_recur.hip) says what the elements are.
#pragma once
#include <math.h>

#include "fmk_common.h"
#include "fmk_dpp.h"
#include "fmk_wgscan.h"

#define RC_THREADS 256
#define RC_ITEMS 8                   // consecutive elements per thread: four 16-byte loads per series
#define RC_TILE (RC_THREADS * RC_ITEMS)
#define RC_AGG_UNIT RC_THREADS       // tile maps per trip of the aggregate scan

namespace {

// s -> a * s + b[k] on channel k
template <int K>
struct RcMap {
    double a;
    double b[K];
};

template <int K>
__device__ __forceinline__ RcMap<K> rc_identity()
{
    RcMap<K> m;
    m.a = 1.0;
#pragma unroll
    for (int k = 0; k < K; ++k) m.b[k] = 0.0;
    return m;
}

// f first, then g
template <int K>
__device__ __forceinline__ RcMap<K> rc_compose(const RcMap<K> &f, const RcMap<K> &g)
{
    RcMap<K> r;
    r.a = g.a * f.a;
#pragma unroll
    for (int k = 0; k < K; ++k) r.b[k] = g.a * f.b[k] + g.b[k];
    return r;
}

// the composition of RcMap<K> as a monoid of fmk_wgscan.h
template <int K>
struct RcMonoid {
    using T = RcMap<K>;
    static __device__ __forceinline__ T identity() { return rc_identity<K>(); }
    static __device__ __forceinline__ T combine(const T &first, const T &then) { return rc_compose(first, then); }
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ T dpp(const T &m)
    {
        T r;
        r.a = fmk_dpp<CTRL, ROW_MASK>(1.0, m.a);
#pragma unroll
        for (int k = 0; k < K; ++k) r.b[k] = fmk_dpp<CTRL, ROW_MASK>(0.0, m.b[k]);
        return r;
    }
};

// ---- the thread's 8 consecutive elements.  whole: every element of the workgroup's tile exists and none of them is element 0
// (uniform over the workgroup); the other tiles read element by element with range checks (0.0 for what is not there).
typedef double rc_d2 __attribute__((ext_vector_type(2), aligned(8)));          // 16-byte accesses on an 8-byte alignment promise

__device__ __forceinline__ bool rc_whole(int64_t tile, int64_t n) { return tile > 0 && (tile + 1) * RC_TILE <= n; }

__device__ __forceinline__ void rc_load8(const double *__restrict__ src, int64_t i0, int64_t n, bool whole, double (&v)[RC_ITEMS])
{
    if (whole) {
        const rc_d2 *q = (const rc_d2 *)(src + i0);
#pragma unroll
        for (int k = 0; k < RC_ITEMS / 2; ++k) { const rc_d2 t = q[k]; v[2 * k] = t.x; v[2 * k + 1] = t.y; }
    } else {
#pragma unroll
        for (int k = 0; k < RC_ITEMS; ++k) v[k] = i0 + k < n ? src[i0 + k] : 0.0;
    }
}
// src[i0 - 1]: the element in front of the thread's first (0.0 in front of element 0 and beyond the series)
__device__ __forceinline__ double rc_prev(const double *__restrict__ src, int64_t i0, int64_t n)
{
    return (i0 >= 1 && i0 - 1 < n) ? src[i0 - 1] : 0.0;
}
__device__ __forceinline__ void rc_store8(double *__restrict__ dst, int64_t i0, int64_t n, bool whole, const double (&v)[RC_ITEMS])
{
    if (whole) {
        rc_d2 *q = (rc_d2 *)(dst + i0);
#pragma unroll
        for (int k = 0; k < RC_ITEMS / 2; ++k) { rc_d2 t; t.x = v[2 * k]; t.y = v[2 * k + 1]; q[k] = t; }
    } else {
#pragma unroll
        for (int k = 0; k < RC_ITEMS; ++k)
            if (i0 + k < n) dst[i0 + k] = v[k];
    }
}

// The seed value, by the whole workgroup: the terms of 256 elements at a time go to LDS, thread 0 adds them in index order.  Every
// thread returns with the value in sv.
template <class S>
__device__ __forceinline__ void rc_seed(const S &sp, double (*stage)[RC_THREADS], double (&sv)[S::K])
{
    constexpr int K = S::K;
    double s[K];
    int64_t cnt = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    const int64_t lo = sp.seed_lo(), hi = sp.seed_hi();
    for (int64_t c0 = lo; c0 <= hi; c0 += RC_THREADS) {
        const int64_t i = c0 + threadIdx.x;
        if (i <= hi) {
            double t[K];
            sp.term(i, t);
#pragma unroll
            for (int k = 0; k < K; ++k) stage[k][threadIdx.x] = t[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = (int)(hi - c0 + 1 < RC_THREADS ? hi - c0 + 1 : RC_THREADS);
            for (int j = 0; j < m; ++j) {
                double t[K];
#pragma unroll
                for (int k = 0; k < K; ++k) t[k] = stage[k][j];
                sp.acc(s, cnt, t);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sp.fin(s, cnt);
#pragma unroll
        for (int k = 0; k < K; ++k) stage[k][0] = s[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) sv[k] = stage[k][0];
    __syncthreads();
}

// the thread's elements and what they do to a state: the identity before the seed and beyond the series, the constant sv at the seed
template <class S>
__device__ __forceinline__ RcMap<S::K> rc_thread_map(const S &sp, int64_t tile, int64_t n, const double (&sv)[S::K], typename S::In &in)
{
    constexpr int K = S::K;
    const int64_t i0 = tile * RC_TILE + (int64_t)threadIdx.x * RC_ITEMS;
    sp.load(i0, n, rc_whole(tile, n), in);
    RcMap<K> m = rc_identity<K>();
#pragma unroll
    for (int j = 0; j < RC_ITEMS; ++j) {
        const int64_t i = i0 + j;
        if (i >= n) continue;
        if (i > sp.seed) {
            double x[K];
            sp.x(in, j, i, x);
            m.a = sp.a * m.a;
#pragma unroll
            for (int k = 0; k < K; ++k) m.b[k] = sp.a * m.b[k] + sp.lin(x[k]);
        } else if (i == sp.seed) {
            m.a = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) m.b[k] = sv[k];
        }
    }
    return m;
}

__device__ __forceinline__ bool rc_has_seed(int64_t tile, int64_t seed) { return seed >= tile * RC_TILE && seed < (tile + 1) * RC_TILE; }

// first launch: the tile's map; the tile with the seed index leaves the seed value in seedv[K].  The host launches only when seed < n.
template <class S>
__global__ __launch_bounds__(RC_THREADS) void k_rc_tiles(S sp, int64_t n, RcMap<S::K> *__restrict__ tile_map, double *__restrict__ seedv)
{
    constexpr int K = S::K;
    __shared__ RcMap<K> wl[RC_THREADS / 64];
    __shared__ double stage[K][RC_THREADS];
    double sv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sv[k] = 0.0;
    if (rc_has_seed(blockIdx.x, sp.seed)) {                          // uniform over the workgroup
        rc_seed(sp, stage, sv);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) seedv[k] = sv[k];
        }
    }
    typename S::In in;
    const RcMap<K> m = rc_thread_map(sp, blockIdx.x, n, sv, in);
    RcMap<K> tot;
    (void)fmk_wg_exclusive<RcMonoid<K>, RC_THREADS / 64>(m, wl, &tot);
    if (threadIdx.x == 0) tile_map[blockIdx.x] = tot;
}

// Two optional members of a specification (fmk_runsum.hip).  NOUT > 1: emit(s, in, j, r) gives NOUT values per element, series c of
// the output lies at out + c * n.  tile_end(in, n): called by every thread of the workgroup after its elements are stored (it may
// use barriers), for what a later launch needs to know about the tile.  `in` is the thread's own S::In, the one load() filled and
// every emit() of the thread was handed, and the core does not read it: an emit() that takes it as `In &` may leave there, per
// element, what is not a float64 series (RsPrefix's 4-byte counts), and tile_end() stores it, checking i < n itself as rc_store8 does.
template <class S, class = void> struct RcNout { static constexpr int N = 1; };
template <class S> struct RcNout<S, decltype((void)S::NOUT)> { static constexpr int N = S::NOUT; };
template <class S, class = void> struct RcTileEnd { static constexpr bool has = false; };
template <class S> struct RcTileEnd<S, decltype((void)&S::tile_end)> { static constexpr bool has = true; };

// third launch: the outputs
template <class S>
__global__ __launch_bounds__(RC_THREADS) void k_rc_apply(S sp, int64_t n, const RcMap<S::K> *__restrict__ tile_pre,
                                                         const double *__restrict__ seedv, double *__restrict__ out)
{
    constexpr int K = S::K, NO = RcNout<S>::N;
    __shared__ RcMap<K> wl[RC_THREADS / 64];
    double sv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sv[k] = rc_has_seed(blockIdx.x, sp.seed) ? seedv[k] : 0.0;
    typename S::In in;
    const RcMap<K> m = rc_thread_map(sp, blockIdx.x, n, sv, in);
    RcMap<K> tot;
    const RcMap<K> ex = fmk_wg_exclusive<RcMonoid<K>, RC_THREADS / 64>(m, wl, &tot);
    const RcMap<K> pre = tile_pre[blockIdx.x];                       // applied to the zero state: its b
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = ex.a * pre.b[k] + ex.b[k];
    const int64_t i0 = (int64_t)blockIdx.x * RC_TILE + (int64_t)threadIdx.x * RC_ITEMS;
    double res[NO][RC_ITEMS];
#pragma unroll
    for (int j = 0; j < RC_ITEMS; ++j) {
        const int64_t i = i0 + j;
        if (i < sp.seed) {
#pragma unroll
            for (int c = 0; c < NO; ++c) res[c][j] = sp.before();
            continue;
        }
        if (i == sp.seed) {
#pragma unroll
            for (int k = 0; k < K; ++k) s[k] = sv[k];
        } else {
            double x[K];
            sp.x(in, j, i, x);
#pragma unroll
            for (int k = 0; k < K; ++k) s[k] = sp.step(s[k], x[k]);
        }
        if constexpr (NO == 1) {
            res[0][j] = sp.emit(s, in, j);
        } else {
            double r[NO];
            sp.emit(s, in, j, r);
#pragma unroll
            for (int c = 0; c < NO; ++c) res[c][j] = r[c];
        }
    }
#pragma unroll
    for (int c = 0; c < NO; ++c) rc_store8(out + (int64_t)c * n, i0, n, rc_whole(blockIdx.x, n), res[c]);
    if constexpr (RcTileEnd<S>::has) sp.tile_end(in, n);
}

__global__ __launch_bounds__(256) void k_rc_fill(double *out, int64_t n, double v)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = v;
}

int rc_fill(fmk_ctx *ctx, double *d_out, int64_t n, double v)
{
    k_rc_fill<<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>(d_out, n, v);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

// one recurrence over n > 0 elements on the context's stream; a series that ends before the seed is before() everywhere
template <class S>
int rc_scan(fmk_ctx *ctx, const S &sp, int64_t n, double *d_out, double before)
{
    if (sp.seed >= n) return rc_fill(ctx, d_out, n, before);
    const int64_t tiles = fmk_ceil_div(n, RC_TILE);
    void *scr;
    FMK_TRY(fmk_scratch(ctx, (size_t)tiles * sizeof(RcMap<S::K>) + S::K * sizeof(double), &scr));
    RcMap<S::K> *maps = (RcMap<S::K> *)scr;
    double *seedv = (double *)(maps + tiles);
    k_rc_tiles<S><<<(unsigned)tiles, RC_THREADS, 0, ctx->stream>>>(sp, n, maps, seedv);
    FMK_LAUNCH_CHECK(ctx);
    k_fmk_agg_scan<RcMonoid<S::K>, RC_AGG_UNIT><<<1, RC_AGG_UNIT, 0, ctx->stream>>>(maps, tiles, nullptr);
    FMK_LAUNCH_CHECK(ctx);
    k_rc_apply<S><<<(unsigned)tiles, RC_THREADS, 0, ctx->stream>>>(sp, n, maps, seedv, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

}  // namespace
