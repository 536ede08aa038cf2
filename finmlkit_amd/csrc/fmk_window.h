// fmk_window.h -- the lockstep window walk of the rolling moments (fmk_rolling.hip), the windowed order statistics (fmk_order.hip),
// the price-volume correlation (fmk_corr.hip) and the window statistics (fmk_shape.hip).
// A workgroup of BLOCK lanes owns BLOCK * OPL consecutive outputs, a lane OPL of them, BLOCK apart.  The tile reads a span of
// window - 1 + outputs elements; the window of output r of lane l of the wave whose first lane is `wave0` is the span elements
// wave0 + r * BLOCK + l + p, p = 0 .. window - 1.  All lanes walk p upwards in lockstep, so a wave reads 64 consecutive LDS words
// per step and output.  The span is staged in LDS in slabs of at most FMK_SLAB_MAX words; from each slab an output takes the part of
// its window that lies in it, slabs and positions ascending.  No atomics, no cross-lane exchange.  DESIGN.md section 7c.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include "fmk_common.h"
#define FMK_HD __host__ __device__ __forceinline__
#else
#define FMK_HD static inline
#endif

#define FMK_SLAB_MAX 4096            // LDS words per staging (32 KiB): five workgroups per CU

// the slab of a walk whose full tile holds `tile` outputs: what that tile reads, at most FMK_SLAB_MAX
FMK_HD int fmk_slab(int64_t window, int64_t tile)
{
    const int64_t span = window - 1 + tile;
    return (int)(span < FMK_SLAB_MAX ? span : FMK_SLAB_MAX);
}

#define FMK_SLAB_MAX16 2048          // the same 32 KiB in 16-byte words (fmk_corr.hip: a word holds a pair)

// fmk_slab for a walk over 16-byte words
FMK_HD int fmk_slab16(int64_t window, int64_t tile)
{
    const int64_t span = window - 1 + tile;
    return (int)(span < FMK_SLAB_MAX16 ? span : FMK_SLAB_MAX16);
}

#define FMK_SLAB_MAX32 1024          // and in 32-byte words (fmk_shape.hip: a word holds four running sums)

// fmk_slab for a walk over 32-byte words
FMK_HD int fmk_slab32(int64_t window, int64_t tile)
{
    const int64_t span = window - 1 + tile;
    return (int)(span < FMK_SLAB_MAX32 ? span : FMK_SLAB_MAX32);
}

// The steps of one wave in one slab of `len` words.  w0 = wave0 - (the slab's start in the span); with q = w0 + p, position p of
// every window of the wave is LDS word q + r * BLOCK + l, and reach = (OPL - 1) * BLOCK + 63 is the last word a wave reads at q,
// less q.  any: some position of some window of the wave lies in the slab.  Then q runs over [qlo, hb] (the steps before word 0:
// some lanes are not in the slab yet; every word checked), [fa, fb] (every word q .. q + reach lies in the slab: no lane needs a
// check) and [fb + 1, qhi] (checked); a range is empty when its end is below its start.
struct fmk_walk_steps {
    bool any;
    int qlo, hb, fa, fb, qhi;
};

FMK_HD fmk_walk_steps fmk_walk_plan(int64_t w0, int64_t window, int len, int reach)
{
    fmk_walk_steps s;
    const int64_t qa = w0 > -(int64_t)reach ? w0 : -(int64_t)reach;
    const int64_t qb = w0 + window - 1 < (int64_t)len - 1 ? w0 + window - 1 : (int64_t)len - 1;
    s.any = qa <= qb;
    s.qlo = (int)qa;
    s.qhi = (int)qb;
    s.fa = s.qlo > 0 ? s.qlo : 0;
    s.fb = s.qhi < len - 1 - reach ? s.qhi : len - 1 - reach;
    if (s.fb < s.fa) s.fb = s.fa - 1;
    s.hb = s.fa - 1 < s.qhi ? s.fa - 1 : s.qhi;
    return s;
}

#ifdef __HIPCC__
// One walk over the tile's span of `span` elements, which load(i) gives as Words; take(r, word) consumes one element of output r of
// the lane.  stage == false: the (single) slab is in LDS already.  Every lane of the workgroup comes here (barriers); lanes without
// an output read staged words and the caller drops what they take.
template <int BLOCK, int OPL, typename Word, typename Load, typename Take>
__device__ __forceinline__ void fmk_window_walk(Word *lds, int64_t span, int64_t window, int slab, bool stage, Load load, Take take)
{
    const int lane = fmk_lane();
    constexpr int REACH = (OPL - 1) * BLOCK + 63;
    for (int64_t s0 = 0; s0 < span; s0 += slab) {
        const int len = (int)(span - s0 < (int64_t)slab ? span - s0 : (int64_t)slab);
        if (stage) {
            __syncthreads();                                         // the readers of the previous slab are done
            for (int i = threadIdx.x; i < len; i += BLOCK) lds[i] = load(s0 + i);
            __syncthreads();
        }
        const fmk_walk_steps s = fmk_walk_plan((int64_t)(threadIdx.x & ~63u) - s0, window, len, REACH);
        if (!s.any) continue;
        const int hb = fmk_uniform(s.hb), fa = fmk_uniform(s.fa), fb = fmk_uniform(s.fb), qhi = fmk_uniform(s.qhi);
        auto checked = [&](int q0, int q1) {
            for (int q = q0; q <= q1; ++q) {
#pragma unroll
                for (int r = 0; r < OPL; ++r) {
                    const int i = q + r * BLOCK + lane;
                    if ((unsigned)i < (unsigned)len) take(r, lds[i]);
                }
            }
        };
        checked(fmk_uniform(s.qlo), hb);
        const Word *row = lds + lane;
#pragma unroll 4
        for (int q = fa; q <= fb; ++q) {
#pragma unroll
            for (int r = 0; r < OPL; ++r) take(r, row[q + r * BLOCK]);
        }
        checked(fb + 1, qhi);
    }
}
#endif  // __HIPCC__
