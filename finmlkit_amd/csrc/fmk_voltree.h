// fmk_voltree.h -- the tree of jump tables behind the three table tiers of the volume bar indexer (fmk_volume.hip: vol_run and
// vol_global_tables, fmk_volume_exact.h: vx_run).
//
// A tier's level-0 kernel leaves, for each of the first W ticks of every block of span0 ticks (W >= the longest bar, so the chain of
// closes enters every block through one of them), a ROW: the tick e at which the chain that enters the block there leaves it
// (VOL_END: it ends inside) and the number c of closes it makes inside.  From there on the tiers are one algorithm:
//   level k  composes `radix` blocks of level k - 1 over the W entry ticks of the first of them:  e = E_last[.. E_2nd[E_1st[i]]],
//            c = the sum of the counts on the way.  O(N W / (span0 radix^k)) work; the top level is one block.
//   descent  the top block's entry is the first close and its output slot is 1; every block hands its (entry, slot) to its first
//            child, and to each further child the exit and the count of the child before it.
// Afterwards every level-0 block knows where the chain enters it and where its closes go, and the tier's emit kernel writes them.
// Radix 16 (VOL_RADIX): composing two at a time wrote and re-read a table of N / 2^k entries at every one of ~20 levels (24 GB per
// 1e9 ticks, 4.2 of the indexer's 12.1 ms); measured at 1e9 ticks, radix 2 / 4 / 8 / 16 / 32 -> 11.6 / 9.5 / 8.9 / 8.7 / 8.6 ms for
// the whole indexer.
//
// The first part is plain C++ (tools/voltree_check.cpp runs it on the host): the plan of the levels and its memory, one row's
// composition, one block's hand-down, the packed level-0 word of the exact-sum tier.  The kernels and the host driver below are
// thin wrappers over it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include "fmk_common.h"
#define FMK_HD __host__ __device__ __forceinline__
#else
#define FMK_HD static inline
#endif

#define VOL_END 0xFFFFFFFFu
#define VOL_RADIX 16                    // blocks composed per table level
#define VOL_MAX_LEVELS 32               // radix >= 2 and fewer than 2^31 blocks

// status word bits of the table tiers
#define VOL_ST_OVERFLOW 1   // a bar is longer than the W ticks the tables span
#define VOL_ST_BAD 2        // negative / NaN volume
#define VOL_ST_INEXACT 4    // an amount that is not a multiple of 2^-20 below 2^20: sums are not exact in float64

// The levels of one call and where their arrays lie.  Level k has nblk[k] blocks of span[k] ticks and, per block, W table rows
// (E, C) and one (ent, off) pair.  packed0: level 0 is ONE array of packed words (vol_unpack0) in E[0]; C[0] keeps its room.
struct VolTree {
    int K, radix;                       // levels above level 0; blocks composed per level
    bool packed0;
    int64_t W;
    int64_t nblk[VOL_MAX_LEVELS], span[VOL_MAX_LEVELS];
    size_t tbl, ents;                   // words of all E tables (as many again for C); (ent, off) pairs of all levels
    uint32_t *E[VOL_MAX_LEVELS], *C[VOL_MAX_LEVELS], *ent[VOL_MAX_LEVELS];
    int64_t *off[VOL_MAX_LEVELS];
};

FMK_HD VolTree vol_tree_plan(int64_t nblk0, int64_t span0, int64_t W, int radix, bool packed0 = false)
{
    VolTree t;
    t.radix = radix; t.packed0 = packed0; t.W = W;
    t.nblk[0] = nblk0;
    t.span[0] = span0;
    int K = 0;
    while (t.nblk[K] > 1) { t.nblk[K + 1] = (t.nblk[K] + radix - 1) / radix; t.span[K + 1] = t.span[K] * radix; ++K; }
    t.K = K;
    t.tbl = t.ents = 0;
    for (int k = 0; k <= t.K; ++k) { t.tbl += (size_t)t.nblk[k] * (size_t)W; t.ents += (size_t)t.nblk[k]; }
    for (int k = 0; k < VOL_MAX_LEVELS; ++k) { t.E[k] = t.C[k] = t.ent[k] = nullptr; t.off[k] = nullptr; }
    return t;
}
// bytes of the tree's region: E tables, C tables, off (int64), ent
FMK_HD size_t vol_tree_bytes(const VolTree &t) { return 2 * t.tbl * 4 + t.ents * (8 + 4); }
// base: 8-byte aligned, vol_tree_bytes(t) bytes
FMK_HD void vol_tree_bind(VolTree &t, void *base)
{
    uint32_t *Eall = (uint32_t *)base, *Call = Eall + t.tbl;
    int64_t *offall = (int64_t *)(Call + t.tbl);
    uint32_t *entall = (uint32_t *)(offall + t.ents);
    size_t to = 0, eo = 0;
    for (int k = 0; k <= t.K; ++k) {
        t.E[k] = Eall + to; t.C[k] = Call + to; to += (size_t)t.nblk[k] * (size_t)t.W;
        t.ent[k] = entall + eo; t.off[k] = offall + eo; eo += (size_t)t.nblk[k];
    }
}

struct VolRow { uint32_t e, c; };       // exit tick (absolute; VOL_END: none), closes inside

// The packed level-0 word of the exact-sum tier (k_vx_level0): the count in the high 16 bits, the exit as an offset into the next
// block's first W ticks (0xFFFF: none) in the low ones.  (Two 32-bit arrays made that table 4.8 B/tick written and read again.)
FMK_HD VolRow vol_unpack0(uint32_t w, int64_t block, int64_t span)
{
    return VolRow{(w & 0xFFFFu) == 0xFFFFu ? VOL_END : (uint32_t)((block + 1) * span + (w & 0xFFFFu)), w >> 16};
}

template <bool PACKED>
FMK_HD VolRow vol_tree_row(const uint32_t *E, const uint32_t *C, int64_t block, int64_t i, int64_t W, int64_t span)
{
    if constexpr (PACKED) return vol_unpack0(E[block * W + i], block, span);
    else return VolRow{E[block * W + i], C[block * W + i]};
}

// Row i of block b of a level from the tables (Ep, Cp) of the level below (nblk_prev blocks of span_prev ticks).  A chain that does
// not enter the next child within its first W ticks (a bar longer than W) has no row: *overflow, and the row ends the chain.
template <bool PACKED>
FMK_HD VolRow vol_tree_compose(const uint32_t *Ep, const uint32_t *Cp, int64_t nblk_prev, int64_t span_prev, int64_t W, int radix,
                               int64_t b, int64_t i, bool *overflow)
{
    const int64_t c0 = (int64_t)radix * b;
    VolRow r = vol_tree_row<PACKED>(Ep, Cp, c0, i, W, span_prev);
    for (int j = 1; j < radix; ++j) {
        const int64_t child = c0 + j;
        if (r.e == VOL_END || child >= nblk_prev) break;
        const int64_t i2 = (int64_t)r.e - child * span_prev;
        if (i2 < 0 || i2 >= W) { *overflow = true; r.e = VOL_END; break; }
        const VolRow next = vol_tree_row<PACKED>(Ep, Cp, child, i2, W, span_prev);
        r.e = next.e;
        r.c += next.c;
    }
    return r;
}

// Block b of a level, entered at tick e (VOL_END: the chain ended before it) with output slot o, hands every child its own pair.
// An entry outside a child's first W ticks is passed on unchanged: level k's composition reported that bar (overflow) already.
template <bool PACKED>
FMK_HD void vol_tree_hand_down(uint32_t e, int64_t o, const uint32_t *Ep, const uint32_t *Cp, int64_t nblk_prev, int64_t span_prev,
                               int64_t W, int radix, int64_t b, uint32_t *ent_p, int64_t *off_p)
{
    const int64_t c0 = (int64_t)radix * b;
    ent_p[c0] = e;
    off_p[c0] = o;
    for (int j = 1; j < radix; ++j) {
        const int64_t child = c0 + j;
        if (child >= nblk_prev) break;
        if (e != VOL_END) {
            const int64_t i = (int64_t)e - (child - 1) * span_prev;
            if (i >= 0 && i < W) {
                const VolRow r = vol_tree_row<PACKED>(Ep, Cp, child - 1, i, W, span_prev);
                e = r.e;
                o += r.c;
            }
        }
        ent_p[child] = e;
        off_p[child] = o;
    }
}

#ifdef __HIPCC__
__device__ __forceinline__ void vol_flag(int *status, int bit)     // one atomic per kernel, not per wave
{
    if (!(__atomic_load_n(status, __ATOMIC_RELAXED) & bit)) atomicOr(status, bit);
}

// One thread per (block, row), W any number: workgroup g serves 256 rows of block g / chunks, chunks = ceil(W / 256).  Block-major,
// so that the workgroups of one block run together and the child tables they all gather from are fetched once: with the block as
// the fast dimension of a 2-D grid the 2048-row tables took 0.85 ms more per 1e9 ticks (10.99 against 10.14 ms for the call).
// nblk * chunks is about N W / (span0 radix 256): far below 2^31 workgroups.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_vol_tree_up(int W, unsigned chunks, const uint32_t *__restrict__ Ep,
                                                     const uint32_t *__restrict__ Cp, int64_t nblk_prev, int64_t span_prev,
                                                     uint32_t *__restrict__ Ek, uint32_t *__restrict__ Ck, int64_t nblk,
                                                     int *__restrict__ status, int radix)
{
    const int64_t b = blockIdx.x / chunks;
    const int i = (int)((blockIdx.x % chunks) * 256 + threadIdx.x);
    if (i >= W || b >= nblk) return;
    bool overflow = false;
    const VolRow r = vol_tree_compose<PACKED>(Ep, Cp, nblk_prev, span_prev, W, radix, b, i, &overflow);
    if (overflow) vol_flag(status, VOL_ST_OVERFLOW);
    Ek[b * W + i] = r.e;
    Ck[b * W + i] = r.c;
}

// one thread per block of level k
template <bool PACKED>
__global__ __launch_bounds__(256) void k_vol_tree_down(int W, const uint32_t *__restrict__ ent_k, const int64_t *__restrict__ off_k,
                                                       int64_t nblk_k, int64_t span_prev, const uint32_t *__restrict__ Ep,
                                                       const uint32_t *__restrict__ Cp, int64_t nblk_prev,
                                                       uint32_t *__restrict__ ent_p, int64_t *__restrict__ off_p, int radix)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblk_k) return;
    vol_tree_hand_down<PACKED>(ent_k[b], off_k[b], Ep, Cp, nblk_prev, span_prev, W, radix, b, ent_p, off_p);
}

// ---- the host driver, in the three phases between which the tiers differ.  The caller has bound the tree and queued its level 0.

// Phase 1: queue the level-ups.  A bar beyond W sets VOL_ST_OVERFLOW in *d_status.
static int vol_tree_up(fmk_ctx *ctx, const VolTree &t, int *d_status)
{
    for (int k = 1; k <= t.K; ++k) {
        const unsigned chunks = (unsigned)fmk_ceil_div(t.W, 256), grid = (unsigned)t.nblk[k] * chunks;
        if (k == 1 && t.packed0)
            k_vol_tree_up<true><<<grid, 256, 0, ctx->stream>>>((int)t.W, chunks, t.E[0], nullptr, t.nblk[0], t.span[0], t.E[1], t.C[1],
                                                               t.nblk[1], d_status, t.radix);
        else
            k_vol_tree_up<false><<<grid, 256, 0, ctx->stream>>>((int)t.W, chunks, t.E[k - 1], t.C[k - 1], t.nblk[k - 1], t.span[k - 1],
                                                                t.E[k], t.C[k], t.nblk[k], d_status, t.radix);
        FMK_LAUNCH_CHECK(ctx);
    }
    return FMK_OK;
}

// Phase 2: *closes = the closes behind the first one, `root` (VOL_END: no close at all, and nothing is read).  One host wait; with
// d_status the status word comes back in the same batch.  Returns 1 when the first bar is longer than W: the top block has no row.
static int vol_tree_closes(fmk_ctx *ctx, const VolTree &t, uint32_t root, int64_t *closes, const int *d_status = nullptr,
                           int *status = nullptr)
{
    *closes = 0;
    if (root == VOL_END) return FMK_OK;
    if ((int64_t)root >= t.W) return 1;
    const bool packed = t.K == 0 && t.packed0;                      // a single block: the packed level-0 row itself
    auto &h = ctx->h_mail->vol.closes;
    hipError_t e = hipMemcpyAsync(&h.count, (packed ? t.E[0] : t.C[t.K]) + root, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && d_status) e = hipMemcpyAsync(&h.status, d_status, 4, hipMemcpyDeviceToHost, ctx->stream);
    FMK_TRY(fmk_wait(ctx, e));
    *closes = packed ? vol_unpack0(h.count, 0, t.span[0]).c : h.count;
    if (status) *status = h.status;
    return FMK_OK;
}

// Phase 3: seed the top block with (root, slot 1) and queue the descents.  Afterwards ent[0] / off[0] hold every level-0 block's pair.
static int vol_tree_down(fmk_ctx *ctx, const VolTree &t, uint32_t root)
{
    const int64_t one = 1;
    FMK_HIP(ctx, hipMemcpyAsync(t.ent[t.K], &root, 4, hipMemcpyHostToDevice, ctx->stream));
    FMK_HIP(ctx, hipMemcpyAsync(t.off[t.K], &one, 8, hipMemcpyHostToDevice, ctx->stream));
    for (int k = t.K; k >= 1; --k) {
        const unsigned grid = (unsigned)fmk_ceil_div(t.nblk[k], 256);
        if (k == 1 && t.packed0)
            k_vol_tree_down<true><<<grid, 256, 0, ctx->stream>>>((int)t.W, t.ent[1], t.off[1], t.nblk[1], t.span[0], t.E[0], nullptr,
                                                                 t.nblk[0], t.ent[0], t.off[0], t.radix);
        else
            k_vol_tree_down<false><<<grid, 256, 0, ctx->stream>>>((int)t.W, t.ent[k], t.off[k], t.nblk[k], t.span[k - 1], t.E[k - 1],
                                                                  t.C[k - 1], t.nblk[k - 1], t.ent[k - 1], t.off[k - 1], t.radix);
        FMK_LAUNCH_CHECK(ctx);
    }
    return FMK_OK;
}
#endif  // __HIPCC__
