// fmk_seqboot.hip -- the sequential bootstrap of Advances in Financial Machine Learning §4.5 on label spans (the
// arithmetic that decides a bit is fmk_seqboot_rule.h).  After every draw each event's probability is proportional to its average
// uniqueness given the draws so far.  The definition is in integers, so every sum is exact and the result does not depend on how
// the work is tiled.
//
// The host compresses the axis to the J <= 2m - 1 intervals between span boundaries (fmk_sb_compress).  One workgroup of SB_THREADS
// threads per run, grid = runs.  Thread t owns the contiguous run of `ipt` intervals from t * ipt and the contiguous run of `ept`
// events from t * ept.  Per draw:
//   1. a thread sums len_j * w(c_j) over its intervals and leaves the sum before each of them in P; the workgroup's exclusive scan
//      of the threads' sums (fmk_wgscan.h) gives the thread's offset, kept per thread in LDS: P[j] + offset[owner of j] is the
//      exclusive prefix over all intervals;
//   2. a thread sums Q_i = floor((prefix at hi_i - prefix at lo_i) / L_i) over its events; a second scan gives its offset and T;
//   3. the one thread whose range [offset, offset + sum) holds the target walks the Q of its events again (it left them in the
//      run's scratch in step 2) and publishes the drawn one;
//   4. every thread adds 1 to c over its part of the drawn event's intervals.
// So c has one reader and writer per element, the thread that owns it, and the barriers of a draw are those of the two scans and
// of the two hand-overs (offsets, the drawn event).
// Layout: element k of thread t's run lies at k * SB_THREADS + t, for c, P, the lengths and the events alike ("transposed"), so
// that a wave reads consecutive addresses although every thread walks a contiguous run.  The host writes the lengths and the events
// in that layout and stores, for an event, the POSITIONS of lo and hi in it; the owner of a position is its low ten bits.
// c and P live in LDS when J <= SB_LDS_INTERVALS, else in the run's slab of a scratch block; both run the same body.  The draws of
// a call go out in launches of `draws_per_launch` draws: c persists in global memory between them (the LDS flavour loads it when a
// launch begins and stores it when it ends), so no launch grows with the number of draws and the split changes nothing.
// Barriers only, all of them in the draw loop, whose trip count is the launch's; no workgroup waits for another.
#include <vector>

#include "fmk_common.h"
#include "fmk_seqboot_rule.h"
#include "fmk_wgscan.h"

#define SB_THREADS 1024
#define SB_LOG2_THREADS 10
#define SB_LDS_ROWS 4                      // rows of SB_THREADS intervals in LDS: 12 B each, 48 KiB of the 64 KiB a kernel may declare
#define SB_LDS_INTERVALS (SB_LDS_ROWS * SB_THREADS - 1)     // ipt = J / SB_THREADS + 1 rows hold J intervals and the end of the last
#define SB_DRAWS_PER_LAUNCH 256
#define SB_BATCH 8                         // independent loads a thread keeps in flight: a run is latency bound when runs are few
#define SB_MAX_GRID ((int64_t)1 << 20)     // runs per launch

namespace {

struct SbSum : FmkScalarDpp<SbSum, uint64_t, int64_t> {
    using T = uint64_t;
    static __device__ __forceinline__ uint64_t identity() { return 0; }
    static __device__ __forceinline__ uint64_t combine(uint64_t first, uint64_t then) { return first + then; }
};

// an event in the kernel's layout: the positions of its first interval and of the one behind its last; an empty slot (lo == hi)
// has S = 0 and Q = 0: it is never drawn
struct alignas(16) SbSlot { uint32_t lo, hi, len_m1, pad; };

struct SbArgs {
    const uint32_t *len_m1;                // [ipt][SB_THREADS] interval lengths - 1
    const SbSlot *events;                  // [ept][SB_THREADS]
    int64_t m, J;
    int ipt, ept;                          // intervals / events per thread
    uint32_t *c;                           // [runs][ipt][SB_THREADS] concurrency of the draws so far
    uint64_t *P;                           // [runs][ipt][SB_THREADS], the scratch flavour only
    uint32_t *qbuf;                        // [runs][ept][SB_THREADS]: the Q of step 2, for the thread that walks in step 3
    const uint64_t *words;                 // [runs][K] or null
    uint64_t seed;
    int64_t K, k0, k1;                     // draws per run; this launch makes the draws [k0, k1)
    int64_t r0;                            // ... of the runs r0 + blockIdx.x
    int64_t *draws, *q;                    // [runs][K]; q may be null
};

struct SbPick { int64_t i; uint64_t q; uint32_t lo, hi; };

__device__ __forceinline__ uint32_t sb_at(int k, int tid) { return ((uint32_t)k << SB_LOG2_THREADS) + (uint32_t)tid; }

// the draws [k0, k1) of run r with its c and P at the given addresses
__device__ __forceinline__ void sb_draws(const SbArgs &a, int64_t r, uint32_t *__restrict__ c, uint64_t *__restrict__ P,
                                         uint32_t *__restrict__ qbuf, uint64_t *s_scan, uint64_t *s_off, SbPick *s_pick)
{
    const int tid = threadIdx.x;
    const uint32_t *__restrict__ len_m1 = a.len_m1;
    const SbSlot *__restrict__ events = a.events;
    const int64_t j0 = (int64_t)tid * a.ipt < a.J ? (int64_t)tid * a.ipt : a.J;
    const int nj = (int)(j0 + a.ipt < a.J ? a.ipt : a.J - j0);            // this thread's intervals [j0, j0 + nj)
    const int ept = a.ept;
    if (tid == 0) { s_pick->i = 0; s_pick->q = 0; s_pick->lo = s_pick->hi = 0; }     // ordered before step 3 by the scans' barriers
    for (int64_t k = a.k0; k < a.k1; ++k) {
        // ---- 1: P = the sums before this thread's intervals, s_off = the sum before the thread
        uint64_t s = 0;
        int kk = 0;
        for (; kk + SB_BATCH <= nj; kk += SB_BATCH) {
            uint32_t cv[SB_BATCH], lv[SB_BATCH];
#pragma unroll
            for (int u = 0; u < SB_BATCH; ++u) { cv[u] = c[sb_at(kk + u, tid)]; lv[u] = len_m1[sb_at(kk + u, tid)]; }
#pragma unroll
            for (int u = 0; u < SB_BATCH; ++u) {
                P[sb_at(kk + u, tid)] = s;
                s += ((uint64_t)lv[u] + 1u) * fmk_sb_w(cv[u]);
            }
        }
        for (; kk < nj; ++kk) {
            P[sb_at(kk, tid)] = s;
            s += ((uint64_t)len_m1[sb_at(kk, tid)] + 1u) * fmk_sb_w(c[sb_at(kk, tid)]);
        }
        if (nj < a.ipt) P[sb_at(nj, tid)] = s;                            // the end of a short run: interval J lies in one of them
        uint64_t totP;
        const uint64_t offP = fmk_wg_exclusive<SbSum, SB_THREADS / 64>(s, s_scan, &totP);
        s_off[tid] = offP;
        __syncthreads();
        // ---- 2: the sum of this thread's Q_i, its offset and the total
        uint64_t sq = 0;
        for (kk = 0; kk < ept; kk += SB_BATCH) {
            SbSlot e[SB_BATCH];
            uint64_t ph[SB_BATCH], pl[SB_BATCH];
#pragma unroll
            for (int u = 0; u < SB_BATCH; ++u) e[u] = kk + u < ept ? events[sb_at(kk + u, tid)] : SbSlot{0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < SB_BATCH; ++u) { ph[u] = P[e[u].hi]; pl[u] = P[e[u].lo]; }
#pragma unroll
            for (int u = 0; u < SB_BATCH; ++u) {
                const uint64_t S = (ph[u] + s_off[e[u].hi & (SB_THREADS - 1)]) - (pl[u] + s_off[e[u].lo & (SB_THREADS - 1)]);
                const uint64_t qi = fmk_sb_q(S, (uint64_t)e[u].len_m1 + 1u);                  // at most 2^30
                if (kk + u < ept) qbuf[sb_at(kk + u, tid)] = (uint32_t)qi;
                sq += qi;
            }
        }
        uint64_t T;
        const uint64_t offQ = fmk_wg_exclusive<SbSum, SB_THREADS / 64>(sq, s_scan, &T);
        const uint64_t idx = (uint64_t)r * (uint64_t)a.K + (uint64_t)k;
        const uint64_t word = a.words ? a.words[idx] : fmk_sb_word(a.seed, idx);
        const uint64_t target = fmk_sb_target(word, T);
        // ---- 3: the smallest i with Q_0 + .. + Q_i > target lies in exactly one thread's run (T > 0, target < T)
        if (offQ <= target && target - offQ < sq) {
            uint64_t acc = offQ, q_at = 0;
            int k_at = 0;
#pragma unroll 8
            for (kk = 0; kk < ept; ++kk) {
                const uint64_t qi = qbuf[sb_at(kk, tid)];                                    // this thread's own stores of step 2
                if (acc <= target && target - acc < qi) { k_at = kk; q_at = qi; }
                acc += qi;
            }
            const SbSlot e = events[sb_at(k_at, tid)];
            s_pick->i = (int64_t)tid * ept + k_at; s_pick->q = q_at; s_pick->lo = e.lo; s_pick->hi = e.hi;
        }
        __syncthreads();
        const SbPick pick = *s_pick;
        if (tid == 0) {
            a.draws[idx] = pick.i;
            if (a.q) a.q[idx] = (int64_t)pick.q;
        }
        // ---- 4: the drawn span covers its intervals once more; a thread changes its own c alone
        const int64_t lo_j = (int64_t)(pick.lo & (SB_THREADS - 1)) * a.ipt + (pick.lo >> SB_LOG2_THREADS);
        const int64_t hi_j = (int64_t)(pick.hi & (SB_THREADS - 1)) * a.ipt + (pick.hi >> SB_LOG2_THREADS);
        const int64_t ka = (lo_j > j0 ? lo_j : j0) - j0, kb = (hi_j < j0 + nj ? hi_j : j0 + nj) - j0;      // ka < kb: both in [0, nj]
        for (int64_t kq = ka; kq < kb; ++kq) c[sb_at((int)kq, tid)] += 1u;
    }
}

template <bool LDS>
__global__ __launch_bounds__(SB_THREADS) void k_seqboot(const SbArgs a)
{
    __shared__ uint64_t s_scan[SB_THREADS / 64];
    __shared__ uint64_t s_off[SB_THREADS];
    __shared__ SbPick s_pick;
    const int64_t r = a.r0 + blockIdx.x;
    const size_t slab = (size_t)a.ipt << SB_LOG2_THREADS;
    uint32_t *gc = a.c + (size_t)r * slab;
    uint32_t *qb = a.qbuf + (size_t)r * ((size_t)a.ept << SB_LOG2_THREADS);
    if constexpr (LDS) {
        __shared__ uint64_t s_P[SB_LDS_ROWS * SB_THREADS];
        __shared__ uint32_t s_c[SB_LDS_ROWS * SB_THREADS];
        for (int kk = 0; kk < a.ipt; ++kk) s_c[sb_at(kk, threadIdx.x)] = gc[sb_at(kk, threadIdx.x)];      // a thread's own column
        sb_draws(a, r, s_c, s_P, qb, s_scan, s_off, &s_pick);
        for (int kk = 0; kk < a.ipt; ++kk) gc[sb_at(kk, threadIdx.x)] = s_c[sb_at(kk, threadIdx.x)];
    } else {
        sb_draws(a, r, gc, a.P + (size_t)r * slab, qb, s_scan, s_off, &s_pick);
    }
}

int sb_check_sizes(fmk_ctx *ctx, int64_t m, int64_t n, int64_t K, int64_t R, int64_t dpl, const void *draws)
{
    if (m < 1 || m > FMK_SB_MAX_EVENTS)
        return fmk_set_error(ctx, FMK_E_ARG, "sequential_bootstrap: n_events must be between 1 and 2^31 - 1.");
    if (K < 1 || K > FMK_SB_MAX_DRAWS) return fmk_set_error(ctx, FMK_E_ARG, "sequential_bootstrap: n_draws must be between 1 and 2^24.");
    if (R < 1 || R > FMK_SB_MAX_WORDS / K)
        return fmk_set_error(ctx, FMK_E_ARG, "sequential_bootstrap: n_runs must be at least 1 and n_runs * n_draws at most 2^40.");
    if (n < 0 || n > FMK_SB_MAX_AXIS) return fmk_set_error(ctx, FMK_E_ARG, "sequential_bootstrap: n must be between 0 and 2^32.");
    if (dpl < 0) return fmk_set_error(ctx, FMK_E_ARG, "sequential_bootstrap: draws_per_launch must not be negative.");
    if (!draws) return fmk_set_error(ctx, FMK_E_ARG, "sequential_bootstrap: a null output");
    return FMK_OK;
}

// events and touches are HOST arrays; words, draws and q device arrays
int sb_run(fmk_ctx *ctx, const int64_t *ev, const int64_t *touch, int64_t m, int64_t n, int64_t K, int64_t R, uint64_t seed,
           const uint64_t *d_words, int64_t dpl, int64_t *d_draws, int64_t *d_q)
{
    long long bad = 0;
    for (int64_t i = 0; i < m; ++i) bad += ev[i] < 0 || touch[i] < ev[i] || touch[i] >= n;
    if (bad)
        return fmk_set_error(ctx, FMK_E_ARG, "sequential_bootstrap: %lld events outside 0 <= event_idx <= touch_idx < %lld", bad,
                             (long long)n);
    std::vector<uint32_t> len_m1;
    std::vector<FmkSbEvent> events;
    fmk_sb_compress(ev, touch, m, len_m1, events);
    const int64_t J = (int64_t)len_m1.size();
    const bool lds = J <= SB_LDS_INTERVALS;
    if (dpl == 0) dpl = SB_DRAWS_PER_LAUNCH;
    // the kernel's layout: ipt rows of SB_THREADS intervals (J < ipt * SB_THREADS: the end of the last interval has a place too),
    // ept rows of events; positions are 32-bit
    const int64_t ipt = J / SB_THREADS + 1, ept = fmk_ceil_div(m, SB_THREADS);
    const size_t slab = (size_t)ipt * SB_THREADS, ev_slots = (size_t)ept * SB_THREADS;
    if (slab > ((size_t)1 << 32))
        return fmk_set_error(ctx, FMK_E_NOMEM, "sequential_bootstrap: %lld intervals are more than the kernel's 32-bit positions hold",
                             (long long)J);
    auto pos = [ipt](uint32_t j) { return (uint32_t)(((uint64_t)(j % ipt) << SB_LOG2_THREADS) + (uint64_t)(j / ipt)); };
    std::vector<uint32_t> len_t(slab, 0u);
    for (int64_t j = 0; j < J; ++j) len_t[pos((uint32_t)j)] = len_m1[(size_t)j];
    std::vector<SbSlot> ev_t(ev_slots, SbSlot{0, 0, 0, 0});
    for (int64_t i = 0; i < m; ++i) {
        const FmkSbEvent e = events[(size_t)i];
        ev_t[(size_t)(i % ept) * SB_THREADS + (size_t)(i / ept)] = SbSlot{pos(e.lo), pos(e.hi), e.len_m1, 0};
    }

    FMK_HIP(ctx, hipSetDevice(ctx->device));
    // one block: events | lengths | c of every run | the Q of every run | P of every run (the scratch flavour); every part a
    // multiple of 4 KiB
    const size_t b_ev = ev_slots * sizeof(SbSlot), b_len = slab * 4, b_c = (size_t)R * slab * 4, b_q = (size_t)R * ev_slots * 4;
    const size_t b_p = lds ? 0 : (size_t)R * slab * 8;
    void *blk;
    FMK_TRY(fmk_alloc(ctx, b_ev + b_len + b_c + b_q + b_p, &blk));
    char *base = (char *)blk;
    int rc = fmk_h2d(ctx, base, ev_t.data(), b_ev);
    if (rc == FMK_OK) rc = fmk_h2d(ctx, base + b_ev, len_t.data(), b_len);
    if (rc == FMK_OK) rc = fmk_memset(ctx, base + b_ev + b_len, 0, b_c);
    if (rc == FMK_OK) {
        SbArgs a;
        a.events = (const SbSlot *)base;
        a.len_m1 = (const uint32_t *)(base + b_ev);
        a.m = m; a.J = J;
        a.ipt = (int)ipt; a.ept = (int)ept;
        a.c = (uint32_t *)(base + b_ev + b_len);
        a.qbuf = (uint32_t *)(base + b_ev + b_len + b_c);
        a.P = lds ? nullptr : (uint64_t *)(base + b_ev + b_len + b_c + b_q);
        a.words = d_words; a.seed = seed; a.K = K;
        a.draws = d_draws; a.q = d_q;
        for (int64_t k0 = 0; k0 < K && rc == FMK_OK; k0 += dpl) {
            a.k0 = k0;
            a.k1 = k0 + dpl < K ? k0 + dpl : K;
            for (int64_t r0 = 0; r0 < R; r0 += SB_MAX_GRID) {
                a.r0 = r0;
                const unsigned grid = (unsigned)(R - r0 < SB_MAX_GRID ? R - r0 : SB_MAX_GRID);
                if (lds) k_seqboot<true><<<grid, SB_THREADS, 0, ctx->stream>>>(a);
                else k_seqboot<false><<<grid, SB_THREADS, 0, ctx->stream>>>(a);
            }
            if (hipGetLastError() != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "sequential_bootstrap: launch");
        }
    }
    (void)fmk_free(ctx, blk);                                // stream-ordered: the launches above are queued before it
    return rc;
}

}  // namespace

extern "C" int fmk_seqboot_geometry(int64_t *out3)
{
    out3[0] = SB_THREADS;
    out3[1] = SB_LDS_INTERVALS;
    out3[2] = SB_DRAWS_PER_LAUNCH;
    return FMK_OK;
}

extern "C" int fmk_sequential_bootstrap_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, int64_t n_events,
                                            int64_t n, int64_t n_draws, int64_t n_runs, uint64_t seed, const uint64_t *d_words,
                                            int64_t draws_per_launch, int64_t *d_draws, int64_t *d_q)
{
    FMK_TRY(sb_check_sizes(ctx, n_events, n, n_draws, n_runs, draws_per_launch, d_draws));
    // the compression runs on the host: the two index arrays come back (16 bytes per event, nothing of the tape)
    std::vector<int64_t> ev((size_t)n_events), touch((size_t)n_events);
    FMK_TRY(fmk_d2h(ctx, ev.data(), d_event_idx, (size_t)n_events * 8));
    FMK_TRY(fmk_d2h(ctx, touch.data(), d_touch_idx, (size_t)n_events * 8));
    return sb_run(ctx, ev.data(), touch.data(), n_events, n, n_draws, n_runs, seed, d_words, draws_per_launch, d_draws, d_q);
}

extern "C" int fmk_sequential_bootstrap(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, int64_t n_events, int64_t n,
                                        int64_t n_draws, int64_t n_runs, uint64_t seed, const uint64_t *words,
                                        int64_t draws_per_launch, int64_t *draws, int64_t *q)
{
    FMK_TRY(sb_check_sizes(ctx, n_events, n, n_draws, n_runs, draws_per_launch, draws));
    const size_t nw = (size_t)n_runs * (size_t)n_draws * 8;
    void *blk;
    FMK_TRY(fmk_alloc(ctx, nw * 3, &blk));                   // words | draws | q
    uint64_t *d_words = (uint64_t *)blk;
    int64_t *d_draws = (int64_t *)((char *)blk + nw), *d_q = (int64_t *)((char *)blk + 2 * nw);
    int rc = words ? fmk_h2d(ctx, d_words, words, nw) : FMK_OK;
    if (rc == FMK_OK)
        rc = sb_run(ctx, event_idx, touch_idx, n_events, n, n_draws, n_runs, seed, words ? d_words : nullptr, draws_per_launch, d_draws,
                    q ? d_q : nullptr);
    if (rc == FMK_OK) rc = fmk_d2h(ctx, draws, d_draws, nw);
    if (rc == FMK_OK && q) rc = fmk_d2h(ctx, q, d_q, nw);
    if (rc != FMK_OK) (void)hipStreamSynchronize(ctx->stream);   // nothing of the call is left in flight behind a failure
    (void)fmk_free(ctx, blk);
    return rc;
}
