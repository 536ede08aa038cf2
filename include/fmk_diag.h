/* fmk_diag.h -- test and tooling entry points of finmlkit_amd.  NOT part of the drop-in C ABI (include/fmk.h) and not used by any
 * product path (the Python modules of finmlkit_amd never bind them).
 *
 *  (1) probes: built into their own library finmlkit_amd/lib/libfmk_diag.so (csrc/fmk_diag.hip), which links against libfmk_hip.so
 *      only for the context type -- bandwidth / latency calibration kernels, the host-to-device rate of the box, a generator of
 *      full-mantissa trade sizes for bench.py's second cfg-4 timing;
 *  (2) counters: what a product kernel of libfmk_hip.so did on its last call (which tier, how many bars were redone); they read
 *      internal state and therefore live in libfmk_hip.so, but are declared here, not in fmk.h.
 */
#ifndef FMK_DIAG_H
#define FMK_DIAG_H
#include "fmk.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) probes: libfmk_diag.so ---------------------------------------------------------- */
/* Read-only streaming bandwidth probe (tools/readbw.py): calibrates the HBM ceiling quoted in DESIGN.md.
 * variant 0: 16 B loads per lane, 1: 8 B loads per lane, 2: 4 B loads per lane, 3: 8 B STORES per lane (the buffer is
 * overwritten) -- the last three calibrate FETCH_SIZE / WRITE_SIZE for the access widths the reducers use
 * (tools/pmc_calibrate.py).  Not used by any product path. */
int fmk_diag_read_bandwidth(fmk_ctx *ctx, const void *d_buf, size_t bytes, int variant, int blocks_per_cu,
                            double *elapsed_ms);
/* float32 amounts with a full random 24-bit mantissa in [2^-7, 2) (sums inexact in every order, like real trade sizes): the
 * second cfg-4 timing of bench.py.  Not used by any product path. */
int fmk_diag_fill_amounts_dev(fmk_ctx *ctx, uint64_t seed, int64_t n, float *d_amount);
/* a one-thread marker kernel (k_diag_marker) in the stream: tools/cfgprof.py brackets its measured region with which = 1 / 2 */
int fmk_diag_marker_dev(fmk_ctx *ctx, int which);
/* Two columns read in lock-step (tools/placement.py): 8 B elements of d_a8 and 4 B elements of d_b4 at the same index.
 * pattern 0: flat grid-stride; 1: each wave streams `seg` contiguous elements of both, then jumps by the number of waves
 * (the one-wave-per-bar walk of the reducers); 2: as 1, d_a8 only; 3: as 1, up to 16 rows of both columns requested before any is used.  Not used by any product path. */
int fmk_diag_read_two_streams(fmk_ctx *ctx, const void *d_a8, const void *d_b4, int64_t n, int pattern, int seg,
                              int blocks_per_cu, double *elapsed_ms);
/* Dependent-access latency of one wave (tools/hoplat.py): `hops` hops of `loads` coalesced 512 B rows, the next address
 * depending on the data read; shader cycles per hop.  Not used by any product path. */
int fmk_diag_hop_latency(fmk_ctx *ctx, const void *d_buf, int64_t n, int64_t stride, int loads, int hops,
                         double *cycles_per_hop, double *elapsed_ms);

/* Price / amount / side read by one wave per `seg`-tick segment in 512-tick tiles with lane l owning r = 1, 2, 4 or 8 CONSECUTIVE
 * ticks (tools/ownedread.py): r = 1 is the reducers' chunk layout, the others read 16-byte vectors per lane.  Not used by any product path. */
int fmk_diag_read_owned(fmk_ctx *ctx, const double *d_price, const float *d_amount, const signed char *d_side, int64_t n, int seg,
                        int r, int blocks_per_cu, double *elapsed_ms);

/* host-to-device rate of this box for one buffer, GB/s, best of three: mode 1 = hipMemcpy from pinned memory (the link's ceiling),
 * 0 = hipMemcpy from pageable memory, 2 = fmk_h2d_columns from pageable memory */
int fmk_diag_h2d_rate(fmk_ctx *ctx, size_t bytes, int mode, double *gbps);

/* ---- (2) counters of the last call: in libfmk_hip.so -------------------------------------- */
/* Which tier the last fmk_cusum_bar_indexer[_dev] call of this process took (tests): *tier 1 = the chain walk of
 * fmk_cusum_chain.hip, 0 = the fixed point; chunks the walk opened; its status (0 done, 1 budget, 2 uncertain decision,
 * 3 non-finite return, -1 not tried).  Not used by any product path. */
int fmk_diag_cusum_last(int64_t *tier, int64_t *opened, int64_t *status);
/* Which path answered the last fmk_dollar_bar_indexer[_dev] call of this process: 0 the closed form alone (every decision certain),
 * 1 closed form + exact tier, 2 the same on a stream with increments >= threshold (block trades: the stretch walk of
 * fmk_dollar_exact.hip), 3 the serial walk.  include/fmk.h makes count (d_close_idx == NULL) and fill the two phases of ONE
 * operation, so the fill half that answers from the cache leaves the value alone: after the pair it is the path that computed
 * the closes (there is no path 4; fmk_diag_dollar_source says whether the last call was such a fill). */
int fmk_diag_dollar_last(int64_t *path);
/* The closed form behind the last fmk_dollar_bar_indexer[_dev] call of this process: *closed_form 1 the one-pass look-back kernel
 * (csrc/fmk_dollar_onepass.h), 2 the two-pass kernels (dl_run, after the one-pass declined), 0 neither (the serial walk from the
 * start, or both declined); it is the form the call COMPUTED, also where the exact tier or the serial walk then replaced its
 * closes.  *cached 1: the call was the fill half of a count-then-fill pair and copied the count call's closes (then
 * *closed_form still names the form that produced them), 0: it computed. */
int fmk_diag_dollar_source(int64_t *closed_form, int64_t *cached);
/* The ladder of the last fmk_volume_bar_indexer[_dev] call of this process (csrc/fmk_volume.hip), in the order it is climbed. */
enum fmk_vol_tier {
    FMK_VOL_TIER_NONE = -1,           /* no call yet, or the call failed before a tier answered */
    FMK_VOL_TIER_EXACT_1024 = 0,      /* exact-sum class (S, W) = (3072, 1024)  (csrc/fmk_volume_exact.h) */
    FMK_VOL_TIER_EXACT_1536 = 1,      /* exact-sum class (2560, 1536) */
    FMK_VOL_TIER_EXACT_2048 = 2,      /* exact-sum class (4096, 2048) */
    FMK_VOL_TIER_LDS_2048 = 3,        /* the 2048-tick LDS tables, chosen by the sample's estimate */
    FMK_VOL_TIER_LDS_2048_TOTAL = 4,  /* the same tables after the total pass ("the sample misled") */
    FMK_VOL_TIER_GLOBAL = 5,          /* the global tables */
    FMK_VOL_TIER_CHAIN = 6,           /* the chain walk */
    FMK_VOL_TIER_SERIAL = 7,          /* the serial walk (fmk_threshold.hip) */
    FMK_VOL_TIER_CACHED = 8,          /* the fill half of a count-then-fill pair: the count call's closes, nothing tried */
    FMK_VOL_PASS_SAMPLE = 9,          /* never answer; in the tried mask when the pass over the first 2^19 ticks ... */
    FMK_VOL_PASS_TOTAL = 10,          /* ... or the total pass met a negative / NaN amount (code 2) */
    FMK_VOL_TIER_COUNT = 11
};
/* *tier: the fmk_vol_tier that answered.  *tried: bit (1 << t) for every tier t that was tried and DECLINED (the answering tier is
 * not in it); codes[t] (FMK_VOL_TIER_COUNT entries) its return code -- 1 next tier, 2 bad amounts, 3 a replay disagrees (vol_certify:
 * k_vol_verify finds another close than the tier listed, or more decisions are listed than the list holds; from the global tables
 * also: settling the fragile ticks would cost more than the serial walk), 4 a window does not certify -- and 0 for every other tier.
 * One serial walk has no declining tier in front of it: a count call made in the fast mode (fmk_ctx_set_fast_threshold) that left
 * uncertified decisions, filled in the default mode -- the fill reports FMK_VOL_TIER_SERIAL with an empty mask.  *est_len: the mean bar
 * length the sample pass estimated (ns * thr / sum of the first ns = min(n, 2^19) amounts), *mean_len: n * thr / total of the total
 * pass; NaN where the ladder did not compute one.  *listed: the fragile decisions the last tier that certified by replay listed on
 * the chain BEFORE the replay (0: none, or no such tier ran). */
int fmk_diag_volume_last(int64_t *tier, int64_t *tried, int64_t *codes, double *est_len, double *mean_len, int64_t *listed);
/* The last fmk_flow_bar_indexer_dev call of this process (csrc/fmk_flowbars.hip).  *rung: 0 the tables, 1 the serial walk (-1: no
 * call yet).  *code: why the tables declined -- 0 not tried (FMK_FLOWBARS_SERIAL, n beyond 2^31 - 4096) or not declined, 2 a bad amount
 * or price (negative, NaN, infinite) or a threshold outside (0, inf), 4 the tape does not certify (its sums are not exact in
 * float64), 1 a bar beyond 2^22 ticks.  *longest: the longest link the tables measured (0: not measured), *ls: log2 of the table
 * span they were built with (0: not built). */
int fmk_diag_flowbars_last(int64_t *rung, int64_t *code, int64_t *longest, int64_t *ls);
/* order-flow redo since the last call: {(bar, column) pairs redone in tick order, 512-term tiles walked, tiles added term by term,
 * pairs of column 0 .. 6 (buy / sell volume, buy / sell dollars, spread, signed volume, signed dollars)} */
int fmk_diag_dir_redo(fmk_ctx *ctx, int64_t *out10);
/* the last one-pass cfg-4 sizing call (csrc/fmk_fused.h): bars it handed to the footprint class kernels / to k_bar_dir / entries of
 * the tick-order redo list (float32 ties of the dollar columns and mean_spread) */
int fmk_diag_fused_last(fmk_ctx *ctx, int64_t *n_fp_list, int64_t *n_dir_list, int64_t *n_redo);
/* the schedule the last fmk_bars_flow_size[_defer]_dev call took: *mode 0 the two-pass schedules, 1 the one-pass kernel with the unit
 * histogram, 2 the one-pass kernel with float64 volumes (written on every call, early returns included); *fill_used_staged 1 if the
 * last footprint fill call consumed the level rows a one-pass sizing call had staged */
int fmk_diag_fused_mode(fmk_ctx *ctx, int64_t *mode, int64_t *fill_used_staged);
/* compute units of the context's device (the one-pass gate of cfg 4 counts bars per CU) */
int fmk_diag_n_cu(fmk_ctx *ctx, int64_t *n_cu);
/* the device's exp (csrc/fmk_exp.h: glibc's, restated) of n doubles on the device -- tests compare it with the host's exp() */
int fmk_diag_exp_dev(fmk_ctx *ctx, const double *d_x, int64_t n, double *d_out);
/* bars of the last fmk_comp_bar_footprints_fill_median_dev call whose median took the generic selection (bracket miss) */
int fmk_diag_fp_median_fallbacks(fmk_ctx *ctx, int64_t *count);
/* ... and into how many LATER segments that walk split the two sides' chains (0: each side walked in one piece); a segment
 * starts at a chunk boundary from which the side's state provably does not depend on earlier ticks (k_cc_sync).  *rate: the
 * estimate the tier was chosen by (512-tick sub-blocks per chunk and side of the leading chunks with a certain close; -1: none). */
int fmk_diag_cusum_segments(int64_t *segments, double *rate);
/* last CUSUM call: 1 if the one-pass form (csrc/fmk_cusum_onepass.h) answered, its fix-up launches, the chunks that had not merged
   within the first launch's limit, the number of chunks */
int fmk_diag_cusum_onepass(int64_t *used, int64_t *fix_launches, int64_t *pending_first, int64_t *chunks);
/* the last fmk_triple_barrier[_dev] call on this context: {schedule (0 every tick walked, 1 the block tables), events, events skipped (no tick in
 * their window), blocks opened by the table schedule, ticks walked}; waits for the context's stream */
int fmk_diag_label_last(fmk_ctx *ctx, int64_t *out5);
/* the context's last fmk_comp_bar_ohlcv[_grid]_dev / fmk_time_bars_ohlcv[_grid]_dev call: the kernel launches that read the tape's
 * int32 price grid (0: every launch read the float64 price column; the pipelined time-bar step makes two) */
int fmk_diag_ohlcv_grid_last(fmk_ctx *ctx, int64_t *launches);
/* last fmk_cusum_filter[_dev] call of this process: the form that answered (0 pass A + the wave-per-chunk fix-up, 1 the
 * lane-per-chunk re-walk took over), launches after pass A (fix-ups and re-walks), the chunks that had not merged within the first
 * fix-up launch's limit, the number of chunks */
int fmk_diag_cusum_filter_last(int64_t *form, int64_t *fix_launches, int64_t *pending_first, int64_t *chunks);
/* the last fmk_cusum_test_{rolling,developing}[_dev] call on this context: {outputs computed, (t, n) pairs walked, slabs one tile's
 * span took (> 1: the window did not fit one LDS staging), quotients formed (the pairs that passed den > 1e-16; there is no
 * screening: one exact quotient per such pair), slab elements, workgroups}; waits for the context's stream */
int fmk_diag_cusum_test_last(fmk_ctx *ctx, int64_t *out6);
/* d_out[i] = sqrt(d_in[i]) as the device's float64 sqrt rounds it (the one fmk_break.hip uses; tests compare it with the host's) */
int fmk_diag_device_sqrt(fmk_ctx *ctx, const double *d_in, int64_t n, double *d_out);
/* the first-pass schedule fmk_comp_bar_ohlcv_dev / fmk_time_bars_ohlcv_dev (time_bar_fused = 1) would take for n ticks in n_bars bars
 * on a device of n_cu compute units (csrc/fmk_ohlcv.hip: ohlcv_plan; pipe_min_stage: what FMK_TB_PIPE_MIN_STAGE holds, default 4096).
 * Plain numbers, no context, no device.  out8 = {kind (0 wave per bar, 1 lane per bar, 2 rows, 3 the pipelined time-bar step), lane
 * tile in ticks, lanes per bar, chunk cap of the wave-per-bar kernel, grid, block size, long_min (bars of more ticks are left to the
 * later passes), bars of the pipelined step's first stage}; fields that do not apply to the kind are 0 */
int fmk_diag_ohlcv_plan(int64_t n, int64_t n_bars, int amount_is_f64, int want_median, int time_bar_fused, int n_cu,
                        int64_t pipe_min_stage, int64_t *out8);

#ifdef __cplusplus
}
#endif
#endif
