/*
 * fmk.h -- C ABI of libfmk_hip.so, the MI355X (gfx950) tick->bar engine.
 *
 * This is the drop-in boundary for the hot path of quantscious/finmlkit
 * (tick arrays -> bar close indices -> per-bar OHLCV / order-flow / footprint,
 * plus the tick-level volatility loops).  The reference has no FFI of its own:
 * its boundary is "a module-level Python function over contiguous 1-D NumPy
 * arrays" (finmlkit/bar/logic.py, finmlkit/bar/base.py:306-850,
 * finmlkit/feature/core/{utils,volatility}.py).  Each entry point below
 * replaces exactly one of those functions; the ctypes binding a maintainer
 * would add is shown in INTEGRATION.md and shipped in finmlkit_amd/_ffi.py.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types.
 *   - every function returns an int status (FMK_OK == 0, negative = error);
 *     fmk_last_error() gives the text.  The Python shim maps the codes to
 *     the exception types the reference raises (see FMK_E_* below).
 *   - *_dev functions take DEVICE pointers and enqueue on the context's HIP
 *     stream without synchronising (fmk_ctx_sync to wait).  The functions
 *     without the suffix take HOST pointers (the NumPy drop-in): they upload,
 *     run the same kernels, download and synchronise.
 *   - `amount` columns may be float32 (the reference's preprocessed dtype,
 *     data_model.py:332-342) or float64: `amount_is_f64` selects.
 *   - close-index arrays follow the reference: n_idx = n_bars + 1 entries,
 *     entry 0 is the "open" edge (may be -1), bar i covers ticks
 *     close_idx[i]+1 .. close_idx[i+1] inclusive (base.py:364,377).
 *   - the caller owns every buffer; the library keeps no host pointer after
 *     a call returns.
 *   - there is NO CPU fallback: without a usable HIP device fmk_ctx_create
 *     fails with FMK_E_NODEVICE.
 */
#ifndef FMK_H
#define FMK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMK_OK 0
#define FMK_E_ARG (-1)      /* ValueError (base.py:332-335, utils.py:33-34, ...) */
#define FMK_E_CAPACITY (-2) /* caller buffer too small (two-phase protocol misuse) */
#define FMK_E_LEVEL (-3)    /* ValueError "Invalid price level index" (base.py:719) */
#define FMK_E_ZERODIV (-4)  /* ZeroDivisionError (base.py:536: bar without signed tick) */
#define FMK_E_NOMEM (-5)    /* MemoryError */
#define FMK_E_HIP (-6)      /* RuntimeError: HIP runtime failure, see fmk_last_error */
#define FMK_E_NODEVICE (-7) /* RuntimeError: no gfx950 device / HIP runtime unusable */
#define FMK_E_COMM (-8)     /* RuntimeError: multi-GPU rendezvous / RCCL failure or a peer that never arrived */

#define FMK_ABI_VERSION 1

typedef struct fmk_ctx fmk_ctx;

/* ---- context, memory, timing --------------------------------------------------------- */
int fmk_abi_version(void);
int fmk_device_count(int *count);
int fmk_ctx_create(int device, fmk_ctx **out);
int fmk_ctx_destroy(fmk_ctx *ctx);
int fmk_ctx_sync(fmk_ctx *ctx);
/* Release everything the context keeps between calls: scratch, the caching allocator's free blocks, the work
 * buffers of the threshold indexers (up to ~20 B/tick).  For long-lived processes; never required. */
int fmk_ctx_trim(fmk_ctx *ctx);
/* hipStream_t of the context (for interop with other HIP users, e.g. RCCL). */
void *fmk_ctx_stream(fmk_ctx *ctx);
/* Text of the last error on this context (ctx == NULL: last context-less error). */
const char *fmk_last_error(const fmk_ctx *ctx);

int fmk_alloc(fmk_ctx *ctx, size_t bytes, void **dptr);
int fmk_free(fmk_ctx *ctx, void *dptr);
int fmk_memset(fmk_ctx *ctx, void *dptr, int value, size_t bytes);
int fmk_h2d(fmk_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes); /* sync */
int fmk_d2h(fmk_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes); /* sync */
/* Several host columns to the device by one call (a TradesData frame -> HBM), complete on return.  Default: each column through
 * the runtime's own pageable copy (56 GB/s = 98 % of the pinned rate on the MI355X boxes, profiles/r03_apibench.txt);
 * FMK_UPLOAD_THREADS=n in the environment: n worker threads stage 4 MiB chunks through their own pinned double buffers and
 * streams instead (for hosts whose runtime copies pageable memory through one bounce buffer). */
int fmk_h2d_columns(fmk_ctx *ctx, int n_cols, void *const *dst_dev, const void *const *src_host, const size_t *bytes);
int fmk_d2d(fmk_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);  /* async */
int fmk_mem_info(fmk_ctx *ctx, size_t *free_bytes, size_t *total_bytes);

/* hipEvent timer on the context stream: ms between start and stop (stop syncs). */
int fmk_timer_start(fmk_ctx *ctx);
int fmk_timer_stop(fmk_ctx *ctx, double *elapsed_ms);
/* Non-blocking event pairs (per-kernel timing inside a timed region): record on the context
 * stream, read the elapsed time after fmk_ctx_sync. */
int fmk_event_create(fmk_ctx *ctx, void **event);
int fmk_event_destroy(fmk_ctx *ctx, void *event);
int fmk_event_record(fmk_ctx *ctx, void *event);
int fmk_event_elapsed(fmk_ctx *ctx, void *start, void *stop, double *elapsed_ms);
/* Per-launch timing of the dominant kernel (k_bar_ohlcv_small / k_bar_ohlcv of comp_bar_ohlcv):
 * while enabled, every fmk_comp_bar_ohlcv_dev call brackets that ONE kernel launch with a HIP event
 * pair on the context stream (ring of 256).  fmk_profile_read synchronises and returns the durations. */
/* Volume / dollar bar indexers: the parallel algorithms work on exactly computed sums and count the decisions that
 * land within the rounding drift of the reference's float64 running sum (n_uncertified).  on = 0 (default):
 * volume bars -- fragile decisions are settled by replaying their bar with the reference's sequential sum (every
 * bar starts from 0, so it can be replayed alone) and n_uncertified comes back 0: at no measurable cost for continuous
 * amounts, at (fragile ticks) x (bar length) additions for decimal lots with round thresholds; when that would cost more
 * than it, and for any uncertified dollar-bar input (the carried remainder never resets: no bar can be replayed alone),
 * the input is redone by the reference's own loop, operation for operation (one wave, 15-22 ns per tick).
 * on = 1: the parallel result is returned as is, each uncertified decision may differ from the reference by one tick
 * (resident pipelines of 1e9 ticks). */
int fmk_ctx_set_fast_threshold(fmk_ctx *ctx, int on);
/* Enqueue-only mode.  on = 0 (default): fmk_comp_bar_ohlcv_dev waits for its first kernel and reads back whether any bar was left
 * for the long-bar schedules; when none was -- streams of 1-minute bars and the like -- the ~36 launches that serve such bars are not
 * issued at all (they would exit at once, ~0.25 ms per call).  on = 1: the call never waits; everything is enqueued unconditionally
 * and it returns before its kernels have run -- for callers that overlap the call with other streams' work and must not block
 * (the sharded step of finmlkit_amd/dist.py between its halo exchange and its boundary bar).  One wait remains in this mode:
 * fmk_time_bars_ohlcv_dev takes the long-bar census from its INDEX stages (~0.1 ms into the call, while its first OHLCV launch runs:
 * the device never idles for it) instead of enqueuing the ~36 launches blindly -- 0.25 ms per sharded step (FMK_TB_PIPE_EO_CENSUS=0
 * restores the blind enqueue).  A call whose tick array is no longer than the first kernel's reach enqueues nothing more either way. */
int fmk_ctx_set_enqueue_only(fmk_ctx *ctx, int on);
/* Price grid.  on = 1 (default): fmk_comp_bar_ohlcv_grid_dev / fmk_time_bars_ohlcv_grid_dev read the int32 grid column they are
 * handed where a kernel can; on = 0: they read the float64 price column like the entry points without a grid -- the same results bit
 * for bit, for A/B timing and for tests on one object. */
int fmk_ctx_set_price_grid(fmk_ctx *ctx, int on);
int fmk_profile_enable(fmk_ctx *ctx, int on);
int fmk_profile_read(fmk_ctx *ctx, double *ms, int capacity, int *count);
int fmk_profile_count(fmk_ctx *ctx, int64_t *total);   /* launches timed since enable (> 256: the ring holds the last 256, oldest at slot total mod 256) */

/* ---- synthetic tick stream (same definition as oracle/orc_synth) ----- */
/* Writes ticks [first, first+n) of stream `seed` into device columns (any may be NULL). */
int fmk_synth_trades_dev(fmk_ctx *ctx, uint64_t seed, int64_t first, int64_t n, uint64_t gap_mod,
                         int64_t *d_ts, double *d_price, float *d_amount, int8_t *d_side);

/* ---- bar indexers: finmlkit/bar/logic.py ---------------------------------------------- */
/* _time_bar_indexer (logic.py:12-51).  fmk_time_bar_clock is pure host arithmetic: the
 * float64 clock of logic.py:30-39 as NumPy evaluates it -> edge k = first_edge + k*delta. */
int fmk_time_bar_clock(int64_t ts_first, int64_t ts_last, double interval_seconds,
                       int64_t *n_edges, int64_t *first_edge, int64_t *delta);
/* Fills d_clock[n_edges] and d_close_idx[n_edges] (searchsorted(ts, clock, 'right') - 1). */
int fmk_time_bar_indexer_dev(fmk_ctx *ctx, const int64_t *d_ts, int64_t n, int64_t first_edge,
                             int64_t delta, int64_t n_edges, int64_t *d_clock,
                             int64_t *d_close_idx);
/* Host flavour, two-phase: call with clock == NULL to get *n_edges, then with buffers. */
int fmk_time_bar_indexer(fmk_ctx *ctx, const int64_t *ts, int64_t n, double interval_seconds,
                         int64_t *clock, int64_t *close_idx, int64_t capacity, int64_t *n_edges);

/* _tick_bar_indexer (logic.py:54-84): closed form.  *n_idx receives the number of close
 * indices (first is 0); d_close_idx may be NULL to query the count only. */
int fmk_tick_bar_indexer_dev(fmk_ctx *ctx, int64_t n, int64_t threshold, int64_t *d_close_idx,
                             int64_t capacity, int64_t *n_idx);
/* _volume_bar_indexer (logic.py:87-115) and _dollar_bar_indexer (logic.py:118-149).
 * Two-phase: d_close_idx == NULL -> count only.  *n_uncertified (may be NULL) receives the
 * number of close decisions whose margin to the threshold was below the floating-point
 * reordering bound (see DESIGN.md "threshold bars"); 0 means certified bit-identical. */
int fmk_volume_bar_indexer_dev(fmk_ctx *ctx, const void *d_amount, int amount_is_f64, int64_t n,
                               double threshold, int64_t *d_close_idx, int64_t capacity,
                               int64_t *n_idx, int64_t *n_uncertified);
int fmk_dollar_bar_indexer_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount,
                               int amount_is_f64, int64_t n, double threshold,
                               int64_t *d_close_idx, int64_t capacity, int64_t *n_idx,
                               int64_t *n_uncertified);
/* Imbalance (rule 0) and run (rule 1) bars with a FIXED threshold (AFML 2.3.2; the reference has only stubs, logic.py:224-261; the
 * loops that define them: DESIGN.md "Imbalance and run bars").  Tick size by kind: 0 one per tick, 1 the amount, 2 price * amount
 * (d_price is read for kind 2 only).  d_side: -1 / 0 / +1 per tick.  ONE call does the work once: *d_close_idx receives a buffer of
 * exactly *n_idx close indices (the first is 0) from fmk_alloc, which the caller gives back with fmk_free.  Nothing is cached
 * between calls, so a column overwritten in place is read again.  Bit-equal to the loops on every input. */
int fmk_flow_bar_indexer_dev(fmk_ctx *ctx, int rule, int kind, const double *d_price, const void *d_amount,
                             int amount_is_f64, const int8_t *d_side, int64_t n, double threshold,
                             int64_t **d_close_idx, int64_t *n_idx);
/* d_out[i] = d_in[idx[i]] for int64 (close_ts = timestamps[close_indices], kit.py:66). */
int fmk_gather_i64_dev(fmk_ctx *ctx, const int64_t *d_in, int64_t n_in, const int64_t *d_idx,
                       int64_t n_idx, int64_t *d_out);

/* ---- per-bar reducers: finmlkit/bar/base.py ------------------------------------------- */
/* comp_bar_ohlcv (base.py:306-407).  d_median may be NULL (skip the order statistic). */
int fmk_comp_bar_ohlcv_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount,
                           int amount_is_f64, int64_t n, const int64_t *d_close_idx,
                           int64_t n_idx, double *d_open, double *d_high, double *d_low,
                           double *d_close, float *d_volume, double *d_vwap, int64_t *d_trades,
                           double *d_median);
/* TimeBarKit.build_ohlcv on resident columns in ONE call (kit.py:42-66 -> base.py:126-158): _time_bar_indexer
 * (logic.py:12-51) + comp_bar_ohlcv (base.py:306-407).  Results = fmk_time_bar_indexer_dev(first_edge, delta, n_edges)
 * followed by fmk_comp_bar_ohlcv_dev on its close indices, bit for bit (d_clock may be NULL, d_close_idx[n_edges] is
 * always written; ts_first / ts_last = d_ts[0] / d_ts[n-1], the two values the clock was made from).  For streams of
 * 1-minute-sized bars (mean bar length above 600 ticks, float32 amounts) the call is pipelined: the clock edges of the first eighth of
 * the bars, then OHLCV + median of those bars while the remaining edges are searched on a second stream (csrc/fmk_ohlcv.hip). */
int fmk_time_bars_ohlcv_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_price, const void *d_amount,
                            int amount_is_f64, int64_t n, int64_t ts_first, int64_t ts_last, int64_t first_edge,
                            int64_t delta, int64_t n_edges, int64_t *d_clock, int64_t *d_close_idx,
                            double *d_open, double *d_high, double *d_low, double *d_close, float *d_volume,
                            double *d_vwap, int64_t *d_trades, double *d_median);
/* ---- the price grid of a tape ---------------------------------------------------------- */
/* Exchange prices lie on a tick grid.  Where EVERY price of a tape is reproduced bit for bit from an int32 k -- form 1: (double)k * r,
 * form 2: the correctly rounded quotient k / 10^d -- the tape can carry k as a fifth column and the 1-minute OHLCV kernel reads 4 B
 * per tick of it instead of the 8 B of the price.  struct fmk_price_grid { int32_t form; int32_t d; double r; double s; } (form 0: no
 * grid; r = the double nearest 10^-d, s = 10^d; csrc/fmk_common.h, next to the decode).
 * fmk_price_grid_build_dev: one pass over the price column, once per tape (8 B read + 4 B written per tick): picks d in 0 .. 8 from
 * a sample, writes d_k[n] and certifies it by running the decode on every tick.  *grid comes back with form 0 when the tape does not
 * certify (a NaN, an infinity, -0.0, one off-grid tick, |k| >= 2^31): d_k is then of no use and the caller frees it.  Waits. */
typedef struct fmk_price_grid fmk_price_grid;
int fmk_price_grid_build_dev(fmk_ctx *ctx, const double *d_price, int64_t n, int32_t *d_k, fmk_price_grid *grid);
/* fmk_comp_bar_ohlcv_dev / fmk_time_bars_ohlcv_dev with the tape's grid (d_k and grid from fmk_price_grid_build_dev on this very
 * d_price[n]; both NULL, or form 0: no grid): the same results bit for bit.  The grid is read by the 1-minute schedule on float32
 * amounts; bars beyond 1 344 ticks, open / close and every other schedule read d_price. */
int fmk_comp_bar_ohlcv_grid_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount,
                                int amount_is_f64, int64_t n, const int64_t *d_close_idx,
                                int64_t n_idx, double *d_open, double *d_high, double *d_low,
                                double *d_close, float *d_volume, double *d_vwap, int64_t *d_trades,
                                double *d_median, const int32_t *d_k, const fmk_price_grid *grid);
int fmk_time_bars_ohlcv_grid_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_price, const void *d_amount,
                                 int amount_is_f64, int64_t n, int64_t ts_first, int64_t ts_last, int64_t first_edge,
                                 int64_t delta, int64_t n_edges, int64_t *d_clock, int64_t *d_close_idx,
                                 double *d_open, double *d_high, double *d_low, double *d_close, float *d_volume,
                                 double *d_vwap, int64_t *d_trades, double *d_median, const int32_t *d_k,
                                 const fmk_price_grid *grid);
/* The order statistic alone (np.median of the bar's trade sizes, base.py:373-403). */
int fmk_comp_bar_median_dev(fmk_ctx *ctx, const void *d_amount, int amount_is_f64, int64_t n,
                            const int64_t *d_close_idx, int64_t n_idx, double *d_median);
int fmk_comp_bar_ohlcv(fmk_ctx *ctx, const double *price, const void *amount, int amount_is_f64,
                       int64_t n, const int64_t *close_idx, int64_t n_idx, double *open_,
                       double *high, double *low, double *close_, float *volume, double *vwap,
                       int64_t *trades, double *median);

/* comp_bar_directional_features (base.py:409-546).  Outputs in the reference's tuple order.
 * d_n_zero_div (device int64, may be NULL) counts bars without a signed tick, for which the
 * reference raises ZeroDivisionError; their mean_spread is written as NaN.  The host flavour
 * returns FMK_E_ZERODIV in that case (outputs are still filled). */
typedef struct fmk_directional_out {
    int64_t *ticks_buy, *ticks_sell;
    float *volume_buy, *volume_sell, *dollars_buy, *dollars_sell;
    float *mean_spread, *max_spread;
    int64_t *cum_ticks_min, *cum_ticks_max;
    float *cum_volumes_min, *cum_volumes_max, *cum_dollars_min, *cum_dollars_max;
} fmk_directional_out;
int fmk_comp_bar_directional_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount,
                                 int amount_is_f64, int64_t n, const int64_t *d_close_idx,
                                 int64_t n_idx, const int8_t *d_side,
                                 const fmk_directional_out *d_out, int64_t *d_n_zero_div);
int fmk_comp_bar_directional(fmk_ctx *ctx, const double *price, const void *amount,
                             int amount_is_f64, int64_t n, const int64_t *close_idx,
                             int64_t n_idx, const int8_t *side, const fmk_directional_out *out);

/* comp_bar_footprints + comp_footprint_features (base.py:615-850), CSR output.
 * Phase 1: level_offsets[n_bars+1] from the bars' lows/highs (exclusive scan of
 *          int(round(high/tick)) - int(round(low/tick)) + 1); *total_levels and *max_levels
 *          are returned to the host (synchronises).
 * Phase 2: fills the flat per-level arrays (length total_levels) and the per-bar arrays. */
typedef struct fmk_footprint_out {
    int32_t *price_levels;   /* flat [total_levels] */
    float *buy_volumes, *sell_volumes;
    int32_t *buy_ticks, *sell_ticks;
    uint8_t *buy_imbalances, *sell_imbalances;   /* numpy bool */
    uint16_t *buy_imbalances_sum, *sell_imbalances_sum;   /* per bar [n_bars] */
    int32_t *cot_price_levels;
    int16_t *imb_max_run_signed;
    double *vp_skew, *vp_gini;
} fmk_footprint_out;
int fmk_comp_bar_footprints_size_dev(fmk_ctx *ctx, const double *d_bar_lows,
                                     const double *d_bar_highs, int64_t n_bars,
                                     double price_tick_size, int64_t *d_level_offsets,
                                     int64_t *total_levels, int64_t *max_levels);
int fmk_comp_bar_footprints_fill_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount,
                                     int amount_is_f64, int64_t n, const int64_t *d_close_idx,
                                     int64_t n_idx, const int8_t *d_side, double price_tick_size,
                                     const double *d_bar_lows, double imbalance_factor,
                                     const int64_t *d_level_offsets, int64_t max_levels,
                                     const fmk_footprint_out *d_out, int64_t *d_n_bad_level);
/* Host flavour, two-phase: out == NULL -> fills level_offsets only. */
int fmk_comp_bar_footprints(fmk_ctx *ctx, const double *price, const void *amount,
                            int amount_is_f64, int64_t n, const int64_t *close_idx, int64_t n_idx,
                            const int8_t *side, double price_tick_size, const double *bar_lows,
                            const double *bar_highs, double imbalance_factor,
                            int64_t *level_offsets, const fmk_footprint_out *out);

/* comp_bar_trade_size_features (base.py:549-612).  theta[n_bars] float64;
 * outputs float32[n_bars]: mean_size_rel, size_95_rel, pct_block, size_gini (NaN where the reference
 * leaves NaN: empty bar, theta == 0, zero total volume). */
int fmk_comp_bar_trade_size_dev(fmk_ctx *ctx, const void *d_amount, int amount_is_f64, int64_t n,
                                const double *d_theta, const int64_t *d_close_idx, int64_t n_idx,
                                double theta_mult, float *d_mean_size_rel, float *d_size_95_rel,
                                float *d_pct_block, float *d_size_gini);
int fmk_comp_bar_trade_size(fmk_ctx *ctx, const void *amount, int amount_is_f64, int64_t n,
                            const double *theta, const int64_t *close_idx, int64_t n_idx,
                            double theta_mult, float *mean_size_rel, float *size_95_rel,
                            float *pct_block, float *size_gini);

/* comp_bar_microstructure_features: the tick-level estimators of AFML ch. 19 per bar (the reference has none; DESIGN.md "Per-bar
 * microstructure features" is the definition).  Bar b holds the ticks s = ci[b] + 1 .. e = ci[b + 1], L of them.  For t = s + 1 .. e,
 * in float64 without contraction (m = L - 1 of each; a bar reads no tick outside itself):
 *   d_t = p_t - p_{t-1};  r_t = log(p_t / p_{t-1}), the quotient rounded, then the host's log bits (as comp_lagged_returns);
 *   xk_t = side_t * v_t;  xa_t = p_t * v_t;  xh_t = side_t * sqrt(p_t * v_t), product rounded, root correctly rounded;
 *   q_t = d_t * d_{t-1} for t = s + 2 .. e.
 * Three regressions through the origin over the m differences -- Kyle (d on xk), Amihud (|r| on xa), Hasbrouck (r on xh) -- from the
 * float64 moments Sxx, Sxy, Syy, whose summation ORDER IS FREE but a function of the bar alone.  The first rule that holds:
 *   1. m < 2, a moment not finite, or Sxx == 0 -> lambda = t = NaN;          2. Syy == 0 -> lambda = t = 0.0;
 *   3. lambda = Sxy / Sxx, u = 1 - Sxy Sxy / (Sxx Syy); u <= 2^-26 -> t = copysign(inf, Sxy);
 *   4. t = Sxy / sqrt(Sxx Syy) * sqrt((m - 1) / u).
 * Roll: serial_cov = sum(q) / (m - 1) for m >= 2, else NaN; roll_spread = 2 sqrt(-serial_cov) where it is negative, 0.0 where it is
 * >= 0, NaN where it is NaN.  Nothing fails for a degenerate bar: bars of 0, 1 and 2 ticks are NaN rows, and rule 1 makes a
 * non-positive or non-finite price or an infinite amount a NaN row.
 * Refused (FMK_E_ARG): n_idx < 1, an output that overlaps an input, a close index outside [-1, n) -- the host flavour before
 * anything is uploaded; the device flavour finds a bad close index on the device: such a bar is not read, the call waits once for
 * that flag.  n_idx == 1 is zero bars and succeeds. */
typedef struct fmk_microstructure_out {
    double *kyle_lambda, *kyle_t, *amihud_lambda, *amihud_t, *hasbrouck_lambda, *hasbrouck_t, *serial_cov, *roll_spread;
} fmk_microstructure_out;
int fmk_comp_bar_microstructure_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount, int amount_is_f64, int64_t n,
                                    const int64_t *d_close_idx, int64_t n_idx, const int8_t *d_side,
                                    const fmk_microstructure_out *d_out);
int fmk_comp_bar_microstructure(fmk_ctx *ctx, const double *price, const void *amount, int amount_is_f64, int64_t n,
                                const int64_t *close_idx, int64_t n_idx, const int8_t *side, const fmk_microstructure_out *out);

/* ---- cfg 4: time bars + order-flow + footprints ----------------------------------------
 * Replaces BarBuilderBase.build_ohlcv + build_directional_features + build_footprints (base.py:126-300) called back to back (38 B/tick
 * as three reducers).  Two phases like comp_bar_footprints (the CSR row count must reach the caller's allocator).  (Round 1's
 * fmk_bars_fused_size_dev / _fill_dev -- comp_bar_ohlcv, then the two other reducers back to back -- were superseded by the entry
 * points below and removed in round 6.) */
/* cfg 4 in TWO passes over the ticks (round 2; 26 B/tick): build_ohlcv + build_directional_features semantics from one read of
 * price / amount / side (float32 amounts: one kernel; float64 amounts: the two kernels back to back), then the CSR level
 * counts.  The second pass is fmk_comp_bar_footprints_fill_dev with the offsets and lows produced here. */
int fmk_bars_flow_size_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount, int amount_is_f64, int64_t n,
                           const int64_t *d_close_idx, int64_t n_idx, const int8_t *d_side, double price_tick_size,
                           double *d_open, double *d_high, double *d_low, double *d_close, float *d_volume, double *d_vwap,
                           int64_t *d_trades, double *d_median /* may be NULL */, const fmk_directional_out *d_dir,
                           int64_t *d_n_zero_div, int64_t *d_level_offsets, int64_t *total_levels, int64_t *max_levels);
/* cfg 4 at 26 B/tick (round 3): the same first pass, but the median trade size of comp_bar_ohlcv (base.py:401-404) may be left
 * to the footprint sweep, whose waves hold every amount of their bar anyway -- no pass of its own over the amount column.
 * *median_deferred = 1: nothing was written to d_median, the caller passes it to fmk_comp_bar_footprints_fill_median_dev;
 * 0: d_median is complete (float64 amounts, very short / very long bars) and the plain fill call follows. */
int fmk_bars_flow_size_defer_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount, int amount_is_f64, int64_t n,
                                 const int64_t *d_close_idx, int64_t n_idx, const int8_t *d_side, double price_tick_size,
                                 double *d_open, double *d_high, double *d_low, double *d_close, float *d_volume,
                                 double *d_vwap, int64_t *d_trades, double *d_median, const fmk_directional_out *d_dir,
                                 int64_t *d_n_zero_div, int64_t *d_level_offsets, int64_t *total_levels, int64_t *max_levels,
                                 int *median_deferred);
/* comp_bar_footprints' fill phase (as fmk_comp_bar_footprints_fill_dev) that ALSO writes the per-bar median trade size
 * (float32 amounts only; d_median NULL = the plain fill). */
int fmk_comp_bar_footprints_fill_median_dev(fmk_ctx *ctx, const double *d_price, const void *d_amount, int amount_is_f64,
                                            int64_t n, const int64_t *d_close_idx, int64_t n_idx, const int8_t *d_side,
                                            double price_tick_size, const double *d_bar_lows, double imbalance_factor,
                                            const int64_t *d_level_offsets, int64_t max_levels,
                                            const fmk_footprint_out *d_out, int64_t *d_n_bad_level, double *d_median);

/* ---- tick-level feature loops: finmlkit/feature/core ---------------------------------- */
/* comp_lagged_returns (core/utils.py:12-64). */
int fmk_comp_lagged_returns_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_close,
                                int64_t n, double return_window_sec, int is_log, double *d_out);
int fmk_comp_lagged_returns(fmk_ctx *ctx, const int64_t *ts, const double *close_, int64_t n,
                            double return_window_sec, int is_log, double *out);
/* ewmst / ewmst_mean0 (core/volatility.py:139-219, 72-136).  Every tick is the reference's own update and closing expression, but
 * the state that enters a thread's 8 ticks is composed from per-tile affine maps: NaN positions, out[0], exact zeros and every
 * output that is sigma_floor are the reference's; the rest is within 1e-9 relative, or 1e-11 x the series' typical sigma absolute.
 * Any half life is taken as the reference takes it (zero, negative and non-finite ones included).  Not part of the contract: an
 * infinite y.  The loop keeps an infinite state where a composed map whose decay product has underflowed to 0 gives 0 * inf = NaN.
 * What holds there: the outputs before the first infinite element are unaffected; from it on ewmst is sigma_floor, as the
 * reference's (a NaN and an infinite state give the same closing expression); ewmst_mean0 is inf or NaN from it on, and equals the
 * reference's where no decay product up to the tick has underflowed.
 * ewmst after a restart.  A tick with 1 - alpha <= 1e-5 (a weekend gap) leaves the state one sample, and so does the first tick
 * that carries a weight.  While only gaps of nanoseconds follow, the closing expression is a quotient of two cancellation residues
 * and only the loop's own state gives the loop's sigma, so those ticks are stepped in the reference's order (k_ew_restart_walk),
 * from the end of the 8-tick group that holds the restart until the weights are those of more than one sample
 * (V^2 - V2 >= 1e-4 V^2), the next restart or the end of the series.  Limits, behind which the composed state's outputs stay and
 * the 1e-9 is not promised for such ticks: 65 536 ticks per walk (a run of that many ticks within nanoseconds of a restart), and
 * 65 536 8-tick groups with a restart per call (a call with more is not walked at all; its result does not depend on the run).
 * fmk_ewmst_shard_apply_dev walks too (a shard that enters with weights has no first tick of its own); the kernel behind
 * FMK_EW_ONE_PASS does not. */
int fmk_ewmst_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_y, int64_t n,
                  double half_life, double sigma_floor, int mean0, double *d_out);
int fmk_ewmst(fmk_ctx *ctx, const int64_t *ts, const double *y, int64_t n, double half_life,
              double sigma_floor, int mean0, double *out);
/* Shards of ONE series across GPUs: tick 0 of the arrays is the last tick of the previous shard
 * (rank 0: its own first tick).  _map: affine map (a, a2, bV, bV2, bSy, bSyy) of ticks 1..n-1 -> d_map_out[6];
 * _apply: outputs from the incoming state d_state_in[4] = (V, V2, Sy, Syy) (device pointers; NULL = zeros). */
int fmk_ewmst_shard_map_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_y, int64_t n, double half_life,
                            int mean0, double *d_map_out);
int fmk_ewmst_shard_apply_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_y, int64_t n, double half_life,
                              double sigma_floor, int mean0, const double *d_state_in, double *d_out);
/* ewms (core/volatility.py:9-69): fixed alpha = 2/(span+1); span <= 1 -> all NaN. */
int fmk_ewms_dev(fmk_ctx *ctx, const double *d_y, int64_t n, int64_t span, double *d_out);
int fmk_ewms(fmk_ctx *ctx, const double *y, int64_t n, int64_t span, double *out);
/* realized_vol (core/volatility.py:256-286): rolling sqrt(nansum(r^2)/(valid - is_sample)) over `window`
 * elements; NaN where fewer than 2 valid returns or before the first full window.  FMK_E_ARG: window < 1 (the host
 * layer answers window == 0 itself: all NaN, like the reference; negative windows stay rejected). */
int fmk_realized_vol_dev(fmk_ctx *ctx, const double *d_r, int64_t n, int64_t window, int is_sample,
                         double *d_out);
int fmk_realized_vol(fmk_ctx *ctx, const double *r, int64_t n, int64_t window, int is_sample, double *out);

/* ---- rolling volume profile: finmlkit/feature/core/volume.py:133-456 ("next" rank 2) --------- */
/* volume_profile_rolling on CSR footprints (level_offsets[n_bars+1] + flat level arrays, the layout
 * fmk_comp_bar_footprints produces).  first_bar = searchsorted(bar_ts, bar_ts[0] + window_ns) (volume.py:432):
 * earlier bars keep 0.  n_bins < 0: no bucketing (n_bins=None).  Outputs: POC / HVA / LVA in tick units (int32) and
 * the share of volume above the POC (float32).  FMK_E_LEVEL: a level outside its window (the reference raises IndexError above the
 * range and folds a level below it onto the lowest one), or a single-level window with bucketing (refused here; the interpreted
 * reference hands the one level back as its only bin -- both on record in tests/golden/vp_edges.json); FMK_E_ZERODIV: n_bins == 0; FMK_E_CAPACITY: a window wider than 1 << 24
 * levels (up to 8192 the histogram is in LDS, above in global scratch).
 * NaN rule: a NaN low or high in a window that is computed makes np.min / np.max NaN and the reference's int(round(nan)) raises
 * ValueError; so does this entry, with FMK_E_ARG, for the whole call and before any histogram is sized -- also where a window's
 * lows / highs over price_tick are infinite or beyond 2^61 (the reference: OverflowError, or a level no int32 holds).  A NaN in a bar
 * that no computed window holds is not looked at.  fmk_aggregate_footprint follows the same rule for its one window. */
int fmk_volume_profile_rolling_dev(fmk_ctx *ctx, const int64_t *d_bar_ts, const double *d_highs, const double *d_lows,
                                   const int64_t *d_level_offsets, const int32_t *d_price_levels,
                                   const float *d_buy_volumes, const float *d_sell_volumes, int64_t n_bars,
                                   int64_t first_bar, int64_t window_ns, int64_t n_bins, double price_tick,
                                   double va_pct, int32_t *d_poc, int32_t *d_hva, int32_t *d_lva, float *d_pct);
int fmk_volume_profile_rolling(fmk_ctx *ctx, const int64_t *bar_ts, const double *highs, const double *lows,
                               const int64_t *level_offsets, const int32_t *price_levels, const float *buy_volumes,
                               const float *sell_volumes, int64_t n_bars, int64_t first_bar, int64_t window_ns,
                               int64_t n_bins, double price_tick, double va_pct, int32_t *poc, int32_t *hva,
                               int32_t *lva, float *pct);

/* volume_profile_developing (volume.py:493-569) on CSR footprints: the session-anchored profile.  For every range r of bars
 * [range_starts[r], range_ends[r]) (host arrays of bar indices; the Python layer makes them from time stamps by searchsorted left of
 * start_ts, right of end_ts) and every bar t of it, POC / HVA / LVA (int32, tick units) of everything traded from the range's first
 * bar up to and including t.  Ranges are independent; they may touch or overlap.  THE CONTRACT:
 *  1 level range   int(round(min(lows) / price_tick)) .. int(round(max(highs) / price_tick)) over ALL bars of the range, once (it
 *                  looks ahead, as the reference does), half-even like the rolling entry.
 *  2 accumulation  bars one after another, per level float32 `+=` for buy and for sell (a bar's levels are distinct); after every
 *                  bar total = buy + sell in float32.
 *  3 n_bins < 0    (n_bins=None) comp_poc_hva_lva on the whole dense range with the unrounded totals, no trim.
 *  4 n_bins > 0    np.round(total, 8) evaluated in float32 (rint(v * 1e8f) / 1e8f, both operations rounded to float32); leading and
 *                  trailing entries that compare == 0 are dropped (a NaN or a negative entry stops the trim); bucket_price_levels on
 *                  the trimmed levels -- the layout changes from bar to bar as the trimmed range grows -- then comp_poc_hva_lva.
 *  5 position      the outputs of bar t of range r go to element out_offsets[r] + (t - range_starts[r]) of d_poc / d_hva / d_lva; no
 *                  other element is written.  (The reference indexes its range-long outputs with t itself, which fails for every
 *                  range that does not begin at bar 0; t - start is the documented intent, and equals the reference on the arrays
 *                  sliced from the range's first bar.)
 *  6 one level     a trimmed profile of one level under bucketing comes back as its only (leftover) bin: POC = HVA = LVA = that level,
 *                  as the interpreted reference hands it back behind its warning.  (The rolling entry refuses that case.)
 *  7 all zero      every rounded total 0 under bucketing (an empty first bar): FMK_E_LEVEL for the whole call -- the reference raises
 *                  ValueError, np.min of nothing; the message names the first such bar: lowest range, then lowest bar.  Without
 *                  bucketing the call returns; the POC is the lowest level (the argmax of zeros is 0).
 *  8 stages        total, argmax and walk as stated for fmk_comp_poc_hva_lva below.  There is no share above the POC.
 * n_bins < 0: no bucketing, as in the rolling entry.  chunk_bars: 0 = chosen by the entry; the results do not depend on it in any bit
 * (a range's bars are replayed in chunks of that many bars from snapshots of the float32 sums).
 * FMK_E_ARG: an empty range (the reference: ValueError) or one that reaches outside the bars, price_tick not above 0, a NaN or
 * infinite low or high inside a range (outside every range it is not looked at); FMK_E_LEVEL: a footprint level outside its range's
 * level range, a range whose highest high lies below its lowest low, item 7; FMK_E_ZERODIV: n_bins == 0; FMK_E_CAPACITY: a range wider
 * than 1 << 24 levels (up to 8192 the working set is in LDS, above in global scratch).
 * The host-pointer twin takes n_out, the length of poc / hva / lva; elements that no range covers keep what they held. */
int fmk_volume_profile_developing_dev(fmk_ctx *ctx, const double *d_highs, const double *d_lows, const int64_t *d_level_offsets,
                                      const int32_t *d_price_levels, const float *d_buy_volumes, const float *d_sell_volumes,
                                      int64_t n_bars, const int64_t *range_starts, const int64_t *range_ends,
                                      const int64_t *out_offsets, int64_t n_ranges, int64_t n_bins, double price_tick, double va_pct,
                                      int64_t chunk_bars, int32_t *d_poc, int32_t *d_hva, int32_t *d_lva);
int fmk_volume_profile_developing(fmk_ctx *ctx, const double *highs, const double *lows, const int64_t *level_offsets,
                                  const int32_t *price_levels, const float *buy_volumes, const float *sell_volumes, int64_t n_bars,
                                  const int64_t *range_starts, const int64_t *range_ends, const int64_t *out_offsets,
                                  int64_t n_ranges, int64_t n_bins, double price_tick, double va_pct, int64_t chunk_bars,
                                  int32_t *poc, int32_t *hva, int32_t *lva, int64_t n_out);

/* calc_volume_percentage_above_poc (volume.py:367-391) on ONE profile: share of the volume on levels above `poc_price`
 * (NumPy-pairwise float32 total, the levels above added in order in float64, float64 quotient = the Numba-typed function). */
int fmk_calc_volume_percentage_above_poc_dev(fmk_ctx *ctx, const int32_t *d_price_levels, const float *d_volumes, int64_t n,
                                             int32_t poc_price, double *d_out);
int fmk_calc_volume_percentage_above_poc(fmk_ctx *ctx, const int32_t *price_levels, const float *volumes, int64_t n,
                                         int32_t poc_price, double *out);

/* The three stages of volume_profile_rolling as the reference exposes them (host arrays; the rolling entry above is the hot path):
 * aggregate_footprint (volume.py:134-203): the window [start_ts, end_ts] of bars (searchsorted left / right, the one-bar fallback),
 *   its dense level range from min(lows) / max(highs) (int(round(x / price_tick))), buy / sell volumes of the window's footprints
 *   (CSR: level_offsets[n_bars + 1]) added bar after bar in float32.  aligned_buy == NULL: sizes only (*min_level, *n_levels).
 * bucket_price_levels (volume.py:207-275): odd-width buckets over [min, max] of the levels, float32 sums in element order, the
 *   leftover bucket when the last level falls past the last edge.  binned_* == NULL: *n_out only.
 * comp_poc_hva_lva (volume.py:278-365): first argmax, then the value area grown two levels at a time towards the heavier side
 *   until va_pct of the total is covered.  THE CONTRACT: the total is np.sum of the float32 array as NumPy computes it (pairwise
 *   float32 -- the reference's pinned pure-Python mode; a jitted np.sum is a sequential float32 loop and can differ in the last bit),
 *   the walk's scalars are float64 (the typed reading of the function's `0.0` literals; pure Python under NumPy 2 adds its np.float32
 *   scalars in float32).  The readings coincide whenever the partial sums are exact, and on all 400 lognormal float32 profiles of
 *   tests/golden/volume_profile_stages.npz (`poc_lognormal`, made by the reference itself); a knife-edge profile whose covered volume
 *   equals the threshold to the last float32 bit can move HVA / LVA by one step between them. */
int fmk_aggregate_footprint(fmk_ctx *ctx, const int64_t *bar_ts, const double *highs, const double *lows,
                            const int64_t *level_offsets, const int32_t *price_levels, const float *buy_volumes,
                            const float *sell_volumes, int64_t n_bars, int64_t start_ts, int64_t end_ts, double price_tick,
                            int32_t *min_level, int64_t *n_levels, float *aligned_buy, float *aligned_sell, int64_t capacity);
int fmk_bucket_price_levels(fmk_ctx *ctx, const int32_t *all_price_levels, const float *total_volumes, int64_t n, int64_t n_bins,
                            int32_t *binned_price_levels, float *binned_volumes, int64_t capacity, int64_t *n_out);
int fmk_comp_poc_hva_lva(fmk_ctx *ctx, const int32_t *price_levels, const float *volumes, int64_t n, double va_pct,
                         int32_t *poc_price, int32_t *hva_price, int32_t *lva_price);

/* ---- CUSUM bars: finmlkit/bar/logic.py:152-221 ("next" rank 3) ------------------------------ */
/* _cusum_bar_indexer: sigma is forward-filled IN PLACE from its first non-NaN entry (like the reference); the
 * result starts with that entry's index, then one index per close.  d_out == NULL: count only (*n_out).
 * *n_rounds (may be NULL): rounds the parallel-in-time fixed point needed (chunks opened, when the chain walk for rarely
 * reached thresholds served the call).  FMK_E_CAPACITY: capacity < *n_out. */
int fmk_cusum_bar_indexer_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_price, double *d_sigma, int64_t n,
                              double sigma_floor, double sigma_mult, int64_t *d_out, int64_t capacity,
                              int64_t *n_out, int64_t *n_rounds);
int fmk_cusum_bar_indexer(fmk_ctx *ctx, const int64_t *ts, const double *price, double *sigma, int64_t n,
                          double sigma_floor, double sigma_mult, int64_t *out, int64_t capacity, int64_t *n_out);

/* ---- the symmetric CUSUM event filter: finmlkit/sampling/filters.py:7-70 ------------------------------------------
 * cusum_filter on any float64 series x of n >= 2 elements: for i = 1 .. n-1, ret = log(x[i] / x[i-1]) (the host's log:
 * csrc/fmk_log.h), s_pos = max(0, s_pos + ret), s_neg = min(0, s_neg + ret); s_neg < -thr[i] resets s_neg and emits i, else
 * s_pos > thr[i] resets s_pos and emits i (the negative side first, strict comparisons).  thr: one constant (n_thr == 1) or one
 * value per element (n_thr == n).  The indices are the reference's bit for bit on every input (NaN / non-positive x, NaN /
 * negative / infinite thresholds included).  d_out == NULL: count only (*n_out).  *n_rounds (may be NULL): launches over the
 * chunks (pass A + fix-ups).  FMK_E_ARG with the reference's messages: n <= 1, n_thr not 1 or n.  FMK_E_CAPACITY: capacity <
 * *n_out (which is set).  FMK_CUSUM_FILTER_FORM=onepass|fixed forces one of the two schedules (tests). */
int fmk_cusum_filter_dev(fmk_ctx *ctx, const double *d_x, int64_t n, const double *d_thr, int64_t n_thr, int64_t *d_out,
                         int64_t capacity, int64_t *n_out, int64_t *n_rounds);
int fmk_cusum_filter(fmk_ctx *ctx, const double *x, int64_t n, const double *thr, int64_t n_thr, int64_t *out, int64_t capacity,
                     int64_t *n_out);

/* ---- the Chu-Stinchcombe-White CUSUM test on levels: finmlkit/feature/core/structural_break/cusum.py -------------
 * cusum_test_rolling / cusum_test_developing on a float64 price series x of n elements -> four float64 arrays of n elements: the
 * one-sided statistics (up, down) and their critical values, bit for bit what the reference's code gives with the host's log()
 * (csrc/fmk_log.h) as its np.log -- the log it has when Numba compiles it; interpreted, NumPy's own log rounds a few arguments
 * in a thousand differently -- NaN positions included (every window's variance summed in index order; the first n that attains a side's
 * maximum gives its critical value).  Output t looks back to base(t) = max(0, t - window_size) (developing: 0); outputs below
 * warmup_period are NaN.  Rolling raises window_size to warmup_period + 2, returns all-NaN when n < warmup_period + 2 and checks
 * the prices first; developing checks nothing (log of 0 or a negative number flows through).  window_size may be anything: a
 * window that does not fit one LDS staging is walked in slabs (FMK_BREAK_SLAB=<elements> shrinks the slab: tests only).
 * FMK_E_ARG: "All close prices must be positive." (rolling: an element <= 0; NaN passes), "warmup_period must be at least 2."
 * (the reference divides by zero or reads out of bounds there), n >= 2^31.  The rolling call waits once, for the price check. */
int fmk_cusum_test_rolling_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window_size, int64_t warmup_period,
                               double *d_up, double *d_down, double *d_crit_up, double *d_crit_down);
int fmk_cusum_test_developing_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t warmup_period, double *d_up, double *d_down,
                                  double *d_crit_up, double *d_crit_down);
int fmk_cusum_test_rolling(fmk_ctx *ctx, const double *x, int64_t n, int64_t window_size, int64_t warmup_period, double *up,
                           double *down, double *crit_up, double *crit_down);
int fmk_cusum_test_developing(fmk_ctx *ctx, const double *x, int64_t n, int64_t warmup_period, double *up, double *down,
                              double *crit_up, double *crit_down);

/* ---- rolling-window moments: finmlkit/feature/core/ma.py (sma), utils.py (comp_zscore), volatility.py (rolling_variance_nb,
 * variance_ratio_1_4_core) on a float64 series of n elements -> one float64 array of n elements, NaN before the first full window
 * (everywhere when window > n).  Bit for bit the reference's evaluation order as Numba compiles it: every window summed on its own,
 * left to right, one rounded addition per element, nothing contracted (interpreted NumPy sums pairwise from 8 elements up and
 * differs there); NaN positions included.
 *   sma:      (1.0 / window) * sum.
 *   zscore:   mean = sum / window, std = sqrt(sum((x - mean)^2) / (window - ddof)), (x[t] - mean) / std, NaN where std == 0.
 *   rolling_variance: cnt, s, q over the non-NaN elements; cnt >= min_periods and cnt > ddof: m = s / cnt,
 *             max(0, (q / cnt - m * m) * (cnt / (cnt - ddof))), else NaN.
 *   variance_ratio_1_4: r1 = log(p[i] / p[i-1]) (is_log; the host's log: csrc/fmk_log.h; NaN where a price is NaN or <= 0) or
 *             p[i] / p[i-1] - 1 (NaN where a price is NaN or p[i-1] <= 0), r4 = ((r1[i] + r1[i-1]) + r1[i-2]) + r1[i-3], v1 / v4 the
 *             rolling variances (min_periods 1), out = v1 / (v4 / 4) where both are numbers and v4 > 0; all NaN when n < window + 4.
 *             Scratch (3 n float64) comes from the context's pool.
 * FMK_E_ARG, checked before a device is touched: window < 1, n >= 2^31, zscore with window - ddof <= 0 (the reference divides by
 * zero or takes the root of a negative number there). */
int fmk_sma_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out);
int fmk_sma(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out);
int fmk_zscore_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t ddof, double *d_out);
int fmk_zscore(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, int64_t ddof, double *out);
int fmk_rolling_variance_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t ddof, int64_t min_periods,
                             double *d_out);
int fmk_rolling_variance(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, int64_t ddof, int64_t min_periods, double *out);
int fmk_variance_ratio_1_4_dev(fmk_ctx *ctx, const double *d_price, int64_t n, int64_t window, int64_t ddof, int is_log,
                               double *d_out);
int fmk_variance_ratio_1_4(fmk_ctx *ctx, const double *price, int64_t n, int64_t window, int64_t ddof, int is_log, double *out);

/* ---- windowed order statistics: finmlkit/feature/core/utils.py (comp_burst_ratio, pct_change), momentum.py (roc, stoch_k) on float64
 * series of n elements -> one float64 array of n elements.  A median, a minimum and a maximum are selections without an evaluation
 * order; the arithmetic after them is the reference's, one rounded operation each, nothing contracted: every output is the
 * reference's bits (its pure-Python mode), NaN positions included.
 *   burst_ratio: NaN before window - 1 (everywhere when window > n); W = x[i - window + 1 .. i]: NaN when W holds a NaN (np.median),
 *             med = the middle element of sorted W (odd window) or (a + b) / 2.0 over the two middle ones (even window),
 *             out = x[i] / med when med > 0, NaN otherwise.  Windows up to 3073 sort a tile's span in LDS; longer ones select by
 *             bisection over the key's bits (csrc/fmk_order.hip); no window <= n is refused.
 *   stoch_k:  NaN before length - 1 (everywhere when length > n); lo = min(low[W]), hi = max(high[W]),
 *             out = (100.0 * (close[t] - lo)) / (hi - lo) when hi > lo, NaN otherwise and when low or high holds a NaN in W (the
 *             reference carries its extremes and is path-dependent there: a documented deviation).  Signed zeros among low / high
 *             are not part of the contract.
 *   roc:      NaN before period; ((x[i] - x[i - period]) / x[i - period]) * 100.0, a zero divisor giving the IEEE result.
 *   pct_change: NaN before periods; base = x[t - periods]: (x[t] - base) / base when base > 0, NaN otherwise.
 * No scratch memory is taken.  FMK_E_ARG, checked before a device is touched and before any pointer is looked at: window < 1,
 * length < 1, period < 0, periods < 0, n >= 2^31. */
int fmk_burst_ratio_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out);
int fmk_burst_ratio(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out);
int fmk_stoch_k_dev(fmk_ctx *ctx, const double *d_close, const double *d_low, const double *d_high, int64_t n, int64_t length,
                    double *d_out);
int fmk_stoch_k(fmk_ctx *ctx, const double *close, const double *low, const double *high, int64_t n, int64_t length, double *out);
int fmk_roc_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t period, double *d_out);
int fmk_roc(fmk_ctx *ctx, const double *x, int64_t n, int64_t period, double *out);
int fmk_pct_change_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t periods, double *d_out);
int fmk_pct_change(fmk_ctx *ctx, const double *x, int64_t n, int64_t periods, double *out);

/* ---- recursive indicators: finmlkit/feature/core/ma.py (ewma), momentum.py (rsi_wilder), volatility.py (true_range, atr),
 * trend.py (adx_core) on float64 series of n elements -> one float64 array of n elements (csrc/fmk_recur.hip).
 *   true_range: bar 0: high - low, NaN when one of them is; bar i: max(high - low, |high - close[i-1]|, |low - close[i-1]|), NaN
 *             when high, low or close[i-1] is NaN.  The reference's bits.
 *   atr:      window 0 or window > n: NaN everywhere.  SMA mode (ema_based == 0): NaN before window - 1, then the mean of the non-NaN
 *             true ranges of the window, added left to right (NaN when there is none; NaN at bar 2 when its high, low and close are
 *             all NaN).  The reference's bits.  EMA mode: NaN before window - 1, there the mean of the non-NaN true ranges so far,
 *             then ((window - 1) * atr + tr) / window, NaN for good from the first NaN true range on.  normalize: divided by
 *             (high + low) / 2.0 where that and the value are numbers and it is > 0.
 *   ewma:     alpha = 2 / (span + 1), u = y + (1 - alpha) * u, v = 1 + (1 - alpha) * v from (y[0], 1), out = u / v.
 *   rsi_wilder: NaN before `window` (everywhere when n <= window); the gains and losses of close[1 .. window] summed and divided by
 *             window, then avg = ((window - 1) * avg + x) / window; out = 100 - 100 / (1 + gain / loss) where loss > 0, NaN
 *             otherwise.  A NaN difference inside the first window gives NaN everywhere; later it counts as no gain and no loss.
 *   adx:      true range (0 at bar 0, no NaN checks), +DM and -DM summed over bars 1 .. length, then s = s - s / length + x; the
 *             directional indices and dx from them; adx[2 length - 1] = mean(dx[length .. 2 length)), then
 *             (adx * (length - 1) + dx) / length.  0.0 before 2 length - 1 and everywhere when n < 2 length.
 * The four recurrences run as a device-wide scan: every step is the reference's own expression, but the state that enters a
 * thread's 8 elements is composed from per-tile aggregates, so the outputs from the seed index on agree with the reference to a few
 * units in the last place of the running averages (1e-9 relative is the contract; for rsi_wilder and adx 1e-7 absolute on their
 * 0 .. 100 scale), while NaN positions, the outputs before the seed and adx's exact zeros are the reference's.  The seeds are added
 * in index order.  Not part of the contract: infinite inputs to the four recurrences, and a state that has decayed below
 * 2^-969 over elements that add nothing to it, until every channel has taken a non-zero term again (the reference stalls at the
 * smallest subnormals for windows >= 3 and reaches 0.0 for windows <= 2; the composed state here underflows to 0.0).  Scratch: the context's scratch (one record per 2048 elements); adx takes n float64 from the context's pool.
 * FMK_E_ARG, checked before a device is touched and before any pointer is looked at: span < 1, rsi_wilder window < 1, atr window < 0,
 * length < 1, n >= 2^31. */
int fmk_ewma_dev(fmk_ctx *ctx, const double *d_y, int64_t n, double span, double *d_out);
int fmk_ewma(fmk_ctx *ctx, const double *y, int64_t n, double span, double *out);
int fmk_rsi_wilder_dev(fmk_ctx *ctx, const double *d_close, int64_t n, int64_t window, double *d_out);
int fmk_rsi_wilder(fmk_ctx *ctx, const double *close, int64_t n, int64_t window, double *out);
int fmk_true_range_dev(fmk_ctx *ctx, const double *d_high, const double *d_low, const double *d_close, int64_t n, double *d_out);
int fmk_true_range(fmk_ctx *ctx, const double *high, const double *low, const double *close, int64_t n, double *out);
int fmk_atr_dev(fmk_ctx *ctx, const double *d_high, const double *d_low, const double *d_close, int64_t n, int64_t window,
                int ema_based, int normalize, double *d_out);
int fmk_atr(fmk_ctx *ctx, const double *high, const double *low, const double *close, int64_t n, int64_t window, int ema_based,
            int normalize, double *out);
int fmk_adx_dev(fmk_ctx *ctx, const double *d_high, const double *d_low, const double *d_close, int64_t n, int64_t length,
                double *d_out);
int fmk_adx(fmk_ctx *ctx, const double *high, const double *low, const double *close, int64_t n, int64_t length, double *out);

/* ---- running-sum indicators: finmlkit/feature/core/volatility.py (bollinger_percent_b, parkinson_range), reversion.py
 * (vwap_distance), volume.py (comp_flow_acceleration, vpin) on float64 series of n elements -> one array of n elements, float64 but
 * for vpin's float32 (csrc/fmk_runsum.hip).
 *   bollinger_percent_b: NaN before window - 1 and everywhere when n < window or window == 1.  sum and sum of squares of the first
 *             window in index order, then sum += close[i] - close[i-window], sumsq += close[i]^2 - close[i-window]^2; mean = sum /
 *             window, var = (sumsq - T) / (window - 1) with T = window * mean * mean at window - 1 and window * (mean * mean) after
 *             it, sd = sqrt(var < 0 ? 0 : var); (close - lower) / (upper - lower) where upper > lower, NaN otherwise.
 *   vwap_distance: NaN before n_periods - 1 and everywhere when n < n_periods.  wsum and vsum of the first window in index order,
 *             then wsum += close[i] * volume[i] - close[i-w] * volume[i-w], vsum += volume[i] - volume[i-w].  Where vsum > 0:
 *             close / (wsum / vsum) - 1.0, with is_log after the first window log(close / (wsum / vsum)); where it is not (a NaN
 *             vsum included) the output before it, NaN when there is none.
 *   flow_acceleration: NaN before window - 1 and everywhere when n < window or recent_periods >= window.  S the prefix sum of the
 *             volumes; log(((S[i+1] - S[i+1-r]) + 1e-12) / ((S[i+1-r] - S[i+1-window]) + 1e-12)).
 *   vpin:     prefix sums of buy, sell, |buy - sell| and of the bars with a NaN (which add 0.0 to the three sums).  Where i >= window
 *             - 1, the window holds no NaN bar and its buy + sell total is > 1e-9: float32(|buy - sell| total / total), the division
 *             in float64; NaN otherwise.  window 0: NaN everywhere.
 *   parkinson_range: log(high / low)^2 / (log(2.0) * 4.0).  The reference's bits.
 * log is the host's.  The four running sums are the scan of the recursive indicators with the coefficient 1: every step is the
 * reference's own expression, but the sum that enters a thread's 8 elements is added in another order, so the outputs agree with the
 * reference bit for bit on exactly summable inputs and to a few units in the last place of the largest running sum otherwise
 * (measured: DESIGN.md section 7f); NaN positions, the outputs before the seed and which vwap_distance outputs are held are the
 * reference's.  Not part of the contract: infinite inputs; on inputs that are not exactly summable, a Bollinger window whose elements
 * are all equal and whether a window of all-zero volumes holds.  Memory: the context's scratch (one record per 2048 elements);
 * from the context's pool vwap_distance takes n / 4 bytes, flow_acceleration n and vpin 4 n float64.
 * FMK_E_ARG, checked before a device is touched and before any pointer is looked at: bollinger window < 1, n_periods < 1,
 * recent_periods < 0, vpin window < 0, n >= 2^31. */
int fmk_bollinger_percent_b_dev(fmk_ctx *ctx, const double *d_close, int64_t n, int64_t window, double num_std, double *d_out);
int fmk_bollinger_percent_b(fmk_ctx *ctx, const double *close, int64_t n, int64_t window, double num_std, double *out);
int fmk_vwap_distance_dev(fmk_ctx *ctx, const double *d_close, const double *d_volume, int64_t n, int64_t n_periods, int is_log,
                          double *d_out);
int fmk_vwap_distance(fmk_ctx *ctx, const double *close, const double *volume, int64_t n, int64_t n_periods, int is_log, double *out);
int fmk_flow_acceleration_dev(fmk_ctx *ctx, const double *d_volumes, int64_t n, int64_t window, int64_t recent_periods, double *d_out);
int fmk_flow_acceleration(fmk_ctx *ctx, const double *volumes, int64_t n, int64_t window, int64_t recent_periods, double *out);
int fmk_vpin_dev(fmk_ctx *ctx, const double *d_volume_buy, const double *d_volume_sell, int64_t n, int64_t window, float *d_out);
int fmk_vpin(fmk_ctx *ctx, const double *volume_buy, const double *volume_sell, int64_t n, int64_t window, float *out);
int fmk_parkinson_range_dev(fmk_ctx *ctx, const double *d_high, const double *d_low, int64_t n, double *d_out);
int fmk_parkinson_range(fmk_ctx *ctx, const double *high, const double *low, int64_t n, double *out);

/* ---- rolling price-volume correlation: finmlkit/feature/core/correlation.py (rolling_price_volume_correlation) on two float64
 * series of n elements -> float64 array of n elements (csrc/fmk_corr.hip).
 *   ret[0] = NaN; ret[i] = (price[i] - price[i-1]) / price[i-1] where neither price is NaN and price[i-1] != 0 (-0.0 is zero), NaN
 *   otherwise.  out[t] = NaN for t < window (one more than sma; everywhere when window >= n) and where ret[t] or volume[t] is NaN.
 *   Otherwise, over the pairs (ret[j], volume[j]), j = t - window + 1 .. t, with no NaN, ascending: fewer than 2 -> NaN; the means
 *   sr / cnt and sv / cnt of left-to-right sums; cov, qr, qv the left-to-right sums of dr * dv, dr * dr, dv * dv; where qr > 0 and
 *   qv > 0: cov / (sqrt(qr) * sqrt(qv)) clamped to [-1, 1]; NaN otherwise.  For 4 <= t < 10 the reference's special case comes
 *   before the sums: with up / incv / decv = no price[j+1] <= price[j] / no volume[j+1] <= volume[j] / no volume[j+1] >= volume[j]
 *   over j = t - window + 1 .. t - 1, up and incv give 1.0, else up and decv -1.0 (a NaN there fails no comparison).
 * The reference's bits: every window is computed on its own in the reference's order.
 * FMK_E_ARG, checked before a device is touched and before any pointer is looked at: window < 1 (the reference indexes from the end
 * of the arrays there), n >= 2^31. */
int fmk_price_volume_corr_dev(fmk_ctx *ctx, const double *d_price, const double *d_volume, int64_t n, int64_t window, double *d_out);
int fmk_price_volume_corr(fmk_ctx *ctx, const double *price, const double *volume, int64_t n, int64_t window, double *out);

/* ---- window statistics of finmlkit/feature/transforms.py on a float64 series of n elements -> float64 array of n elements
 * (csrc/fmk_shape.hip): KurtosisTransform (:900-933), TrendSlope (:936-988), HurstExponent (:1341-1397), BiPowerVariation (:1551-1602).
 * Every window is recomputed on its own.  A window that reads a NaN or an infinity gives NaN; window > n gives NaN everywhere.
 *   kurtosis  t >= window - 1 over x[t-window+1 .. t]: m4 / (m2 * m2) - 3 of the biased central moments; NaN where the window's
 *             elements all compare equal (==), whatever the rounded mean is, and where m2 == 0.
 *   slope     t >= window - 1: the least-squares slope of ln x on 0 .. window-1 as an angle, atan(slope) * 180 / pi; a price that is
 *             not finite and > 0 gives NaN; window 1 gives NaN.
 *   hurst     t >= window - 1, window >= 9: with tau_k the population standard deviation of the window - k sums of k consecutive
 *             elements of x[t-window+2 .. t], k = 1, 2, 4, 8: the least-squares slope of ln tau_k on ln k where all four are > 0,
 *             NaN otherwise (everywhere at window 9), and NaN where for some k those window - k sums, as held in float64 (a tree,
 *             oldest first inside a pair), all compare equal.  x[t-window+1] enters no sum and must be finite all the same.
 *   bipower   t >= window over x[t-window .. t]: sqrt(pi / 2) * the sum of |x[j]| * |x[j-1]|, j = t-window+1 .. t.
 * The reference's values within the tolerances of tests/golden/shape.json, its NaN positions exactly --
 * except, on purpose, that a window without a statistic (a held price: the two NaN rules above) gives NaN where the reference may
 * return rounding noise; elsewhere the exact value within the per-family tolerances of tests/golden/shape_degenerate.json.
 * FMK_E_ARG, checked before a device is touched and before any pointer is looked at: window < 1 (the reference returns all NaN or
 * zeros there), hurst with window < 9 (the reference raises TypeError), n >= 2^31. */
int fmk_rolling_kurtosis_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out);
int fmk_rolling_kurtosis(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out);
int fmk_trend_slope_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out);
int fmk_trend_slope(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out);
int fmk_hurst_exponent_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out);
int fmk_hurst_exponent(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out);
int fmk_bipower_variation_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, double *d_out);
int fmk_bipower_variation(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out);

/* ---- rolling approximate entropy of a float64 series of n elements -> float64 array of n elements (csrc/fmk_entropy.hip): the
 * reference's ApproximateEntropy transform (transforms.py:1400-1457), antropy.app_entropy(x, order=m, metric="chebyshev",
 * tolerance=tolerance * std(x)) on every window.  For t >= window - 1 over x[t-window+1 .. t], written x_0 .. x_{w-1}:
 *   r = tolerance * the window's population standard deviation; for k in (m, m + 1) the N_k = window - k + 1 vectors
 *   (x_i .. x_{i+k-1}); C_k[i] = the number of j with max_q |x_{i+q} - x_{j+q}| <= r (inclusive, j = i counts);
 *   phi_k = mean_i ln(C_k[i] / N_k); out[t] = phi_m - phi_{m+1}, which can be negative.
 * NaN before the first full window and in every window that reads a NaN or an infinity; window > n gives NaN everywhere.  A window
 * in which every pair matches (a constant one; tolerance 0 means only equal values match) gives exactly 0.0.  The published
 * algorithm within the tolerance of tests/golden/entropy.json, NaN positions exactly.  O(n * window^2).
 * FMK_E_ARG, checked in this order before a device is touched and before any pointer is looked at: m < 1, m > 4, window < m + 1,
 * window > 1024, tolerance negative, NaN or infinite; n >= 2^31. */
int fmk_approximate_entropy_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int64_t window, int64_t m, double tolerance, double *d_out);
int fmk_approximate_entropy(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, int64_t m, double tolerance, double *out);

/* ---- bar-clock, run-length and opening-range features (csrc/fmk_clock.hip): the reference's BarDuration, BarDurationEWMA,
 * BarRate, DirRunLen and ORBBreak transforms (transforms.py:1511-1548, :1460-1508, :1210-1270, :1605-1664, :1122-1207) on series of
 * n elements.  ts: int64 nanoseconds, non-decreasing (unsorted stamps: undefined, as for comp_lagged_returns).
 *   bar_duration:      out[i] = (double)(ts[i] - ts[i - periods]) / 1e9 where 0 <= i - periods < n, NaN elsewhere; any periods
 *                      (pandas' diff).  The reference's bits.
 *   bar_duration_ewma: out[0] = NaN; from element 1 on ewma's recursion over the durations d[t] = (double)(ts[t] - ts[t-1]) / 1e9,
 *                      seeded (d[1], 1) at element 1: u = d[t] + (1 - alpha) * u, v = 1 + (1 - alpha) * v, out = u / v, alpha =
 *                      2 / (span + 1).  A device-wide scan like ewma: within 1e-9 relative of pandas' ewm(span, adjust=True).mean().
 *   bar_rate:          lb(i) = the first j with ts[j] >= ts[i] - window_ns (on int64); out[i] = (double)(i - lb(i) + 1) / window_sec
 *                      * 3600.0.  window_ns is pd.Timedelta(seconds=window_sec).value, computed by the caller.  The reference's
 *                      bits (rolling(window, closed='both').sum() / window_sec * 3600), duplicate stamps included.
 *   dir_run_len:       s = sign(x) (-0.0 is zero, +-inf is +-1, NaN is unequal to everything).  out[0] = 0; for i >= 1 out[i] = 0
 *                      where s[i] == 0, else i - h(i) + 1 with h(i) the last j <= i that starts a run: j == 1, s[j] != s[j-1] or
 *                      s[j] NaN.  Stored as the low 8 bits (int8): a run of 128 reads -128, one of 256 reads 0.
 *   orb_break:         day(i) = floor(ts[i] / 86 400e9); s(i) = the first row of i's day.  Where ts[s] - day * 86 400e9 < 60e9 and
 *                      i - s >= 4: orb_long[i] = close[i] > max(high[s .. s+3]), orb_short[i] = close[i] < min(low[s .. s+3]), max
 *                      and min skipping NaN (all four NaN: no signal); 0 elsewhere.  uint8 outputs.  Strictly increasing stamps.
 * dir_run_len and orb_break run the last-head scan of csrc/fmk_lasthead.h (three launches, 4 bytes of scratch per 2048 elements).
 * FMK_E_ARG, checked before a device is touched and before any pointer is looked at: span < 1, window_ns < 1, n >= 2^31. */
int fmk_bar_duration_dev(fmk_ctx *ctx, const int64_t *d_ts, int64_t n, int64_t periods, double *d_out);
int fmk_bar_duration(fmk_ctx *ctx, const int64_t *ts, int64_t n, int64_t periods, double *out);
int fmk_bar_duration_ewma_dev(fmk_ctx *ctx, const int64_t *d_ts, int64_t n, double span, double *d_out);
int fmk_bar_duration_ewma(fmk_ctx *ctx, const int64_t *ts, int64_t n, double span, double *out);
int fmk_bar_rate_dev(fmk_ctx *ctx, const int64_t *d_ts, int64_t n, double window_sec, int64_t window_ns, double *d_out);
int fmk_bar_rate(fmk_ctx *ctx, const int64_t *ts, int64_t n, double window_sec, int64_t window_ns, double *out);
int fmk_dir_run_len_dev(fmk_ctx *ctx, const double *d_x, int64_t n, int8_t *d_out);
int fmk_dir_run_len(fmk_ctx *ctx, const double *x, int64_t n, int8_t *out);
int fmk_orb_break_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_high, const double *d_low, const double *d_close, int64_t n,
                      uint8_t *d_orb_long, uint8_t *d_orb_short);
int fmk_orb_break(fmk_ctx *ctx, const int64_t *ts, const double *high, const double *low, const double *close, int64_t n,
                  uint8_t *orb_long, uint8_t *orb_short);
/* The tile sizes of these kernels, for callers that place work at tile edges: out4[0] elements per workgroup of the scans
 * (bar_duration_ewma, dir_run_len, orb_break), [1] tiles per trip of their aggregate scan, [2] rows per workgroup of bar_rate, [3] the
 * stamps bar_rate stages in LDS (a longer slice is searched in global memory).  Needs no context and no device. */
int fmk_clock_geometry(int64_t *out4);

/* ---- labels and sample weights on the tick tape: finmlkit/label/tbm.py, label/weights.py ------------------------
 * triple_barrier (tbm.py:11-158) on the raw tape.  Per event: label (side labels -1 / +1; meta labels 0 / 1 when d_side is given),
 * index of the first barrier touch, the return there and the max return / barrier ratio.  Labels, touch indices, returns and ratios
 * are the reference's bit for bit (the host's log: csrc/fmk_log.h).  d_side == NULL: side labels.  Events may come in any order.
 * An event whose window holds no later tick (t1_idx <= event_idx; the reference skips it and leaves its touch index
 * uninitialised) gets label 0, NaN return and ratio, and its own event_idx as touch index; *d_n_skipped (device int64, may be
 * NULL; the caller zeroes it) counts them.  Contract: prices finite and > 0, timestamps sorted.  FMK_E_ARG with the reference's
 * messages: vertical_barrier <= 0, min_ret < 0, no events; also an event index outside [0, n).
 * Two schedules (DESIGN.md "labels"): every tick of the path walked, or -- barriers hours long or disabled -- a (min, max) table of
 * log(close) per 1024 ticks built per call, so that only the block holding the first touch is opened.  The call chooses by the
 * ticks one vertical barrier spans at the tape's mean tick rate; it waits once, for that and for the index check.
 * Host flavour: *n_skipped (host int64, may be NULL too) receives the count. */
int fmk_triple_barrier_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_close, int64_t n, const int64_t *d_event_idx,
                           const double *d_targets, const int8_t *d_side, int64_t n_events, double bottom_mult, double top_mult,
                           double vertical_barrier_sec, double min_close_time_sec, double min_ret, int8_t *d_labels,
                           int64_t *d_touch_idx, double *d_ret, double *d_max_rb_ratio, int64_t *d_n_skipped);
int fmk_triple_barrier(fmk_ctx *ctx, const int64_t *ts, const double *close_, int64_t n, const int64_t *event_idx,
                       const double *targets, const int8_t *side, int64_t n_events, double bottom_mult, double top_mult,
                       double vertical_barrier_sec, double min_close_time_sec, double min_ret, int8_t *labels, int64_t *touch_idx,
                       double *ret, double *max_rb_ratio, int64_t *n_skipped);
/* trend_scanning (Lopez de Prado, Machine Learning for Asset Managers, ch. 5; the reference's label/trend_scanning.py is an empty
 * placeholder, so the definition is this project's: DESIGN.md "trend scanning") on any float64 series y of n elements.  From an event
 * t0, span L covers y[t0 .. t0+L-1] for L = min_len, min_len + step, ... <= max_len.  With d_j = y[t0+j] - y[t0], S1 = sum d_j,
 * Sx = sum j*d_j, S2 = sum d_j^2: Sxx = L(L^2-1)/12, Sxy = Sx - (L-1)/2*S1, Syy = S2 - S1^2/L, u = 1 - Sxy^2/(Sxx*Syy) and
 * t(L) = Sxy / sqrt(Sxx*Syy) * sqrt((L-2)/u), the t-value of the slope of the least-squares line through the span.  In this order:
 * a NaN in the span (or an infinity: the sums become NaN) -> t(L) is NaN and the span is never chosen; S2 == 0 (a constant span) ->
 * 0.0; u <= 2^-26 (an exact fit up to rounding) -> copysign(inf, Sxy).  Per event the span of largest |t| among the non-NaN ones,
 * the smallest L among equals (several +-inf included): label = sign of its t (-1, 0, 1), t_value = its t, touch_idx = t0 + L - 1,
 * ret = y[touch_idx] / y[t0] - 1.  ret, the special t-values and the count are exact; a finite t-value is a re-associated float64
 * sum (64-tick blocks plus a carry; the measured tolerance is in DESIGN.md).  Events may come in any order, duplicates included.
 * An event whose longest span does not fit (t0 + max_len > n) or all of whose spans are NaN gets label 0, NaN t-value and return
 * and its own event_idx as touch index; *d_n_skipped (device int64, may be NULL; the caller zeroes it) counts them, as
 * fmk_triple_barrier_dev counts its window-less events.  FMK_E_ARG: min_len < 3, max_len < min_len, step < 1, an event index outside
 * [0, n).  n_events == 0 is a valid empty call.  One wave per event reads 8 B x max_len; the call waits once, for the index check.
 * Host flavour: *n_skipped (host int64, may be NULL too) receives the count. */
int fmk_trend_scanning_dev(fmk_ctx *ctx, const double *d_y, int64_t n, const int64_t *d_event_idx, int64_t n_events,
                           int64_t min_len, int64_t max_len, int64_t step, int8_t *d_labels, double *d_t_value,
                           int64_t *d_touch_idx, double *d_ret, int64_t *d_n_skipped);
int fmk_trend_scanning(fmk_ctx *ctx, const double *y, int64_t n, const int64_t *event_idx, int64_t n_events, int64_t min_len,
                       int64_t max_len, int64_t step, int8_t *labels, double *t_value, int64_t *touch_idx, double *ret,
                       int64_t *n_skipped);
/* The concurrency column of average_uniqueness (weights.py:31-38): how many events [event_idx, touch_idx] cover each tick, int16
 * with the reference's wrap-around.  n_events == 0: a zero column.  FMK_E_ARG: an event outside 0 <= event_idx <= touch_idx < n
 * (the reference slices silently into something else there). */
int fmk_label_concurrency_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, int64_t n_events, int64_t n,
                              int16_t *d_concurrency);
int fmk_label_concurrency(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, int64_t n_events, int64_t n,
                          int16_t *concurrency);
/* average_uniqueness' weights (weights.py:41-47: mean of 1 / concurrency over the event) and return_attribution without its
 * normalisation (weights.py:76-94: |sum of log(close[j] / close[j-1]) / concurrency[j]|) from ONE pass over close + concurrency
 * (10 B/tick) that leaves per-block partial sums.  Either output may be NULL; d_close may be NULL when d_return_attribution is.
 * Re-associated float64 sums (1e-9 relative for the positive terms of the first; the second within L * 2^-52 * sum|term|).
 * FMK_E_ARG: an event outside 0 <= event_idx <= touch_idx < n. */
int fmk_label_weights_dev(fmk_ctx *ctx, const double *d_close, const int16_t *d_concurrency, int64_t n, const int64_t *d_event_idx,
                          const int64_t *d_touch_idx, int64_t n_events, double *d_avg_uniqueness, double *d_return_attribution);
int fmk_label_weights(fmk_ctx *ctx, const double *close_, const int16_t *concurrency, int64_t n, const int64_t *event_idx,
                      const int64_t *touch_idx, int64_t n_events, double *avg_uniqueness, double *return_attribution);
/* The sequential bootstrap (Lopez de Prado, Advances in Financial Machine Learning, section 4.5; the reference has no such function:
 * the definition is this project's; csrc/fmk_seqboot.hip, csrc/fmk_seqboot_rule.h).  Events i = 0 .. m-1 with
 * spans [event_idx[i], touch_idx[i]] on an axis of n positions, in any order, duplicates included; n_draws = K draws per run, n_runs
 * = R independent runs.  The definition is in unsigned integers, so every sum is exact and the output does not depend on any tiling.
 * Per run r, with c_t the number of earlier draws of the run whose span covers position t:
 *   w(c) = floor(2^30 / (c + 1));  S_i = sum of w(c_t) over the span of i;  L_i = its length;  Q_i = floor(S_i / L_i), the average
 *   uniqueness of candidate i, itself counted, in units of 2^-30;  T = sum of all Q_i;
 *   the word of draw k: words[r*K + k] when words is given, else z = seed + (r*K + k + 1) * 0x9E3779B97F4A7C15 (mod 2^64) through
 *   the splitmix64 finaliser (z = (z ^ z>>30) * 0xBF58476D1CE4E5B9, z = (z ^ z>>27) * 0x94D049BB133111EB, word = z ^ z>>31);
 *   target = the high 64 bits of word * T;  draw k = the smallest i with Q_0 + .. + Q_i > target;  then c_t += 1 over its span.
 * draws[r*K + k] = the drawn event's position in the event arrays; q[r*K + k] (may be NULL) = its Q when it was drawn.
 * FMK_E_ARG outside 1 <= m <= 2^31 - 1, 1 <= K <= 2^24, 1 <= R with R*K <= 2^40, n <= 2^32 (they keep every sum inside 64 bits and
 * every Q positive), for draws_per_launch < 0, and for an event outside 0 <= event_idx <= touch_idx < n.  FMK_E_NOMEM when the
 * scratch does not fit: 4 bytes per interval and per event and run, 8 more per interval and run beyond the intervals that fit in
 * LDS (fmk_seqboot_geometry), with at most 2^32 - 1024 intervals between the span boundaries (the kernel's positions are 32-bit).
 * The axis is compressed to the intervals between span boundaries on the HOST, inside both entry points: the _dev flavour reads the
 * two index arrays back for it (16 bytes per event, nothing of a tape) and so waits for the stream; d_words, d_draws and d_q are
 * device arrays.  One workgroup per run; the draws go out in launches of draws_per_launch draws each (0: the library's choice), the
 * concurrency persists in device memory in between, and the split changes nothing in the output. */
int fmk_sequential_bootstrap_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, int64_t n_events, int64_t n,
                                 int64_t n_draws, int64_t n_runs, uint64_t seed, const uint64_t *d_words, int64_t draws_per_launch,
                                 int64_t *d_draws, int64_t *d_q);
int fmk_sequential_bootstrap(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, int64_t n_events, int64_t n,
                             int64_t n_draws, int64_t n_runs, uint64_t seed, const uint64_t *words, int64_t draws_per_launch,
                             int64_t *draws, int64_t *q);
/* The kernel's geometry, for callers that place work at its seams: out3[0] threads of a workgroup (an event or interval count past a
 * multiple of it gives the last thread a shorter run), [1] the intervals that fit in LDS (more: the scratch flavour), [2] the draws
 * per launch when draws_per_launch is 0.  Needs no context and no device. */
int fmk_seqboot_geometry(int64_t *out3);

/* ---- optimal trading rules (Lopez de Prado, Advances in Financial Machine Learning, ch. 13, snippets 13.1 / 13.2; the reference has no
 * such function: the definition is this project's; csrc/fmk_otr.hip, csrc/fmk_otr_rule.h).  Paths of a discrete
 * Ornstein-Uhlenbeck process are closed at a profit-taking level, a stop-loss level or a maximum holding period, for every pair
 * (pt[i], sl[j]) of a mesh; the outputs are the statistics of the closing values.  A result is a function of the arguments alone, bit
 * for bit, on any device and on the host (tools/otr_check.cpp runs the same rule text).
 *   Inputs: n_cfg parameter sets (forecast[c], phi[c], sigma[c]), all finite, 0 <= phi <= 1, sigma >= 0; pt[0 .. n_pt) and
 *     sl[0 .. n_sl), each non-negative, non-decreasing, without NaN (+inf: the barrier is off); max_hp, n_paths, seed; normals: NULL,
 *     or a HOST array [n_paths][max_hp] of finite float64 that replaces the generator.
 *   Limits: 1 <= n_pt, n_sl <= 32, 1 <= max_hp <= 4096, 1 <= n_paths <= 2^32, 1 <= n_cfg <= 1024; anything else is FMK_E_ARG.
 *   Normal variates (Marsaglia's polar method on counter words): path p takes step h = 1 .. max_hp from pair k = (h-1) >> 1, member
 *     (h-1) & 1.  For attempt a = 0 .. 63: index = ((((p << 12) | k) << 6 | a) << 1) | w (w = 0 for u, 1 for v); word = splitmix64 at
 *     counter index + 1 from seed (the bootstrap's word); u = (double)(word >> 11) * 2^-52 - 1.0 (exact, in [-1, 1)); s = u*u + v*v (the
 *     products and the sum rounded separately); the first attempt with s < 1.0 && s != 0.0 is taken: f = sqrt((-2.0 * log(s)) / s)
 *     with the host's logarithm, the pair is (u*f, v*f).  After 64 rejections the pair is (0.0, 0.0).  The variates depend on
 *     (seed, p, h) only: all parameter sets of a call see the same random numbers.
 *   Path: c0 = (1.0 - phi) * forecast, P_0 = 0.0, P_h = (c0 + phi * P_{h-1}) + sigma * z_h, every operation rounded on its own.
 *   Exit of node (i, j): the smallest h with P_h > pt[i] (profit) or P_h < -sl[j] (stop), strict, else max_hp (time); x = P_h there.  A
 *     crossing at h = max_hp counts as the barrier's.
 *   Sums: paths are cut into blocks [b B, (b+1) B), B a constant of the library (fmk_otr_geometry).  Per node and block
 *     S1_b = (((0 + x_0) + x_1) + ...) in path order, S2_b the same with x*x (the product rounded, then added); the totals are the
 *     left-to-right sums of the block partials in block order.  mean = S1 / n; var = S2 / n - mean*mean, 0.0 when negative;
 *     std = sqrt(var); sharpe = mean / std with IEEE semantics (0/0 NaN, x/0 +-inf).
 *   Outputs, HOST arrays [n_cfg][n_pt][n_sl], each may be NULL: mean, std, sharpe (float64); n_profit, n_stop, n_time (their sum is
 *     n_paths) and hold, the sum of the exit steps (int64).
 * A host-pointer entry without a _dev flavour: the inputs are a few hundred bytes and the outputs a few KiB.  The arguments are
 * checked before a device is touched.  FMK_E_NOMEM when the scratch does not fit: 16 bytes per node and block of one parameter set
 * (several sets share a launch while their partials stay under 256 MiB), 8 bytes per normal. */
int fmk_otr_mesh(fmk_ctx *ctx, const double *forecast, const double *phi, const double *sigma, int64_t n_cfg, const double *pt,
                 int64_t n_pt, const double *sl, int64_t n_sl, int64_t max_hp, int64_t n_paths, uint64_t seed, const double *normals,
                 double *mean, double *std, double *sharpe, int64_t *n_profit, int64_t *n_stop, int64_t *n_time, int64_t *hold);
/* The kernel's geometry, for callers that place work at its seams: out4[0] B, the paths of a block of the sums, [1] the paths of a
 * tile (walked at once, one per lane), [2] the most levels on either side, [3] the largest max_hp.  Needs no context and no device. */
int fmk_otr_geometry(int64_t *out4);

/* ---- bet sizing (Lopez de Prado, Advances in Financial Machine Learning, ch. 10, snippets 10.1 - 10.3 and section 10.2; the
 * reference has no such function: the definition is this project's; csrc/fmk_bet.hip, csrc/fmk_bet_rule.h).
 * From the signals of the events to the position per tick of the tape: the average of the signals of the bets still open.
 *   Spans: event i is open on the ticks event_idx[i] <= t < touch_idx[i] -- the bet is closed AT the touch (the book's
 *     index <= loc < t1), which is not the closed range fmk_label_concurrency counts.  touch_idx[i] == event_idx[i] (a skipped
 *     label) is never open.  Events in any order, duplicates included.  1 <= n_events <= 2^31 - 1, 1 <= n <= 2^32.
 *   Signal: float64 in [-1, 1], counted in units of 2^-30: q_i = rint(signal[i] * 2^30), an exact product with one rounding, ties to
 *     even.
 *   Value: c[t] the number of open events at tick t, S[t] the sum of their q_i (an integer).  value[t] = fl(S[t] / c[t]) * 2^-30
 *     where c[t] > 0 -- one correctly rounded division, the scaling is exact -- and +0.0 where c[t] == 0; -0.0 never appears here.
 *     out_count (int16, may be NULL) receives c[t].
 *   Discretisation: step == 0: none; 0 < step <= 1: value = min(1, max(-1, rint(value / step) * step)), each operation rounded
 *     on its own (NumPy's bits).
 * The sums are integer sums made with integer atomics, so a result is a function of the arguments alone, bit for bit, run to run.
 * FMK_E_ARG, before a device is touched: n_events or n outside the bounds, a step that is neither 0 nor in (0, 1].  FMK_E_ARG, counted
 * on the device (the message holds the count; the outputs are then undefined): an event outside 0 <= event_idx <= touch_idx < n, a
 * signal that is NaN or outside [-1, 1], a concurrency above 32767 on any tick (the message holds the largest).  The sum and the
 * count are carried in an int64 and an int32 of their own, which cannot wrap below 2^31 events: the last refusal is certain for every
 * n_events.  Scratch: 12 bytes per tick (rounded up to a tile), freed in the stream's order; the call waits once, for the mailbox. */
int fmk_bet_size_path_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, const double *d_signal,
                          int64_t n_events, int64_t n, double step, double *d_out_value, int16_t *d_out_count);
int fmk_bet_size_path(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, const double *signal, int64_t n_events,
                      int64_t n, double step, double *out_value, int16_t *out_count);
/* out[k] = value[idx[k]] of the path above, k = 0 .. n_idx - 1: the path (8 more bytes per tick) is a temporary of the call.  n_idx ==
 * 0 is a valid call that still checks the events.  FMK_E_ARG as above, and for an index outside [0, n) (counted on the device). */
int fmk_bet_size_at_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, const double *d_signal,
                        int64_t n_events, int64_t n, double step, const int64_t *d_idx, int64_t n_idx, double *d_out);
int fmk_bet_size_at(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, const double *signal, int64_t n_events,
                    int64_t n, double step, const int64_t *idx, int64_t n_idx, double *out);
/* The budget approach (section 10.2).  side: int8 per event; cl[t] / cs[t] = the open events (spans as above) with side > 0 /
 * side < 0, side 0 counts nowhere; Ml = max_t cl[t], Ms = max_t cs[t];
 *   out_m[t] = (Ml ? fl(cl[t] / Ml) : 0) - (Ms ? fl(cs[t] / Ms) : 0),   out_max2 (int64[2], may be NULL) = {Ml, Ms}.
 * FMK_E_ARG: the bounds of n_events and n, an event outside the tape, Ml or Ms above 32767.  Scratch: 8 bytes per tick. */
int fmk_bet_size_budget_dev(fmk_ctx *ctx, const int64_t *d_event_idx, const int64_t *d_touch_idx, const int8_t *d_side,
                            int64_t n_events, int64_t n, double *d_out_m, int64_t *d_out_max2);
int fmk_bet_size_budget(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, const int8_t *side, int64_t n_events,
                        int64_t n, double *out_m, int64_t *out_max2);
/* The kernels' geometry, for callers that place work at its seams: out3[0] the ticks of a tile (one workgroup), [1] the ticks of a
 * row (one workgroup scan; a thread owns 4 consecutive ticks of it), [2] the tiles of one trip of the aggregate scan.  Needs no
 * context and no device. */
int fmk_bet_geometry(int64_t *out3);

/* ---- causal FIR filter on a float64 series of n elements -> float64 array of n elements (csrc/fmk_fir.hip), and with the weights
 * of feature/core/fracdiff.py the fixed-width window fractional differentiation "FFD" (Lopez de Prado, Advances in Financial
 * Machine Learning, ch. 5; the reference has no such function: the definition is this project's).
 * w[0 .. width-1] is a HOST array in both flavours (at most 64 KiB; the call checks it and copies it to the device in the stream's
 * order); w[k] multiplies x[t-k].  With x~[i] = x[i] where x[i] is finite and NaN elsewhere:
 *   out[t] = NaN for t < width - 1;
 *   out[t] = acc after  acc = +0.0;  for k = width-1, width-2, .. 0: acc = fma(w[k], x~[t-k], acc)
 * -- one correctly rounded fused multiply-add per tap, oldest tap first, one chain per output.  So a NaN or an infinity anywhere in
 * x[t-width+1 .. t] makes out[t] NaN, n < width gives NaN everywhere, and the bits depend on nothing but x and w: not on the tile, on
 * the taps per staging pass (fmk_fir_geometry) or on the pointers' alignment beyond 8 bytes.  n == 0 succeeds and touches nothing.
 * FMK_E_ARG, checked in this order before a device is touched and before x or out is looked at: width < 1, width > 8192, a weight
 * that is not finite, out == x; then n >= 2^31. */
int fmk_fir_dev(fmk_ctx *ctx, const double *d_x, int64_t n, const double *w, int64_t width, double *d_out);
int fmk_fir(fmk_ctx *ctx, const double *x, int64_t n, const double *w, int64_t width, double *out);
/* The kernel's geometry, for callers that place work at its seams: out2[0] outputs per workgroup, [1] taps per staging pass.  Needs
 * no context and no device. */
int fmk_fir_geometry(int64_t *out2);

/* ---- augmented Dickey-Fuller statistic of backward windows and its supremum, SADF (csrc/fmk_sadf.hip; Lopez de Prado, Advances in
 * Financial Machine Learning, ch. 17; the reference has no such function: the definition is this project's).
 * y: any float64 series of n elements, taken as given (pass log prices); an element that is not finite counts as NaN.  L = lags in
 * 0..4, trend FMK_ADF_C or FMK_ADF_CT.  With dy_i = y_i - y_{i-1}, row i (i >= L + 1) of END POINT t has the target dy_i and the
 * k = L + 2 (+ 1 for CT) regressors, in the order of the factor,
 *   1, (i - t if CT), dy_{i-1}, .., dy_{i-L}, y_{i-1} - y_t
 * (centring the level on y_t and the trend on t changes neither the coefficient of the level nor its t-statistic: there is an
 * intercept; it keeps float64 moments usable at price levels of 10^5 and is part of the definition).  A window is the m rows
 * i in [s, t], s = t - m + 1 >= L + 1; it reads y[s-L-1 .. t].  A = the (k+1) x (k+1) matrix of the window's moments (sums of
 * products of the columns above, the target as the last row and column; the moments of 1 and i - t alone are m, -m(m-1)/2 and
 * (m-1)m(2m-1)/6).  For j = 0 .. k-1: d_j = A[j][j]; the window is DEGENERATE when !(d_j > 2^-26 * G_jj), G_jj the moment A[j][j]
 * started as; then for i > j: l = A[i][j] * (1 / d_j), A[i][r] -= l * A[r][j] for r = j+1 .. i.  This leaves SSR = A[k][k]; with
 * z = A[k][k-1] and d = A[k-1][k-1]:
 *   ADF(s, t) = z / sqrt(d * SSR / (m - k));      SSR / (sum of dy_i^2) <= 2^-26 (an exact fit) -> copysign(inf, z).
 * A degenerate window (a constant stretch, an exact ramp under CT or with lags, collinear lags) and a window that holds a NaN (its
 * sums are NaN and fail the pivot test) are never chosen.  stat[e] = the largest ADF(s, t) over m = min_len, min_len + step, ..
 * <= max_len with s >= L + 1, start[e] = the s of that window, the shortest window among equal statistics (several +inf included);
 * an end point without a usable window gets NaN and -1, and *d_n_skipped (device int64, may be NULL; the caller zeroes it) counts
 * them.  min_len == max_len is the rolling ADF; one end point n-1 with min_len = max_len = n-L-1 the ADF of the whole series.
 * d_end_idx: n_end end points in any order, duplicates included; NULL: end point e is element e (n_end = n: every t).  The special
 * values and the count are exact; a finite statistic is float64 arithmetic on re-associated sums (64-row blocks plus a carry; the
 * measured tolerance is in DESIGN.md).  FMK_E_ARG, the rules before a device is touched, in this order: lags outside 0..4, an
 * unknown trend, min_len < k + 1, max_len < min_len, step < 1, d_stat or d_start == d_y; then an end point outside [0, n).
 * n_end == 0 is a valid empty call.  One wave per end point; the call waits once, for the index check.  Host flavour: *n_skipped
 * (host int64, may be NULL too) receives the count, end_idx may be NULL as above. */
#define FMK_ADF_C 0
#define FMK_ADF_CT 1
int fmk_sadf_dev(fmk_ctx *ctx, const double *d_y, int64_t n, const int64_t *d_end_idx, int64_t n_end, int64_t min_len,
                 int64_t max_len, int64_t step, int64_t lags, int trend, double *d_stat, int64_t *d_start, int64_t *d_n_skipped);
int fmk_sadf(fmk_ctx *ctx, const double *y, int64_t n, const int64_t *end_idx, int64_t n_end, int64_t min_len, int64_t max_len,
             int64_t step, int64_t lags, int trend, double *stat, int64_t *start, int64_t *n_skipped);

/* ---- entropy of an encoded series (csrc/fmk_lz.hip; Lopez de Prado, Advances in Financial Machine Learning, ch. 18; the reference
 * has no such functions: the definitions are this project's).  A message is a uint8 array of codes; a code
 * >= alphabet is INVALID and 255 always is (the match lengths and the Kontoyiannis estimator take no alphabet: 255 alone).  A window
 * that reads an invalid code gives NaN.  n == 0 succeeds and touches nothing, not even the context.
 *
 * encode: codes[i] = the number of edges <= x[i] (np.searchsorted(edges, x, side="right"); -inf 0, +inf n_edges), 255 for a NaN.
 * edges[0 .. n_edges) is a HOST array in both flavours (the call checks it and copies it to the device in the stream's order); the
 * alphabet is n_edges + 1.  FMK_E_ARG, in this order: n_edges < 1, n_edges > 254, an edge that is not finite, edges that are not
 * strictly increasing; then n >= 2^31.
 *
 * plugin_entropy, bits per symbol: the window codes[t-window+1 .. t] holds M = window - word + 1 overlapping words of `word` codes;
 * c(v) = the count of word v;  out[t] = (sum over the words v, ascending in their id, of c(v) * (log2 M - log2 c(v))) / M / word
 * -- which is (log2 M - (1/M) sum_c N_c log2 c) / word with N_c the occurrences whose word has count c, and -sum p log2 p / word.
 * log2 M - log2 c is one table entry, 0.0 at c = M: a window whose words are all the same gives exactly 0.0.  NaN for t < window - 1.
 * The bits depend on codes, window, word and alphabet alone.  FMK_E_ARG, in this order: alphabet outside 2..255, word < 1,
 * alphabet^word > 4096, window < word, window > 4096; then n >= 2^31.
 *
 * match_lengths (n = lookback, N = the series' length): for n <= p <= N - n whose codes[p-n .. p+n) are all valid
 *   len[p] = 1 + max over d = 1 .. n of min(n, the number of k >= p in a row with codes[k] == codes[k-d])
 * (a match may run over p itself; len[p] lies in 1 .. n + 1); len[p] = 0 everywhere else.  The work is the same whatever the data.
 * FMK_E_ARG: lookback outside 1..1024; then N >= 2^31.
 *
 * kontoyiannis_entropy, bits per symbol (the sliding-window form of the book's snippet 18.4): with count = window - 2n + 1
 *   out[t] = (log2(n + 1) / count) * (1/len[t-window+1+n] + .. + 1/len[t-n+1]),   the sum oldest first, each quotient rounded
 * NaN for t < window - 1 and where one of those len is 0: exactly the windows that read an invalid code.  len is scratch from the
 * context's pool.  FMK_E_ARG, in this order: lookback outside 1..1024, window < 2 * lookback, window > 4096; then N >= 2^31. */
int fmk_encode_dev(fmk_ctx *ctx, const double *d_x, int64_t n, const double *edges, int64_t n_edges, uint8_t *d_codes);
int fmk_encode(fmk_ctx *ctx, const double *x, int64_t n, const double *edges, int64_t n_edges, uint8_t *codes);
int fmk_plugin_entropy_dev(fmk_ctx *ctx, const uint8_t *d_codes, int64_t n, int64_t window, int64_t word, int64_t alphabet,
                           double *d_out);
int fmk_plugin_entropy(fmk_ctx *ctx, const uint8_t *codes, int64_t n, int64_t window, int64_t word, int64_t alphabet, double *out);
int fmk_match_lengths_dev(fmk_ctx *ctx, const uint8_t *d_codes, int64_t n, int64_t lookback, uint16_t *d_len);
int fmk_match_lengths(fmk_ctx *ctx, const uint8_t *codes, int64_t n, int64_t lookback, uint16_t *len);
int fmk_kontoyiannis_entropy_dev(fmk_ctx *ctx, const uint8_t *d_codes, int64_t n, int64_t window, int64_t lookback, double *d_out);
int fmk_kontoyiannis_entropy(fmk_ctx *ctx, const uint8_t *codes, int64_t n, int64_t window, int64_t lookback, double *out);

/* ---- TradesData(preprocess=True) loops: finmlkit/bar/utils.py ("next" rank 4) ------------ */
/* merge_split_trades (bar/utils.py:263-329): trades with the head's timestamp, maker flag and price (|dp| < 1e-8)
 * are merged, amounts summed in float32 in trade order; side = -1 if is_buyer_maker else 1 (is_buyer_maker may be
 * NULL: no side output).  *n_merged receives the number of merged trades; pass out_ts == NULL to only count.
 * FMK_E_CAPACITY when capacity < *n_merged. */
int fmk_merge_split_trades_dev(fmk_ctx *ctx, const int64_t *d_ts, const double *d_price, const float *d_amount,
                               const uint8_t *d_is_buyer_maker, int64_t n, int64_t *d_out_ts, double *d_out_price,
                               float *d_out_amount, int8_t *d_out_side, int64_t capacity, int64_t *n_merged);
int fmk_merge_split_trades(fmk_ctx *ctx, const int64_t *ts, const double *price, const float *amount,
                           const uint8_t *is_buyer_maker, int64_t n, int64_t *out_ts, double *out_price,
                           float *out_amount, int8_t *out_side, int64_t capacity, int64_t *n_merged);
/* comp_trade_side_vector (bar/utils.py:26-46): tick rule, side[0] = 0. */
int fmk_comp_trade_side_vector_dev(fmk_ctx *ctx, const double *d_price, int64_t n, int8_t *d_out);
int fmk_comp_trade_side_vector(fmk_ctx *ctx, const double *price, int64_t n, int8_t *out);

/* ---- TimeBarReader._resample: finmlkit/bar/io.py:890-950 ("next" rank 4, second half) --------------------------
 * Bars -> coarser bars.  Group g covers the rows [seg[g], seg[g+1]) of the input frame (contiguous; the host computes the
 * groups with pandas' own index.floor(timeframe)).  Per group: open = first / close = last non-NaN, high = max, low = min,
 * volume = pandas' Kahan-compensated sum in the column's dtype (float32 stays float32), trades = integer sum,
 * vwap = float32(sum(vwap * volume) / sum(volume)) with NumPy's dtype promotion of the product, median_trade_size =
 * float32 of the trades-weighted median of the rows' medians (searchsorted(cumsum(w), total / 2, 'left')).
 * o_valid[g] = 0 where every open of the group is NaN (the reference drops those rows, io.py:948). */
int fmk_resample_bars_dev(fmk_ctx *ctx, const int64_t *d_seg, int64_t n_groups, const double *d_open, const double *d_high,
                          const double *d_low, const double *d_close, const void *d_volume, int volume_is_f64,
                          const int64_t *d_trades, const void *d_vwap, int vwap_is_f64, const double *d_median,
                          double *d_o_open, double *d_o_high, double *d_o_low, double *d_o_close, void *d_o_volume,
                          int64_t *d_o_trades, float *d_o_vwap, float *d_o_median, uint8_t *d_o_valid);
int fmk_resample_bars(fmk_ctx *ctx, const int64_t *seg, int64_t n_groups, int64_t n_rows, const double *open,
                      const double *high, const double *low, const double *close, const void *volume, int volume_is_f64,
                      const int64_t *trades, const void *vwap, int vwap_is_f64, const double *median, double *o_open,
                      double *o_high, double *o_low, double *o_close, void *o_volume, int64_t *o_trades, float *o_vwap,
                      float *o_median, uint8_t *o_valid);

/* ---- multi-GPU: one neighbour halo exchange per step (BASELINE cfg 5) ------------------------
 * The reference has no distributed code (last row); these entry points are new.  Rank r of `world` holds
 * a contiguous tick range of one stream; the trailing partial bar of rank r travels as raw ticks to rank r+1.
 * No PyTorch: librccl is dlopen'ed by fmk_comm_create(FMK_COMM_RCCL) and the ranks of the node meet in a shared-memory
 * file (`rendezvous_path`, the same string on every rank; rank 0 creates it and unlinks it once all have attached).
 * Every wait has a deadline (`timeout_s`, <= 0: 120 s): a missing peer is FMK_E_COMM, not a hang. */
typedef struct fmk_comm fmk_comm;
#define FMK_COMM_RCCL 0      /* ncclSend / ncclRecv over xGMI on the communicator's own stream */
#define FMK_COMM_HOST 1      /* host-staged through the rendezvous segment; ctx may be NULL (host pointers) */
#define FMK_COMM_SELF_LOOP 1 /* flags: with world == 1 the rank is its own left and right neighbour (diagnostic) */
int fmk_comm_create(fmk_ctx *ctx, int transport, const char *rendezvous_path, int rank, int world, int flags,
                    size_t ring_bytes /* host transport: bytes of each rank's receive ring, 0 = 1 MiB */,
                    double timeout_s, fmk_comm **out);
int fmk_comm_destroy(fmk_comm *comm);
const char *fmk_comm_last_error(const fmk_comm *comm);
/* Set-up phase, HOST buffers, blocking: `bytes` (<= 4096) from every rank, in rank order; barrier = empty gather. */
int fmk_comm_allgather(fmk_comm *comm, const void *send, size_t bytes, void *recv);
int fmk_comm_barrier(fmk_comm *comm);
/* One exchange: column slice i of `send_*` goes to rank+1 (ignored on the last rank), `recv_*` arrives from rank-1
 * (ignored on rank 0); sizes in bytes, zero-length columns allowed, both sides must agree on them.
 * RCCL: enqueued as ONE ncclGroup on the communicator's stream, which first waits (event) for everything already
 * enqueued on the context's stream; returns at once.  fmk_comm_wait_dev makes the context's stream wait (event) for
 * that exchange -- kernels enqueued between the two calls overlap it.  HOST: synchronous, complete on return. */
int fmk_comm_halo_exchange_dev(fmk_comm *comm, int n_cols, const void *const *send_ptrs, const size_t *send_bytes,
                               void *const *recv_ptrs, const size_t *recv_bytes);
int fmk_comm_wait_dev(fmk_comm *comm);
int fmk_comm_sync(fmk_comm *comm); /* host wait for the communicator's stream, bounded by timeout_s: FMK_E_COMM when the
                                      exchange has not completed by then (call it BEFORE fmk_ctx_sync when a peer may be gone) */
/* Per-exchange timing: the next <= 64 exchanges are timed on their own -- RCCL: a HIP event pair on the communicator's
 * stream around the ncclGroup (device time of the send/recv alone); HOST: wall clock of the staged copy. */
int fmk_comm_profile_enable(fmk_comm *comm, int on);
int fmk_comm_profile_read(fmk_comm *comm, double *ms, int capacity, int *count);
/* First contact with a node, as text: the devices this process sees, the peer-access matrix (hipDeviceCanAccessPeer), the librccl that
 * would be loaded and its version, the environment that decides how RCCL shares memory between processes.  Needs no context and no
 * GPU (`python -m finmlkit_amd.dist --selftest` prints it, bench.py logs it per rank when N > 1). */
int fmk_comm_describe(char *buf, size_t cap);
/* Up to 8 small device column slices copied by one launch on the context's stream (boundary-bar assembly). */
int fmk_copy_cols_dev(fmk_ctx *ctx, int n_cols, const void *const *src, void *const *dst, const size_t *bytes);

/* Diagnostics (bandwidth / latency probes, counters read by tests and tools) are NOT part of this ABI: include/fmk_diag.h. */

#ifdef __cplusplus
}
#endif
#endif /* FMK_H */
