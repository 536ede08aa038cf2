// fmk_common.h -- shared host/device helpers of the gfx950 tick->bar engine.
// gfx950 only: wave = 64 lanes everywhere, no portability shims.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/fmk.h"

#define FMK_WAVE 64
#define FMK_PROFILE_SLOTS 256              // launches fmk_profile_* can time between enable and read

// The context's mailbox: small flags / counters the kernels leave for the host.  One device copy (fmk_ctx::d_mail, hipMalloc) and
// one pinned host copy (fmk_ctx::h_mail, hipHostMalloc) of the same layout; every use has a field of its own, grouped by the file
// that owns it.  A sub-struct is what one memset or one read-back covers.
struct fmk_mail {
    // ---- fields that outlive the call that writes them
    // set by the device through the pinned host copy when a one-pass scan gives up waiting for another workgroup
    // (k_ew_onepass_d, fmk_ticklevel.hip); read and cleared by fmk_check_device_error (fmk_api.hip) on every fmk_ctx_sync
    int64_t device_error;
    // status of the volume prefix pass (k_vc_prefix in vol_chase, fmk_volume.hip); read again by the table tiers of a later
    // vol_chase(..., have_prefix = true) call on the same prefix (d_pstat)
    int vol_prefix_status;
    // [0] a bar beyond the in-sweep median's reach was met (flag of the call), [1] bars that took the generic selection (atomicAdd
    // by k_bar_footprints<MED>, fmk_footprint.hip); [1] is read by fmk_diag_fp_median_fallbacks after the call
    int fp_median[2];
    // host copy only: the list sizes of the last one-pass cfg 4 sizing call (fmk_barflow.hip, queued without a wait: the sizing
    // call waits later); read by fmk_diag_fused_last and by the fill call (n_fp).  mode: the schedule the last cfg 4 sizing call
    // took (0 two-pass, 1 / 2 one pass with / without the unit histogram), fill_staged: the last footprint fill consumed staged
    // rows -- both read by fmk_diag_fused_mode
    struct { int64_t n_fp, n_dir, n_redo, mode, fill_staged; } fused_last;

    // ---- per-call fields
    uint8_t staging[1024];                 // host copy: fmk_read_back's landing area
    struct Vol {                           // fmk_volume.hip / fmk_volume_exact.h / fmk_voltree.h: the level tables
        struct Levels { int status; uint32_t root; int root_tie; } lv;                          // k_vol_level0 / k_vx_level0 / k_vol_tree_up
        struct Table { uint32_t root; uint32_t maxlen; int status; unsigned long long nfrag; } tb;      // k_vg_* / k_vol_tree_up (vol_global_tables)
        struct Closes { uint32_t count; int status; } closes;                                   // host copy: vol_tree_closes' batch
        struct Chase { int64_t res; int prefix_status; } chase;                                 // host copy: vol_chase's batch
        int64_t chase_res;                 // k_vc_chase: closes (or the total, total_only)
        int mismatch;                      // k_vol_verify
    } vol;
    struct Fb {                            // fmk_flowbars.hip
        // k_fb_prefix: status bits, the tape's quantum as a binary exponent (atomicMin); k_fb_scan: the sum of |increment|;
        // k_fb_links / k_fb_root: the longest link, the first close; k_vol_tree_up: tree_status
        struct Tape { int status; int qexp; uint32_t maxlen; uint32_t root; double sum_abs; int tree_status; } tape;
        int64_t serial_count;              // k_fb_serial
    } fb;
    struct Dl {                            // fmk_dollar.hip
        struct Pass1 { int bad; unsigned long long dmax; double whale; double total[2] /* hi, lo; not cleared */; } p1;
        struct Emit { unsigned long long frag; int64_t res; unsigned long long area; } emit;       // res also: k_dl_scan_min
        struct One { int64_t last; unsigned long long frag; int flags; } one;                     // k_dl1
        double sample_sum;                 // k_dl1_sample
    } dl;
    struct { double total; int64_t res[2] /* count, uncertified */; } th;                      // fmk_threshold.hip
    struct Cusum {                         // fmk_cusum.hip
        struct Fill { unsigned long long first; long long nan_count; } ff;                      // k_ff_tile / k_ff_count
        struct Round { unsigned long long changed, pending, nan; } round;                       // k_cs1_fix / k_cusum_chunks
    } cusum;
    struct Fp {                            // fmk_footprint.hip
        unsigned long long max_levels;     // k_fp_level_counts
        struct Sizes { int64_t total; unsigned long long max; } sizes;                          // host copy
        int lds_probe;                     // k_fp_lds_order_probe
    } fp;
    struct { unsigned long long max; unsigned status; } vp;                                    // fmk_volprofile.hip
    // fmk_volprofile_dev.hip (k_vpd_replay): ~(range << 40 | bar of the range) of the first all-zero profile (atomicMax), status bits
    struct Vpd { unsigned long long zero_at; unsigned status; } vpd;
    struct Ohlcv {                         // fmk_ohlcv.hip
        int saw_long;                      // a bar longer than the small kernels take (also the pipelined step's host copy)
        int64_t span[3];                   // k_list_span: listed bars, first tick, last tick
        unsigned long long grid_mis[2];    // k_price_grid_build: ticks whose price form A / form B does not reproduce
    } ohlcv;
    struct Bf {                            // fmk_barflow.hip
        int fu_census[3];                  // k_fu_census: min low bit, max exponent, bad
        int fu_long[2];                    // FuLists::saw_long, FuLists::saw_huge
        int any_long;                      // k_bar_dir_lanes
        int saw_long;                      // k_bar_ohlcv_dir
    } bf;
    struct { unsigned long long sink; long long hops[2]; } diag;                               // fmk_diag.hip
    struct Label {                         // fmk_label.hip
        unsigned long long work;           // k_tb: next event of the persistent grid
        long long skipped, opened, walked; // k_tb: events without a window, blocks opened, ticks walked (fmk_diag_label_last)
        long long bad;                     // k_lb_precheck / k_lc_mark / k_lw_events: indices outside the tape
        int64_t ts_ends[2];                // k_lb_precheck: ts[0], ts[n-1] (the tape's tick rate)
        int64_t last[2];                   // host copy only: schedule (0 direct, 1 tables) and events of this context's last call
    } label;
    struct Trend {                         // fmk_trend.hip
        unsigned long long work;           // k_trend: next event of the persistent grid
        long long skipped;                 // k_trend: events whose longest span does not fit, or all of whose spans are NaN
        long long bad;                     // k_trend: event indices outside the series (the call fails)
    } trend;
    struct Sadf {                          // fmk_sadf.hip
        unsigned long long work;           // k_sadf: next end point of the persistent grid
        long long skipped;                 // k_sadf: end points without a usable window
        long long bad;                     // k_sadf: end-point indices outside the series (the call fails)
    } sadf;
    struct Brk {                           // fmk_break.hip
        int nonpos;                        // k_brk_log: an element <= 0
        unsigned long long pairs, skipped; // k_brk_pairs: (t, n) pairs walked, pairs the den <= 1e-16 test dropped
        int64_t last[4];                   // host copy only: outputs, slabs per tile span, slab elements, tiles of the last call
    } brk;
    struct Micro { int bad; } micro;       // fmk_micro.hip (k_micro_lanes): a bar's close indices outside the tape (the call fails)
    struct Bet {                           // fmk_bet.hip: each of them fails the call
        long long bad, bad_signal;         // k_bet_mark / k_bud_mark: spans outside the tape, signals that are NaN or outside [-1, 1]
        long long bad_idx;                 // k_bet_gather: indices outside the tape
        int max_c;                         // k_bet_apply: the largest concurrency above 32767 (0: none)
        int max2[2];                       // k_bud_scan: the largest long and short concurrency
        int pad;
    } bet;
};
static_assert(sizeof(fmk_mail::fp_median) == 2 * sizeof(int), "k_bar_footprints adds to saw_long + 1");
static_assert(alignof(fmk_mail) == 8, "the 64-bit atomics of the kernels need 8-byte fields");

struct fmk_ctx {
    int device;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    char err[512];
    // grow-on-demand device scratch (scan partials, flags)
    void *scratch;
    size_t scratch_bytes;
    // the mailbox (fmk_mail): pinned host copy, device copy
    fmk_mail *h_mail;
    fmk_mail *d_mail;
    int n_cu;
    // per-launch timing of the dominant kernel (fmk_profile_enable)
    int profile_on, profile_n;
    // threshold indexers: 0 (default) = inputs with uncertified decisions are redone by the exact sequential loop;
    // 1 = return the parallel result with its n_uncertified (fmk_ctx_set_fast_threshold)
    int fast_threshold;
    // 1 = calls never wait for the device where they have the choice (fmk_ctx_set_enqueue_only)
    int enqueue_only;
    // 1 (default) = the OHLCV entry points that are handed a certified price grid read it; 0 = they take the float64 column
    // (fmk_ctx_set_price_grid); grid_launches: the launches of the last OHLCV call that read the grid (fmk_diag_ohlcv_grid_last)
    int price_grid, grid_launches;
    hipEvent_t kev[FMK_PROFILE_SLOTS][2];
    // stream-ordered caching allocator behind fmk_alloc / fmk_free (fmk_api.hip): freed blocks are kept and handed
    // out again to later requests of (almost) the same size -- no hipMalloc / hipFree / synchronisation per call
    void *pool;
    // result / work caches of the threshold indexers (fmk_volume / fmk_dollar / fmk_threshold .hip), one per context
    void *idx_cache[3];
    // the caches are keyed on device POINTERS (amount, price): when fmk_free gives a block back that holds such a key, the
    // cache is marked stale, so a later allocation that recycles the address for other data cannot hit it
    const void *idx_key[3][2];
    int idx_stale[3];
    // pinned staging buffers / streams of fmk_h2d_columns (fmk_upload.hip), made on first use
    void *upload;
    // auxiliary stream, made on first use (fmk_ctx_aux), and the events that order it against the context's stream.  Reached through
    // FmkSide (below) alone: aux_fork "the context's stream has come this far", aux_done "the side work is queued up to here",
    // aux_landed "the copy to the host that FmkSide::post queued has arrived"; side_open: a fork has not ended yet
    hipStream_t aux;
    hipEvent_t aux_fork, aux_done, aux_landed;
    int side_open;
    // cfg 4 in one pass (fmk_fused.h): what the sizing call leaves for the fill call -- staged level rows, the list of bars the class
    // kernels still have to serve (fmk_barflow.hip: FuState); released by the fill call, the next sizing call, trim and destroy
    void *fused;
};
void fmk_fused_release(fmk_ctx *ctx);
// fmk_comp_bar_footprints_size_dev without dropping staged rows: the cfg 4 sizing calls (fmk_barflow.hip)
int fmk_footprints_size(fmk_ctx *ctx, const double *d_bar_lows, const double *d_bar_highs, int64_t n_bars, double price_tick_size,
                        int64_t *d_level_offsets, int64_t *total_levels, int64_t *max_levels);
int fmk_fused_fill(fmk_ctx *ctx, const double *d_price, const void *d_amount, int amount_is_f64, int64_t n, const int64_t *d_close_idx,
                   int64_t n_idx, const int8_t *d_side, double price_tick_size, const double *d_bar_lows, double imbalance_factor,
                   const int64_t *d_level_offsets, int64_t max_levels, const fmk_footprint_out *d_out, int64_t *d_n_bad_level,
                   int *handled);
// fmk_indexers.hip: the time-bar indexer in stages (sample table, then edges [k0, k1) on a given stream, with the long-bar census)
int fmk_time_bar_coarse_launch(fmk_ctx *ctx, const int64_t *d_ts, int64_t n, const int64_t **coarse, int64_t *m_out, int *clear);
int fmk_time_bar_index_stage(fmk_ctx *ctx, hipStream_t st, const int64_t *d_ts, int64_t n, int64_t e0, int64_t d, int64_t ne,
                             const int64_t *coarse, int64_t m, int64_t k0, int64_t k1, int64_t *d_clock, int64_t *d_idx,
                             int *saw_long, int64_t long_min, int64_t max_blocks /* 0: one workgroup per 256 edges */);

int fmk_set_error(fmk_ctx *ctx, int code, const char *fmt, ...);
// Waits for the context's stream after copies to the host were queued (`queued`: the first failure among them, or hipSuccess): also
// on failure, so that no copy is left in flight.  -> FMK_OK or FMK_E_HIP.
int fmk_wait(fmk_ctx *ctx, hipError_t queued);
// d_src -> dst (host memory of any kind, <= sizeof(fmk_mail::staging) bytes) through the pinned mailbox, then fmk_wait.
int fmk_read_back(fmk_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int fmk_scratch(fmk_ctx *ctx, size_t bytes, void **out);
// per-context result / work caches of the threshold indexers (released by fmk_ctx_trim and fmk_ctx_destroy)
void fmk_volume_trim(fmk_ctx *ctx);
void fmk_dollar_trim(fmk_ctx *ctx);
void fmk_threshold_trim(fmk_ctx *ctx);
void fmk_upload_trim(fmk_ctx *ctx);

// fmk_footprint.hip: footprint fill launches for the level classes wider than `lmin_start` (0: all bars)
int fmk_footprints_fill_classes(fmk_ctx *ctx, const double *d_price, const void *d_amount, int amount_is_f64,
                                const int64_t *d_close_idx, int64_t nb, const int8_t *d_side, double price_tick_size,
                                const double *d_bar_lows, double imb_mult, const int64_t *d_level_offsets, int lmin_start,
                                int64_t max_levels, const fmk_footprint_out *d_out, int64_t *d_n_bad_level,
                                int64_t n_ticks /* 0: unknown */,
                                double *d_median = nullptr /* float32 amounts: the median trade size from the same sweep */,
                                const unsigned long long *only_list = nullptr /* a bar list (fmk_bars.h): only these bars, by the wave-per-bar classes */);
// median of the bars of more than min_cnt ticks (flag d_go), except those of skip_lo < ticks <= skip_hi (served by k_bar_ohlcv_mid)
int fmk_median_launch(fmk_ctx *ctx, const void *d_amount, int amount_is_f64, const int64_t *d_close_idx, int64_t nb,
                      int64_t min_cnt, const int *d_go, double *d_median, int64_t n_ticks, int64_t skip_lo = 0,
                      int64_t skip_hi = 0, int64_t skip_above = INT64_MAX /* bars of more ticks were served elsewhere */);
// the workgroup radix select (k_bar_median_long, 1024 threads) on a given list ([0] = count, then bar numbers), float32 amounts
int fmk_median_long_list_launch(fmk_ctx *ctx, const void *d_amount, const int64_t *d_close_idx, const int64_t *d_list, double *d_median);

// fmk_ohlcv.hip: pieces of comp_bar_ohlcv for cfg 4's first half (fmk_barflow.hip)
int fmk_ohlcv_leftover_launch(fmk_ctx *ctx, const double *p, const void *a, int amount_is_f64, const int64_t *ci, int64_t nb,
                              int64_t n, int64_t min_cnt, const int *go, double *d_open, double *d_high, double *d_low,
                              double *d_close, float *d_volume, double *d_vwap, int64_t *d_trades);
int fmk_median_small_launch(fmk_ctx *ctx, const float *d_amount, const int64_t *d_close_idx, int64_t nb, double *d_median,
                            int64_t n_ticks);
int fmk_median_small_ohlcv_long_launch(fmk_ctx *ctx, const double *p, const float *a, const int64_t *ci, int64_t nb, int64_t n,
                                       double *d_open, double *d_high, double *d_low, double *d_close, float *d_volume,
                                       double *d_vwap, int64_t *d_trades, double *d_median);
// fmk_median.hip: the bars of more than `min_cnt` ticks as a list ([0] = how many, then the bar numbers, any order) in a block of
// the context's pool (*list; the caller gives it back with fmk_free after queueing its kernels) -- the workgroup-per-bar
// kernels take their bars from it, so that a handful of very long bars spread over the whole chip
#define FMK_MAX_BAR_LISTS 8
// K lists in one pass and one allocation: list k = bars of edge[k] < ticks <= edge[k + 1]; free lists[0] (fmk_median.hip)
int fmk_long_bar_lists(fmk_ctx *ctx, const int64_t *d_close_idx, int64_t nb, int64_t n, int k, const int64_t *edge, const int *d_go,
                       int64_t **lists);
int fmk_long_bar_list(fmk_ctx *ctx, const int64_t *d_close_idx, int64_t nb, int64_t n, int64_t min_cnt, const int *d_go,
                      int64_t **list, int64_t max_cnt = INT64_MAX /* bars of min_cnt < ticks <= max_cnt */);

#define FMK_HIP(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fmk_set_error((ctx), e__ == hipErrorOutOfMemory ? FMK_E_NOMEM : FMK_E_HIP, \
                                 "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),     \
                                 __FILE__, __LINE__);                                        \
    } while (0)

#define FMK_TRY(expr)                   \
    do {                                \
        int rc__ = (expr);              \
        if (rc__ != FMK_OK) return rc__; \
    } while (0)

#define FMK_LAUNCH_CHECK(ctx) FMK_HIP(ctx, hipGetLastError())

static inline int64_t fmk_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------------------
// The price grid: a tape whose every price is reproduced BIT FOR BIT from an int32 k carries k as a fifth column, and the small-bar
// OHLCV kernel reads 4 B per tick of it instead of the 8 B of the float64 price (fmk_ohlcv.hip).  Exchange prices lie on a tick grid:
//   form A  p = (double)k * r              the synthetic tape (fmk_synth.hip: (double)k * 0.01)
//   form B  p = RN(k / s), s = 10^d        the nearest double to a decimal string; computed without a division as
//           y = (double)k * r; e = fma(-y, s, (double)k); p = fma(e, r, y)   with r = RN(1 / s): one Newton step on the quotient, exact
//           for every int32 k and d = 0 .. 8 (tools/pricegrid_check.cpp sweeps it against (double)k / s)
// The certificate is the decode itself: fmk_price_grid_build_dev runs it on every tick and compares the bits with the price column,
// so -0.0, NaN, infinities, an off-grid tick or a k beyond int32 refuse the tape with no special case, and a certified tape gives the
// float64 path's results whatever the form.  Plain C++ (host and device) so that the tool can check it without a device.
// ---------------------------------------------------------------------------------------
#define FMK_GRID_NONE 0
#define FMK_GRID_A 1
#define FMK_GRID_B 2
#define FMK_GRID_MAX_D 8
#define FMK_GRID_SAMPLE 128                // prices the scale d is chosen from (one read-back through the mailbox)
struct fmk_price_grid {
    int32_t form;                          // FMK_GRID_NONE: no grid, the reducers read the float64 column
    int32_t d;                             // s = 10^d
    double r;                              // RN(10^-d), the double the decimal literal gives (0.01 for d = 2)
    double s;                              // 10^d
};
#define FMK_GRID_HD __host__ __device__ inline
static inline double fmk_grid_scale(int d)
{
    const double s[FMK_GRID_MAX_D + 1] = {1.0, 10.0, 100.0, 1000.0, 10000.0, 100000.0, 1000000.0, 10000000.0, 100000000.0};
    return s[d];
}
static inline double fmk_grid_recip(int d)
{
    const double r[FMK_GRID_MAX_D + 1] = {1.0, 0.1, 0.01, 0.001, 0.0001, 0.00001, 0.000001, 0.0000001, 0.00000001};
    return r[d];
}
template <int FORM>
FMK_GRID_HD double fmk_grid_decode(int32_t k, double r, double s)
{
    const double x = (double)k;
    const double y = x * r;
    if (FORM == FMK_GRID_A) return y;
    const double e = fma(-y, s, x);        // explicit: the library is built with -ffp-contract=off
    return fma(e, r, y);
}
FMK_GRID_HD uint64_t fmk_grid_bits(double x) { return __builtin_bit_cast(uint64_t, x); }
// k = the grid point next to p, false when it does not fit an int32 (NaN and the infinities fail the comparisons)
FMK_GRID_HD bool fmk_grid_encode(double p, double s, int32_t *k)
{
    const double t = rint(p * s);
    if (!(t >= -2147483648.0 && t <= 2147483647.0)) { *k = 0; return false; }
    *k = (int32_t)t;
    return true;
}
// one tick of the certificate: k (0 when out of range) and whether form A / form B give the price's bits
FMK_GRID_HD int32_t fmk_grid_tick(double p, double r, double s, bool *ok_a, bool *ok_b)
{
    int32_t k;
    const bool in = fmk_grid_encode(p, s, &k);
    const uint64_t want = fmk_grid_bits(p);
    *ok_a = in && fmk_grid_bits(fmk_grid_decode<FMK_GRID_A>(k, r, s)) == want;
    *ok_b = in && fmk_grid_bits(fmk_grid_decode<FMK_GRID_B>(k, r, s)) == want;
    return k;
}
// the scale: the smallest d in 0 .. 8 at which every price of the sample certifies under one of the forms; -1: none (or no sample)
static inline int fmk_grid_choose_d(const double *sample, int64_t m)
{
    if (m <= 0) return -1;
    for (int d = 0; d <= FMK_GRID_MAX_D; ++d) {
        const double r = fmk_grid_recip(d), s = fmk_grid_scale(d);
        int64_t mis_a = 0, mis_b = 0;
        for (int64_t i = 0; i < m; ++i) {
            bool a, b;
            (void)fmk_grid_tick(sample[i], r, s, &a, &b);
            mis_a += !a;
            mis_b += !b;
        }
        if (mis_a == 0 || mis_b == 0) return d;
    }
    return -1;
}
// the form from the whole tape's mismatch counts: A where it certifies (two instructions per tick fewer), else B, else no grid
static inline int fmk_grid_choose_form(uint64_t mis_a, uint64_t mis_b)
{
    return mis_a == 0 ? FMK_GRID_A : mis_b == 0 ? FMK_GRID_B : FMK_GRID_NONE;
}

// the workgroups of a 256-lane grid-stride kernel over n elements: at most 16 per CU, at least one
static inline unsigned fmk_grid_blocks(const fmk_ctx *ctx, int64_t n)
{
    int64_t blocks = fmk_ceil_div(n, 256);
    if (blocks > (int64_t)ctx->n_cu * 16) blocks = (int64_t)ctx->n_cu * 16;
    return (unsigned)(blocks > 0 ? blocks : 1);
}
// NaN in d_out[0 .. min(window - 1, n)): the outputs before the first full window (fmk_rolling.hip)
int fmk_nan_head(fmk_ctx *ctx, double *d_out, int64_t n, int64_t window);

// What the series entries (fmk_rolling.hip, fmk_order.hip) refuse before any pointer is looked at and before a device is needed;
// the host-pointer flavours (fmk_host.hip) ask the argument rules before any upload.  what: the name the _dev entry puts in front.
static inline int fmk_series_check(fmk_ctx *ctx, const char *what, int64_t n)
{
    if (n < 0 || n >= ((int64_t)1 << 31)) return fmk_set_error(ctx, FMK_E_ARG, "%s: the series must hold fewer than 2^31 elements.", what);
    return FMK_OK;
}
static inline int fmk_rule_least(fmk_ctx *ctx, int64_t arg, int64_t least, const char *message)
{
    return arg < least ? fmk_set_error(ctx, FMK_E_ARG, "%s", message) : FMK_OK;
}
static inline int fmk_rule_window(fmk_ctx *ctx, const char *what, int64_t window)
{
    if (what && window < 1) return fmk_set_error(ctx, FMK_E_ARG, "%s: window must be at least 1.", what);
    return fmk_rule_least(ctx, window, 1, "window must be at least 1.");
}
static inline int fmk_rule_zscore(fmk_ctx *ctx, int64_t window, int64_t ddof)
{
    return ddof >= window ? fmk_set_error(ctx, FMK_E_ARG, "comp_zscore: window - ddof must be positive.") : FMK_OK;
}
static inline int fmk_rule_roc(fmk_ctx *ctx, int64_t period) { return fmk_rule_least(ctx, period, 0, "roc: period must not be negative."); }
static inline int fmk_rule_pct_change(fmk_ctx *ctx, int64_t periods)
{
    return fmk_rule_least(ctx, periods, 0, "pct_change: periods must not be negative.");
}
static inline int fmk_rule_stoch_k(fmk_ctx *ctx, int64_t length) { return fmk_rule_least(ctx, length, 1, "stoch_k: length must be at least 1."); }
// the recursive indicators (fmk_recur.hip); ewma's message is the reference's
static inline int fmk_rule_ewma(fmk_ctx *ctx, double span)
{
    return span >= 1.0 ? FMK_OK
                       : fmk_set_error(ctx, FMK_E_ARG, "span size is less than or equal to 1. Please provide a span size greater than 1.");
}
static inline int fmk_rule_rsi_wilder(fmk_ctx *ctx, int64_t window) { return fmk_rule_least(ctx, window, 1, "rsi_wilder: window must be at least 1."); }
static inline int fmk_rule_atr(fmk_ctx *ctx, int64_t window) { return fmk_rule_least(ctx, window, 0, "atr: window must not be negative."); }
static inline int fmk_rule_adx(fmk_ctx *ctx, int64_t length) { return fmk_rule_least(ctx, length, 1, "adx_core: length must be at least 1."); }
// the running-sum indicators (fmk_runsum.hip)
static inline int fmk_rule_bollinger(fmk_ctx *ctx, int64_t window)
{
    return fmk_rule_least(ctx, window, 1, "bollinger_percent_b: window must be at least 1.");
}
static inline int fmk_rule_vwap_distance(fmk_ctx *ctx, int64_t n_periods)
{
    return fmk_rule_least(ctx, n_periods, 1, "vwap_distance: n_periods must be at least 1.");
}
static inline int fmk_rule_flow_acceleration(fmk_ctx *ctx, int64_t recent_periods)
{
    return fmk_rule_least(ctx, recent_periods, 0, "comp_flow_acceleration: recent_periods must not be negative.");
}
static inline int fmk_rule_vpin(fmk_ctx *ctx, int64_t window) { return fmk_rule_least(ctx, window, 0, "vpin: window must not be negative."); }
// the bar clock (fmk_clock.hip): bar_duration_ewma asks fmk_rule_ewma; the reference's BarRate divides by zero at a zero window
static inline int fmk_rule_bar_rate(fmk_ctx *ctx, int64_t window_ns)
{
    return fmk_rule_least(ctx, window_ns, 1, "bar_rate: the window must be at least one nanosecond.");
}
// the window statistics (fmk_shape.hip): hurst's lag 8 needs one difference (asked after fmk_rule_window)
static inline int fmk_rule_hurst(fmk_ctx *ctx, int64_t window) { return fmk_rule_least(ctx, window, 9, "hurst_exponent: window must be at least 9."); }
// trend scanning (fmk_trend.hip): a line through fewer than three points has no t-value
static inline int fmk_rule_trend(fmk_ctx *ctx, int64_t min_len, int64_t max_len, int64_t step)
{
    FMK_TRY(fmk_rule_least(ctx, min_len, 3, "trend_scanning: min_len must be at least 3."));
    if (max_len < min_len) return fmk_set_error(ctx, FMK_E_ARG, "trend_scanning: max_len must not be less than min_len.");
    return fmk_rule_least(ctx, step, 1, "trend_scanning: step must be at least 1.");
}
// the ADF / SADF statistic (fmk_sadf.hip): k = lags + 2 (+ 1 with a time trend) regressors need k + 1 rows for one degree of freedom
#define FMK_ADF_MAX_LAGS 4
static inline int fmk_rule_sadf(fmk_ctx *ctx, int64_t min_len, int64_t max_len, int64_t step, int64_t lags, int trend, const void *y,
                                const void *stat, const void *start)
{
    if (lags < 0 || lags > FMK_ADF_MAX_LAGS) return fmk_set_error(ctx, FMK_E_ARG, "sadf: lags must be between 0 and 4.");
    if (trend != 0 && trend != 1) return fmk_set_error(ctx, FMK_E_ARG, "sadf: trend must be \"c\" (0) or \"ct\" (1).");
    const int64_t k = lags + 2 + trend;
    if (min_len < k + 1)
        return fmk_set_error(ctx, FMK_E_ARG, "sadf: min_len must be at least %lld (one more than the %lld regressors).", (long long)(k + 1),
                             (long long)k);
    if (max_len < min_len) return fmk_set_error(ctx, FMK_E_ARG, "sadf: max_len must not be less than min_len.");
    FMK_TRY(fmk_rule_least(ctx, step, 1, "sadf: step must be at least 1."));
    if (y && (stat == y || start == y)) return fmk_set_error(ctx, FMK_E_ARG, "sadf: an output must not be the input.");
    return FMK_OK;
}
// the approximate entropy (fmk_entropy.hip): the order-(m + 1) embedding needs one vector; one tile's span and the table of
// logarithms have to fit in LDS; the kernels are instantiated per m
#define FMK_APEN_MAX_M 4
#define FMK_APEN_MAX_WINDOW 1024
static inline int fmk_rule_apen(fmk_ctx *ctx, int64_t window, int64_t m, double tolerance)
{
    FMK_TRY(fmk_rule_least(ctx, m, 1, "approximate_entropy: m must be at least 1."));
    if (m > FMK_APEN_MAX_M) return fmk_set_error(ctx, FMK_E_ARG, "approximate_entropy: m must be at most 4.");
    if (window < m + 1) return fmk_set_error(ctx, FMK_E_ARG, "approximate_entropy: window must be at least m + 1.");
    if (window > FMK_APEN_MAX_WINDOW) return fmk_set_error(ctx, FMK_E_ARG, "approximate_entropy: window must be at most 1024.");
    if (!(tolerance >= 0.0 && tolerance < INFINITY))
        return fmk_set_error(ctx, FMK_E_ARG, "approximate_entropy: tolerance must be finite and not negative.");
    return FMK_OK;
}

// the causal FIR filter (fmk_fir.hip): the weights are a host array in both flavours, so both can look at them; the geometry is
// here for fmk_fir_geometry and the kernel alike
#define FMK_FIR_MAX_WIDTH 8192
#define FMK_FIR_TILE 512                   // outputs per workgroup
#define FMK_FIR_TAPS 512                   // taps per staging pass
static inline int fmk_rule_fir(fmk_ctx *ctx, const double *w, int64_t width, const double *x, const double *out)
{
    FMK_TRY(fmk_rule_least(ctx, width, 1, "fir: at least one weight is needed."));
    if (width > FMK_FIR_MAX_WIDTH) return fmk_set_error(ctx, FMK_E_ARG, "fir: at most 8192 weights.");
    for (int64_t k = 0; k < width; ++k)
        if (!(w[k] - w[k] == 0.0)) return fmk_set_error(ctx, FMK_E_ARG, "fir: the weights must be finite.");
    if (out == x) return fmk_set_error(ctx, FMK_E_ARG, "fir: the output must not be the input.");
    return FMK_OK;
}

// the encoded-series entropies (fmk_lz.hip; the limits are fmk_lz_rule.h's): the edges are a host array in both flavours of encode
static inline int fmk_rule_encode(fmk_ctx *ctx, const double *edges, int64_t n_edges)
{
    if (!edges) n_edges = 0;
    FMK_TRY(fmk_rule_least(ctx, n_edges, 1, "encode: at least one edge is needed."));
    if (n_edges > 254) return fmk_set_error(ctx, FMK_E_ARG, "encode: at most 254 edges.");
    for (int64_t k = 0; k < n_edges; ++k)
        if (!(edges[k] - edges[k] == 0.0)) return fmk_set_error(ctx, FMK_E_ARG, "encode: the edges must be finite.");
    for (int64_t k = 1; k < n_edges; ++k)
        if (!(edges[k - 1] < edges[k])) return fmk_set_error(ctx, FMK_E_ARG, "encode: the edges must be strictly increasing.");
    return FMK_OK;
}
static inline int fmk_rule_plugin_entropy(fmk_ctx *ctx, int64_t window, int64_t word, int64_t alphabet)
{
    if (alphabet < 2 || alphabet > 255) return fmk_set_error(ctx, FMK_E_ARG, "plugin_entropy: alphabet must be between 2 and 255.");
    FMK_TRY(fmk_rule_least(ctx, word, 1, "plugin_entropy: word must be at least 1."));
    int64_t bins = 1;
    for (int64_t j = 0; j < word && bins <= 4096; ++j) bins *= alphabet;
    if (bins > 4096) return fmk_set_error(ctx, FMK_E_ARG, "plugin_entropy: alphabet^word must be at most 4096.");
    if (window < word) return fmk_set_error(ctx, FMK_E_ARG, "plugin_entropy: window must be at least word.");
    if (window > 4096) return fmk_set_error(ctx, FMK_E_ARG, "plugin_entropy: window must be at most 4096.");
    return FMK_OK;
}
static inline int fmk_rule_match_lengths(fmk_ctx *ctx, int64_t lookback)
{
    if (lookback < 1 || lookback > 1024) return fmk_set_error(ctx, FMK_E_ARG, "match_lengths: lookback must be between 1 and 1024.");
    return FMK_OK;
}
static inline int fmk_rule_kontoyiannis(fmk_ctx *ctx, int64_t window, int64_t lookback)
{
    if (lookback < 1 || lookback > 1024)
        return fmk_set_error(ctx, FMK_E_ARG, "kontoyiannis_entropy: lookback must be between 1 and 1024.");
    if (window < 2 * lookback) return fmk_set_error(ctx, FMK_E_ARG, "kontoyiannis_entropy: window must be at least 2 * lookback.");
    if (window > 4096) return fmk_set_error(ctx, FMK_E_ARG, "kontoyiannis_entropy: window must be at most 4096.");
    return FMK_OK;
}

// bet sizing (fmk_bet.hip): what both flavours refuse from their scalars alone (the budget call passes step 0); the limits and the
// step rule are fmk_bet_rule.h's
#include "fmk_bet_rule.h"
static inline int fmk_rule_bet(fmk_ctx *ctx, const char *what, int64_t n_events, int64_t n, double step)
{
    if (n_events < 1 || n_events > FMK_BET_MAX_EVENTS)
        return fmk_set_error(ctx, FMK_E_ARG, "%s: n_events must be between 1 and 2^31 - 1.", what);
    if (n < 1 || n > FMK_BET_MAX_AXIS) return fmk_set_error(ctx, FMK_E_ARG, "%s: n must be between 1 and 2^32.", what);
    if (!fmk_bet_step_ok(step)) return fmk_set_error(ctx, FMK_E_ARG, "%s: step must be 0 (no discretisation) or in (0, 1].", what);
    return FMK_OK;
}

// the per-bar microstructure features (fmk_micro.hip): what both flavours refuse from their arguments alone -- the host flavour with
// its host pointers, before anything is uploaded (it also looks at the close indices themselves, which it can read)
static inline bool fmk_ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}
static inline int fmk_rule_micro(fmk_ctx *ctx, const double *price, const void *amount, int amount_is_f64, int64_t n,
                                 const int64_t *close_idx, int64_t n_idx, const int8_t *side, const fmk_microstructure_out *out)
{
    if (n_idx < 1 || n < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    if (n_idx == 1) return FMK_OK;
    if (!out || !price || !amount || !close_idx || !side)
        return fmk_set_error(ctx, FMK_E_ARG, "comp_bar_microstructure: a null column");
    double *const cols[8] = {out->kyle_lambda, out->kyle_t, out->amihud_lambda, out->amihud_t,
                             out->hasbrouck_lambda, out->hasbrouck_t, out->serial_cov, out->roll_spread};
    const size_t ob = sizeof(double) * (size_t)(n_idx - 1);
    for (int k = 0; k < 8; ++k) {
        if (!cols[k]) return fmk_set_error(ctx, FMK_E_ARG, "comp_bar_microstructure: a null output column");
        if (fmk_ranges_overlap(cols[k], ob, price, sizeof(double) * (size_t)n) ||
            fmk_ranges_overlap(cols[k], ob, amount, (amount_is_f64 ? 8 : 4) * (size_t)n) ||
            fmk_ranges_overlap(cols[k], ob, side, (size_t)n) ||
            fmk_ranges_overlap(cols[k], ob, close_idx, sizeof(int64_t) * (size_t)n_idx))
            return fmk_set_error(ctx, FMK_E_ARG, "comp_bar_microstructure: an output must not alias an input.");
    }
    return FMK_OK;
}

// One excursion of a call onto the context's auxiliary stream (fmk_api.hip), the only way there.  Rules:
//  - one fork per context at a time: fork() while another FmkSide of the context is open is an error;
//  - the context scratch belongs to the context's stream: fmk_scratch inside run() is an error;
//  - success paths wait on the device only (events); a host wait happens in landed() and nowhere else;
//  - an FmkSide that goes out of scope forked but not joined (any early return), or with a post() nobody waited for, drains the
//    auxiliary stream first: no work of a call outlives its return on that stream;
//  - fork(true) parks every fmk_free of the context until the FmkSide ends, so that no block freed on one stream is handed to the
//    other (the allocator's free list follows ONE stream's order); fork(false) is for excursions without fmk_free in between.
struct FmkSide {
    explicit FmkSide(fmk_ctx *c) : ctx(c) {}
    FmkSide(const FmkSide &) = delete;
    FmkSide &operator=(const FmkSide &) = delete;
    ~FmkSide();
    int fork(bool defer_pool);             // the auxiliary stream waits for what the context's stream holds now
    hipStream_t stream() const { return ctx->aux; }      // for callees that take a stream argument (after fork)
    template <class F> int run(F &&f)      // f() with the auxiliary stream as ctx->stream: callees that launch on the context's stream
    {
        if (!forked) return fmk_set_error(ctx, FMK_E_HIP, "FmkSide::run without a fork");
        struct Restore { fmk_ctx *c; hipStream_t keep; ~Restore() { c->stream = keep; } } restore{ctx, ctx->stream};
        ctx->stream = ctx->aux;
        return f();
    }
    int mark();                            // "side done": what the auxiliary stream holds now
    int join();                            // the context's stream waits for the mark
    int post(void *h_dst, const void *d_src, size_t bytes);   // behind the mark: a copy to pinned host memory, then "landed"
    int landed();                          // the host waits for that copy (and for nothing behind it)
private:
    fmk_ctx *ctx;
    bool forked = false, parked = false, joined = false, posted = false;
};

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int fmk_lane() { return threadIdx.x & 63; }

// Make a wave-uniform 64-bit value provably uniform (SGPR pair) for the compiler.
__device__ __forceinline__ int64_t fmk_uniform(int64_t v)
{
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int fmk_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// value of lane `src` (wave-uniform index) broadcast to the wave
__device__ __forceinline__ int64_t fmk_readlane(int64_t v, int src)
{
    uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <typename T>
__device__ __forceinline__ T fmk_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double fmk_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double fmk_wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int64_t fmk_wave_max(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { int64_t w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ int64_t fmk_wave_min(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { int64_t w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}
// inclusive scan across the 64 lanes (Kogge-Stone, 6 steps)
template <typename T>
__device__ __forceinline__ T fmk_wave_iscan(T v)
{
    const int lane = fmk_lane();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        T w = __shfl_up(v, o, 64);
        if (lane >= o) v += w;
    }
    return v;
}

// amount column element j as float64 (float32 -> float64 is exact)
template <bool F64>
__device__ __forceinline__ double fmk_amt(const void *p, int64_t j)
{
    if constexpr (F64) return ((const double *)p)[j];
    else return (double)((const float *)p)[j];
}

// Python negative-index wrap of the reference (prices[-1] when close_idx[0] == -1)
__device__ __forceinline__ int64_t fmk_wrap(int64_t i, int64_t n) { return i < 0 ? i + n : i; }

// splitmix64-style counter hash shared with oracle/fmk_oracle.c (orc_mix64)
__host__ __device__ __forceinline__ uint64_t fmk_mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
#endif  // __HIPCC__
