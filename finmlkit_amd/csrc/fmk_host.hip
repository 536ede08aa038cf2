// fmk_host.hip -- host-pointer flavours of the C ABI (the NumPy drop-in boundary).
// Each function uploads its inputs, runs the same device entry point the resident pipeline
// uses, downloads the outputs and synchronises.  No arithmetic happens here.
#include <vector>

#include "fmk_common.h"

namespace {

// RAII bag of device allocations tied to one call
struct DevBag {
    fmk_ctx *ctx;
    std::vector<void *> ptrs;
    explicit DevBag(fmk_ctx *c) : ctx(c) {}
    ~DevBag()
    {
        (void)hipStreamSynchronize(ctx->stream);
        for (void *p : ptrs) (void)fmk_free(ctx, p);      // back to the context's caching allocator
    }
    int alloc(size_t bytes, void **out)
    {
        int rc = fmk_alloc(ctx, bytes, out);
        if (rc == FMK_OK) ptrs.push_back(*out);
        return rc;
    }
    template <typename T>
    int up(const T *host, int64_t count, T **out)
    {
        void *p;
        FMK_TRY(alloc(sizeof(T) * (size_t)(count > 0 ? count : 1), &p));
        if (count > 0) FMK_TRY(fmk_h2d(ctx, p, host, sizeof(T) * (size_t)count));
        *out = (T *)p;
        return FMK_OK;
    }
    template <typename T>
    int out(int64_t count, T **o)
    {
        void *p;
        FMK_TRY(alloc(sizeof(T) * (size_t)(count > 0 ? count : 1), &p));
        *o = (T *)p;
        return FMK_OK;
    }
    int up_amount(const void *host, int is_f64, int64_t count, void **o)
    {
        size_t es = is_f64 ? 8 : 4;
        FMK_TRY(alloc(es * (size_t)(count > 0 ? count : 1), o));
        if (count > 0) FMK_TRY(fmk_h2d(ctx, *o, host, es * (size_t)count));
        return FMK_OK;
    }
};

template <typename T>
int down(fmk_ctx *ctx, T *host, const T *dev, int64_t count)
{
    if (!host || count <= 0) return FMK_OK;
    return fmk_d2h(ctx, host, dev, sizeof(T) * (size_t)count);
}

// the rolling-window moments (fmk_rolling.hip) and order statistics (fmk_order.hip): one series up, dev(d_x, d_out), one series
// down.  rule: the entry's argument rule (fmk_common.h), asked before anything is uploaded
template <typename Dev>
int series_host(fmk_ctx *ctx, int rule, const double *x, int64_t n, double *out, Dev dev)
{
    FMK_TRY(rule);
    DevBag bag(ctx);
    double *d_x, *d_o;
    FMK_TRY(bag.up(x, n, &d_x));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(dev(d_x, d_o));
    return down(ctx, out, (const double *)d_o, n);
}

// three series up in the order given (high, low, close; stoch_k's close, low, high), dev(d_1, d_2, d_3, d_out), one series down
template <typename Dev>
int hlc_host(fmk_ctx *ctx, int rule, const double *high, const double *low, const double *close, int64_t n, double *out, Dev dev)
{
    FMK_TRY(rule);
    DevBag bag(ctx);
    double *d_h, *d_l, *d_c, *d_o;
    FMK_TRY(bag.up(high, n, &d_h));
    FMK_TRY(bag.up(low, n, &d_l));
    FMK_TRY(bag.up(close, n, &d_c));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(dev(d_h, d_l, d_c, d_o));
    return down(ctx, out, (const double *)d_o, n);
}

// two series up, dev(d_a, d_b, d_out), one series of T down
template <typename T, typename Dev>
int pair_host(fmk_ctx *ctx, int rule, const double *a, const double *b, int64_t n, T *out, Dev dev)
{
    FMK_TRY(rule);
    DevBag bag(ctx);
    double *d_a, *d_b;
    T *d_o;
    FMK_TRY(bag.up(a, n, &d_a));
    FMK_TRY(bag.up(b, n, &d_b));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(dev(d_a, d_b, d_o));
    return down(ctx, out, (const T *)d_o, n);
}

// the encoded-series entropies (fmk_lz.hip): one series of In up, dev(d_in, d_out), one series of Out down; the caller has asked the
// rules, and an empty series is answered before the context is looked at
template <typename In, typename Out, typename Dev>
int lz_host(fmk_ctx *ctx, const In *in, int64_t n, Out *out, Dev dev)
{
    if (n == 0) return FMK_OK;
    DevBag bag(ctx);
    In *d_in;
    Out *d_o;
    FMK_TRY(bag.up(in, n, &d_in));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(dev((const In *)d_in, d_o));
    return down(ctx, out, (const Out *)d_o, n);
}

}  // namespace

extern "C" {

int fmk_time_bar_indexer(fmk_ctx *ctx, const int64_t *ts, int64_t n, double interval_seconds, int64_t *clock,
                         int64_t *close_idx, int64_t capacity, int64_t *n_edges)
{
    if (n <= 0) return fmk_set_error(ctx, FMK_E_ARG, "time_bar_indexer: empty timestamps");
    int64_t ne, e0, d;
    int rc = fmk_time_bar_clock(ts[0], ts[n - 1], interval_seconds, &ne, &e0, &d);
    if (rc) return fmk_set_error(ctx, rc, "%s", fmk_last_error(nullptr));
    *n_edges = ne;
    if (!clock || !close_idx) return FMK_OK;
    if (capacity < ne) return fmk_set_error(ctx, FMK_E_CAPACITY, "time_bar_indexer: capacity");
    DevBag bag(ctx);
    int64_t *d_ts, *d_clock, *d_idx;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.out(ne, &d_clock));
    FMK_TRY(bag.out(ne, &d_idx));
    FMK_TRY(fmk_time_bar_indexer_dev(ctx, d_ts, n, e0, d, ne, d_clock, d_idx));
    FMK_TRY(down(ctx, clock, d_clock, ne));
    FMK_TRY(down(ctx, close_idx, d_idx, ne));
    return FMK_OK;
}

int fmk_comp_bar_ohlcv(fmk_ctx *ctx, const double *price, const void *amount, int amount_is_f64, int64_t n,
                       const int64_t *close_idx, int64_t n_idx, double *open_, double *high, double *low,
                       double *close_, float *volume, double *vwap, int64_t *trades, double *median)
{
    if (n_idx < 2)
        return fmk_set_error(ctx, FMK_E_ARG, "Bar close indices must contain at least two elements.");
    const int64_t nb = n_idx - 1;
    DevBag bag(ctx);
    double *d_p;
    void *d_a;
    int64_t *d_ci;
    FMK_TRY(bag.up(price, n, &d_p));
    FMK_TRY(bag.up_amount(amount, amount_is_f64, n, &d_a));
    FMK_TRY(bag.up(close_idx, n_idx, &d_ci));
    double *d_o, *d_h, *d_l, *d_c, *d_vw, *d_med = nullptr;
    float *d_v;
    int64_t *d_t;
    FMK_TRY(bag.out(nb, &d_o));
    FMK_TRY(bag.out(nb, &d_h));
    FMK_TRY(bag.out(nb, &d_l));
    FMK_TRY(bag.out(nb, &d_c));
    FMK_TRY(bag.out(nb, &d_v));
    FMK_TRY(bag.out(nb, &d_vw));
    FMK_TRY(bag.out(nb, &d_t));
    if (median) FMK_TRY(bag.out(nb, &d_med));
    FMK_TRY(fmk_comp_bar_ohlcv_dev(ctx, d_p, d_a, amount_is_f64, n, d_ci, n_idx, d_o, d_h, d_l, d_c, d_v, d_vw,
                                   d_t, d_med));
    FMK_TRY(down(ctx, open_, d_o, nb));
    FMK_TRY(down(ctx, high, d_h, nb));
    FMK_TRY(down(ctx, low, d_l, nb));
    FMK_TRY(down(ctx, close_, d_c, nb));
    FMK_TRY(down(ctx, volume, d_v, nb));
    FMK_TRY(down(ctx, vwap, d_vw, nb));
    FMK_TRY(down(ctx, trades, d_t, nb));
    FMK_TRY(down(ctx, median, d_med, nb));
    return FMK_OK;
}

}  // extern "C"

extern "C" {

int fmk_comp_bar_directional(fmk_ctx *ctx, const double *price, const void *amount, int amount_is_f64, int64_t n,
                             const int64_t *close_idx, int64_t n_idx, const int8_t *side,
                             const fmk_directional_out *out)
{
    // base.py:409-546 has no length check on bar_close_indices (only comp_bar_ohlcv has, base.py:334-335): one element
    // means zero bars and empty outputs (the reference's tests use that for comp_bar_footprints)
    if (n_idx == 1) return FMK_OK;
    if (n_idx < 1) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    const int64_t nb = n_idx - 1;
    DevBag bag(ctx);
    double *d_p;
    void *d_a;
    int64_t *d_ci, *d_nz;
    int8_t *d_s;
    FMK_TRY(bag.up(price, n, &d_p));
    FMK_TRY(bag.up_amount(amount, amount_is_f64, n, &d_a));
    FMK_TRY(bag.up(close_idx, n_idx, &d_ci));
    FMK_TRY(bag.up(side, n, &d_s));
    FMK_TRY(bag.out(1, &d_nz));
    FMK_TRY(fmk_memset(ctx, d_nz, 0, 8));
    fmk_directional_out d;
    int64_t **di[] = {&d.ticks_buy, &d.ticks_sell, &d.cum_ticks_min, &d.cum_ticks_max};
    float **df[] = {&d.volume_buy, &d.volume_sell, &d.dollars_buy, &d.dollars_sell, &d.mean_spread, &d.max_spread,
                    &d.cum_volumes_min, &d.cum_volumes_max, &d.cum_dollars_min, &d.cum_dollars_max};
    for (auto p : di) FMK_TRY(bag.out(nb, p));
    for (auto p : df) FMK_TRY(bag.out(nb, p));
    FMK_TRY(fmk_comp_bar_directional_dev(ctx, d_p, d_a, amount_is_f64, n, d_ci, n_idx, d_s, &d, d_nz));
    FMK_TRY(down(ctx, out->ticks_buy, d.ticks_buy, nb));
    FMK_TRY(down(ctx, out->ticks_sell, d.ticks_sell, nb));
    FMK_TRY(down(ctx, out->volume_buy, d.volume_buy, nb));
    FMK_TRY(down(ctx, out->volume_sell, d.volume_sell, nb));
    FMK_TRY(down(ctx, out->dollars_buy, d.dollars_buy, nb));
    FMK_TRY(down(ctx, out->dollars_sell, d.dollars_sell, nb));
    FMK_TRY(down(ctx, out->mean_spread, d.mean_spread, nb));
    FMK_TRY(down(ctx, out->max_spread, d.max_spread, nb));
    FMK_TRY(down(ctx, out->cum_ticks_min, d.cum_ticks_min, nb));
    FMK_TRY(down(ctx, out->cum_ticks_max, d.cum_ticks_max, nb));
    FMK_TRY(down(ctx, out->cum_volumes_min, d.cum_volumes_min, nb));
    FMK_TRY(down(ctx, out->cum_volumes_max, d.cum_volumes_max, nb));
    FMK_TRY(down(ctx, out->cum_dollars_min, d.cum_dollars_min, nb));
    FMK_TRY(down(ctx, out->cum_dollars_max, d.cum_dollars_max, nb));
    int64_t nz = 0;
    FMK_TRY(fmk_d2h(ctx, &nz, d_nz, 8));
    if (nz > 0)   // base.py:536: current_cum_spread / (buy + sell) with buy + sell == 0
        return fmk_set_error(ctx, FMK_E_ZERODIV, "division by zero: %lld bar(s) without a signed tick", (long long)nz);
    return FMK_OK;
}

int fmk_comp_bar_footprints(fmk_ctx *ctx, const double *price, const void *amount, int amount_is_f64, int64_t n,
                            const int64_t *close_idx, int64_t n_idx, const int8_t *side, double price_tick_size,
                            const double *bar_lows, const double *bar_highs, double imbalance_factor,
                            int64_t *level_offsets, const fmk_footprint_out *out)
{
    // base.py:615-752 has no length check: one element = zero bars = empty outputs
    // (reference test tests/bars/test_comp_bar_footprints.py::test_comp_bar_footprints_empty_bar)
    if (n_idx == 1) { if (level_offsets) level_offsets[0] = 0; return FMK_OK; }
    if (n_idx < 1) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    const int64_t nb = n_idx - 1;
    DevBag bag(ctx);
    double *d_lo, *d_hi;
    int64_t *d_off;
    FMK_TRY(bag.up(bar_lows, nb, &d_lo));
    FMK_TRY(bag.up(bar_highs, nb, &d_hi));
    FMK_TRY(bag.out(nb + 1, &d_off));
    int64_t total = 0, maxl = 0;
    FMK_TRY(fmk_comp_bar_footprints_size_dev(ctx, d_lo, d_hi, nb, price_tick_size, d_off, &total, &maxl));
    FMK_TRY(down(ctx, level_offsets, d_off, nb + 1));
    if (!out) return FMK_OK;
    double *d_p;
    void *d_a;
    int64_t *d_ci, *d_bad;
    int8_t *d_s;
    FMK_TRY(bag.up(price, n, &d_p));
    FMK_TRY(bag.up_amount(amount, amount_is_f64, n, &d_a));
    FMK_TRY(bag.up(close_idx, n_idx, &d_ci));
    FMK_TRY(bag.up(side, n, &d_s));
    FMK_TRY(bag.out(1, &d_bad));
    FMK_TRY(fmk_memset(ctx, d_bad, 0, 8));
    fmk_footprint_out d;
    FMK_TRY(bag.out(total, &d.price_levels));
    FMK_TRY(bag.out(total, &d.buy_volumes));
    FMK_TRY(bag.out(total, &d.sell_volumes));
    FMK_TRY(bag.out(total, &d.buy_ticks));
    FMK_TRY(bag.out(total, &d.sell_ticks));
    FMK_TRY(bag.out(total, &d.buy_imbalances));
    FMK_TRY(bag.out(total, &d.sell_imbalances));
    FMK_TRY(bag.out(nb, &d.buy_imbalances_sum));
    FMK_TRY(bag.out(nb, &d.sell_imbalances_sum));
    FMK_TRY(bag.out(nb, &d.cot_price_levels));
    FMK_TRY(bag.out(nb, &d.imb_max_run_signed));
    FMK_TRY(bag.out(nb, &d.vp_skew));
    FMK_TRY(bag.out(nb, &d.vp_gini));
    FMK_TRY(fmk_memset(ctx, d.buy_imbalances_sum, 0, 2 * (size_t)nb));
    FMK_TRY(fmk_memset(ctx, d.sell_imbalances_sum, 0, 2 * (size_t)nb));
    FMK_TRY(fmk_memset(ctx, d.cot_price_levels, 0, 4 * (size_t)nb));
    FMK_TRY(fmk_memset(ctx, d.imb_max_run_signed, 0, 2 * (size_t)nb));
    FMK_TRY(fmk_memset(ctx, d.vp_skew, 0, 8 * (size_t)nb));
    FMK_TRY(fmk_memset(ctx, d.vp_gini, 0, 8 * (size_t)nb));
    FMK_TRY(fmk_comp_bar_footprints_fill_dev(ctx, d_p, d_a, amount_is_f64, n, d_ci, n_idx, d_s, price_tick_size, d_lo,
                                             imbalance_factor, d_off, maxl, &d, d_bad));
    FMK_TRY(down(ctx, out->price_levels, d.price_levels, total));
    FMK_TRY(down(ctx, out->buy_volumes, d.buy_volumes, total));
    FMK_TRY(down(ctx, out->sell_volumes, d.sell_volumes, total));
    FMK_TRY(down(ctx, out->buy_ticks, d.buy_ticks, total));
    FMK_TRY(down(ctx, out->sell_ticks, d.sell_ticks, total));
    FMK_TRY(down(ctx, out->buy_imbalances, d.buy_imbalances, total));
    FMK_TRY(down(ctx, out->sell_imbalances, d.sell_imbalances, total));
    FMK_TRY(down(ctx, out->buy_imbalances_sum, d.buy_imbalances_sum, nb));
    FMK_TRY(down(ctx, out->sell_imbalances_sum, d.sell_imbalances_sum, nb));
    FMK_TRY(down(ctx, out->cot_price_levels, d.cot_price_levels, nb));
    FMK_TRY(down(ctx, out->imb_max_run_signed, d.imb_max_run_signed, nb));
    FMK_TRY(down(ctx, out->vp_skew, d.vp_skew, nb));
    FMK_TRY(down(ctx, out->vp_gini, d.vp_gini, nb));
    int64_t bad = 0;
    FMK_TRY(fmk_d2h(ctx, &bad, d_bad, 8));
    if (bad > 0)   // base.py:719
        return fmk_set_error(ctx, FMK_E_LEVEL, "Something went wrong! Invalid price level index!");
    return FMK_OK;
}

int fmk_comp_bar_trade_size(fmk_ctx *ctx, const void *amount, int amount_is_f64, int64_t n, const double *theta,
                            const int64_t *close_idx, int64_t n_idx, double theta_mult, float *mean_size_rel,
                            float *size_95_rel, float *pct_block, float *size_gini)
{
    if (n_idx == 1) return FMK_OK;   // base.py:549-612 checks theta's length only: zero bars, empty outputs
    if (n_idx < 1) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    const int64_t nb = n_idx - 1;
    DevBag bag(ctx);
    void *d_a;
    double *d_th;
    int64_t *d_ci;
    float *d_o[4];
    FMK_TRY(bag.up_amount(amount, amount_is_f64, n, &d_a));
    FMK_TRY(bag.up(theta, nb, &d_th));
    FMK_TRY(bag.up(close_idx, n_idx, &d_ci));
    for (int k = 0; k < 4; ++k) FMK_TRY(bag.out(nb, &d_o[k]));
    FMK_TRY(fmk_comp_bar_trade_size_dev(ctx, d_a, amount_is_f64, n, d_th, d_ci, n_idx, theta_mult, d_o[0], d_o[1],
                                        d_o[2], d_o[3]));
    FMK_TRY(down(ctx, mean_size_rel, d_o[0], nb));
    FMK_TRY(down(ctx, size_95_rel, d_o[1], nb));
    FMK_TRY(down(ctx, pct_block, d_o[2], nb));
    return down(ctx, size_gini, d_o[3], nb);
}

int fmk_comp_bar_microstructure(fmk_ctx *ctx, const double *price, const void *amount, int amount_is_f64, int64_t n,
                                const int64_t *close_idx, int64_t n_idx, const int8_t *side, const fmk_microstructure_out *out)
{
    FMK_TRY(fmk_rule_micro(ctx, price, amount, amount_is_f64, n, close_idx, n_idx, side, out));
    if (n_idx == 1) return FMK_OK;
    for (int64_t i = 0; i < n_idx; ++i)
        if (close_idx[i] < -1 || close_idx[i] >= n)
            return fmk_set_error(ctx, FMK_E_ARG, "comp_bar_microstructure: close index %lld is outside [-1, %lld)",
                                 (long long)close_idx[i], (long long)n);
    const int64_t nb = n_idx - 1;
    DevBag bag(ctx);
    double *d_p;
    void *d_a;
    int64_t *d_ci;
    int8_t *d_s;
    FMK_TRY(bag.up(price, n, &d_p));
    FMK_TRY(bag.up_amount(amount, amount_is_f64, n, &d_a));
    FMK_TRY(bag.up(close_idx, n_idx, &d_ci));
    FMK_TRY(bag.up(side, n, &d_s));
    fmk_microstructure_out d;
    double **dc[] = {&d.kyle_lambda, &d.kyle_t, &d.amihud_lambda, &d.amihud_t, &d.hasbrouck_lambda, &d.hasbrouck_t, &d.serial_cov,
                     &d.roll_spread};
    double *const hc[] = {out->kyle_lambda, out->kyle_t, out->amihud_lambda, out->amihud_t, out->hasbrouck_lambda, out->hasbrouck_t,
                          out->serial_cov, out->roll_spread};
    for (auto p : dc) FMK_TRY(bag.out(nb, p));
    FMK_TRY(fmk_comp_bar_microstructure_dev(ctx, d_p, d_a, amount_is_f64, n, d_ci, n_idx, d_s, &d));
    for (int k = 0; k < 8; ++k) FMK_TRY(down(ctx, hc[k], (const double *)*dc[k], nb));
    return FMK_OK;
}

int fmk_comp_lagged_returns(fmk_ctx *ctx, const int64_t *ts, const double *close_, int64_t n,
                            double return_window_sec, int is_log, double *out)
{
    if (!(return_window_sec > 0))
        return fmk_set_error(ctx, FMK_E_ARG, "The return window must be greater than zero.");
    if (n <= 0) return FMK_OK;
    DevBag bag(ctx);
    int64_t *d_ts;
    double *d_c, *d_o;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.up(close_, n, &d_c));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_comp_lagged_returns_dev(ctx, d_ts, d_c, n, return_window_sec, is_log, d_o));
    return down(ctx, out, d_o, n);
}

int fmk_ewmst(fmk_ctx *ctx, const int64_t *ts, const double *y, int64_t n, double half_life, double sigma_floor,
              int mean0, double *out)
{
    if (n <= 0) return FMK_OK;
    DevBag bag(ctx);
    int64_t *d_ts;
    double *d_y, *d_o;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.up(y, n, &d_y));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_ewmst_dev(ctx, d_ts, d_y, n, half_life, sigma_floor, mean0, d_o));
    return down(ctx, out, d_o, n);
}

int fmk_ewms(fmk_ctx *ctx, const double *y, int64_t n, int64_t span, double *out)
{
    if (n <= 0) return FMK_OK;
    DevBag bag(ctx);
    double *d_y, *d_o;
    FMK_TRY(bag.up(y, n, &d_y));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_ewms_dev(ctx, d_y, n, span, d_o));
    return down(ctx, out, d_o, n);
}

int fmk_realized_vol(fmk_ctx *ctx, const double *r, int64_t n, int64_t window, int is_sample, double *out)
{
    if (window < 1) return fmk_set_error(ctx, FMK_E_ARG, "window must be at least 1");
    if (n <= 0) return FMK_OK;
    DevBag bag(ctx);
    double *d_r, *d_o;
    FMK_TRY(bag.up(r, n, &d_r));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_realized_vol_dev(ctx, d_r, n, window, is_sample, d_o));
    return down(ctx, out, d_o, n);
}

int fmk_merge_split_trades(fmk_ctx *ctx, const int64_t *ts, const double *price, const float *amount,
                           const uint8_t *is_buyer_maker, int64_t n, int64_t *out_ts, double *out_price,
                           float *out_amount, int8_t *out_side, int64_t capacity, int64_t *n_merged)
{
    if (n <= 0) return fmk_set_error(ctx, FMK_E_ARG, "merge_split_trades: empty input");
    DevBag bag(ctx);
    int64_t *d_ts, *d_ots = nullptr;
    double *d_p, *d_op = nullptr;
    float *d_a, *d_oa = nullptr;
    uint8_t *d_m = nullptr;
    int8_t *d_os = nullptr;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.up(price, n, &d_p));
    FMK_TRY(bag.up(amount, n, &d_a));
    if (is_buyer_maker) FMK_TRY(bag.up(is_buyer_maker, n, &d_m));
    if (out_ts) {
        FMK_TRY(bag.out(n, &d_ots));
        FMK_TRY(bag.out(n, &d_op));
        FMK_TRY(bag.out(n, &d_oa));
        if (out_side && is_buyer_maker) FMK_TRY(bag.out(n, &d_os));
    }
    int64_t m = 0;
    FMK_TRY(fmk_merge_split_trades_dev(ctx, d_ts, d_p, d_a, d_m, n, d_ots, d_op, d_oa, d_os, out_ts ? n : 0, &m));
    if (n_merged) *n_merged = m;
    if (!out_ts) return FMK_OK;
    if (capacity < m)
        return fmk_set_error(ctx, FMK_E_CAPACITY, "merge_split_trades: %lld merged trades, capacity %lld", (long long)m,
                             (long long)capacity);
    FMK_TRY(down(ctx, out_ts, d_ots, m));
    FMK_TRY(down(ctx, out_price, d_op, m));
    FMK_TRY(down(ctx, out_amount, d_oa, m));
    if (d_os) FMK_TRY(down(ctx, out_side, d_os, m));
    return FMK_OK;
}

int fmk_comp_trade_side_vector(fmk_ctx *ctx, const double *price, int64_t n, int8_t *out)
{
    if (n <= 0) return fmk_set_error(ctx, FMK_E_ARG, "comp_trade_side_vector: empty input");
    DevBag bag(ctx);
    double *d_p;
    int8_t *d_o;
    FMK_TRY(bag.up(price, n, &d_p));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_comp_trade_side_vector_dev(ctx, d_p, n, d_o));
    return down(ctx, out, d_o, n);
}

int fmk_cusum_bar_indexer(fmk_ctx *ctx, const int64_t *ts, const double *price, double *sigma, int64_t n,
                          double sigma_floor, double sigma_mult, int64_t *out, int64_t capacity, int64_t *n_out)
{
    if (n <= 0) return fmk_set_error(ctx, FMK_E_ARG, "Prices, timestamps, and sigma arrays must have the same length.");
    DevBag bag(ctx);
    int64_t *d_ts, *d_o = nullptr;
    double *d_p, *d_s;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.up(price, n, &d_p));
    FMK_TRY(bag.up((const double *)sigma, n, &d_s));
    if (out) FMK_TRY(bag.out(n, &d_o));
    int64_t m = 0;
    FMK_TRY(fmk_cusum_bar_indexer_dev(ctx, d_ts, d_p, d_s, n, sigma_floor, sigma_mult, d_o, out ? n : 0, &m, nullptr));
    if (n_out) *n_out = m;
    FMK_TRY(down(ctx, sigma, (const double *)d_s, n));          // the reference forward-fills sigma in place
    if (!out) return FMK_OK;
    if (capacity < m)
        return fmk_set_error(ctx, FMK_E_CAPACITY, "cusum: %lld close indices, capacity %lld", (long long)m,
                             (long long)capacity);
    return down(ctx, out, (const int64_t *)d_o, m);
}

int fmk_volume_profile_rolling(fmk_ctx *ctx, const int64_t *bar_ts, const double *highs, const double *lows,
                               const int64_t *level_offsets, const int32_t *price_levels, const float *buy_volumes,
                               const float *sell_volumes, int64_t n_bars, int64_t first_bar, int64_t window_ns,
                               int64_t n_bins, double price_tick, double va_pct, int32_t *poc, int32_t *hva, int32_t *lva,
                               float *pct)
{
    if (n_bars <= 0) return fmk_set_error(ctx, FMK_E_ARG, "Input arrays should have the same length and be non-empty.");
    const int64_t nl = level_offsets[n_bars];
    DevBag bag(ctx);
    int64_t *d_ts, *d_off;
    double *d_hi, *d_lo;
    int32_t *d_pl, *d_poc, *d_hva, *d_lva;
    float *d_b, *d_s, *d_pct;
    FMK_TRY(bag.up(bar_ts, n_bars, &d_ts));
    FMK_TRY(bag.up(highs, n_bars, &d_hi));
    FMK_TRY(bag.up(lows, n_bars, &d_lo));
    FMK_TRY(bag.up(level_offsets, n_bars + 1, &d_off));
    FMK_TRY(bag.up(price_levels, nl, &d_pl));
    FMK_TRY(bag.up(buy_volumes, nl, &d_b));
    FMK_TRY(bag.up(sell_volumes, nl, &d_s));
    FMK_TRY(bag.out(n_bars, &d_poc));
    FMK_TRY(bag.out(n_bars, &d_hva));
    FMK_TRY(bag.out(n_bars, &d_lva));
    FMK_TRY(bag.out(n_bars, &d_pct));
    FMK_TRY(fmk_volume_profile_rolling_dev(ctx, d_ts, d_hi, d_lo, d_off, d_pl, d_b, d_s, n_bars, first_bar, window_ns,
                                           n_bins, price_tick, va_pct, d_poc, d_hva, d_lva, d_pct));
    FMK_TRY(down(ctx, poc, (const int32_t *)d_poc, n_bars));
    FMK_TRY(down(ctx, hva, (const int32_t *)d_hva, n_bars));
    FMK_TRY(down(ctx, lva, (const int32_t *)d_lva, n_bars));
    return down(ctx, pct, (const float *)d_pct, n_bars);
}

int fmk_volume_profile_developing(fmk_ctx *ctx, const double *highs, const double *lows, const int64_t *level_offsets,
                                  const int32_t *price_levels, const float *buy_volumes, const float *sell_volumes, int64_t n_bars,
                                  const int64_t *range_starts, const int64_t *range_ends, const int64_t *out_offsets,
                                  int64_t n_ranges, int64_t n_bins, double price_tick, double va_pct, int64_t chunk_bars,
                                  int32_t *poc, int32_t *hva, int32_t *lva, int64_t n_out)
{
    if (n_bars <= 0) return fmk_set_error(ctx, FMK_E_ARG, "Input arrays should have the same length and be non-empty.");
    for (int64_t r = 0; r < n_ranges; ++r)                        // (every other rule is the _dev entry's)
        if (range_starts[r] < range_ends[r] && (out_offsets[r] < 0 || out_offsets[r] + (range_ends[r] - range_starts[r]) > n_out))
            return fmk_set_error(ctx, FMK_E_ARG, "volume_profile_developing: the outputs of range %lld lie outside the %lld elements given",
                                 (long long)r, (long long)n_out);
    const int64_t nl = level_offsets[n_bars];
    DevBag bag(ctx);
    int64_t *d_off;
    double *d_hi, *d_lo;
    int32_t *d_pl, *d_poc, *d_hva, *d_lva;
    float *d_b, *d_s;
    FMK_TRY(bag.up(highs, n_bars, &d_hi));
    FMK_TRY(bag.up(lows, n_bars, &d_lo));
    FMK_TRY(bag.up(level_offsets, n_bars + 1, &d_off));
    FMK_TRY(bag.up(price_levels, nl, &d_pl));
    FMK_TRY(bag.up(buy_volumes, nl, &d_b));
    FMK_TRY(bag.up(sell_volumes, nl, &d_s));
    FMK_TRY(bag.up((const int32_t *)poc, n_out, &d_poc));         // elements that no range covers keep what they hold
    FMK_TRY(bag.up((const int32_t *)hva, n_out, &d_hva));
    FMK_TRY(bag.up((const int32_t *)lva, n_out, &d_lva));
    FMK_TRY(fmk_volume_profile_developing_dev(ctx, d_hi, d_lo, d_off, d_pl, d_b, d_s, n_bars, range_starts, range_ends, out_offsets,
                                              n_ranges, n_bins, price_tick, va_pct, chunk_bars, d_poc, d_hva, d_lva));
    FMK_TRY(down(ctx, poc, (const int32_t *)d_poc, n_out));
    FMK_TRY(down(ctx, hva, (const int32_t *)d_hva, n_out));
    return down(ctx, lva, (const int32_t *)d_lva, n_out);
}

}  // extern "C"

extern "C" {

int fmk_triple_barrier(fmk_ctx *ctx, const int64_t *ts, const double *close_, int64_t n, const int64_t *event_idx,
                       const double *targets, const int8_t *side, int64_t n_events, double bottom_mult, double top_mult,
                       double vertical_barrier_sec, double min_close_time_sec, double min_ret, int8_t *labels, int64_t *touch_idx,
                       double *ret, double *max_rb_ratio, int64_t *n_skipped)
{
    if (n_events <= 0) return fmk_set_error(ctx, FMK_E_ARG, "The event_idxs array must not be empty.");
    if (n <= 0) return fmk_set_error(ctx, FMK_E_ARG, "triple_barrier: event indices outside the (empty) tape");
    DevBag bag(ctx);
    int64_t *d_ts, *d_ev, *d_touch, *d_skip;
    double *d_c, *d_tg, *d_ret, *d_ratio;
    int8_t *d_sd = nullptr, *d_lab;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.up(close_, n, &d_c));
    FMK_TRY(bag.up(event_idx, n_events, &d_ev));
    FMK_TRY(bag.up(targets, n_events, &d_tg));
    if (side) FMK_TRY(bag.up(side, n_events, &d_sd));
    FMK_TRY(bag.out(n_events, &d_lab));
    FMK_TRY(bag.out(n_events, &d_touch));
    FMK_TRY(bag.out(n_events, &d_ret));
    FMK_TRY(bag.out(n_events, &d_ratio));
    FMK_TRY(bag.out(1, &d_skip));
    FMK_TRY(fmk_memset(ctx, d_skip, 0, sizeof(int64_t)));
    FMK_TRY(fmk_triple_barrier_dev(ctx, d_ts, d_c, n, d_ev, d_tg, d_sd, n_events, bottom_mult, top_mult, vertical_barrier_sec,
                                   min_close_time_sec, min_ret, d_lab, d_touch, d_ret, d_ratio, d_skip));
    FMK_TRY(down(ctx, labels, d_lab, n_events));
    FMK_TRY(down(ctx, touch_idx, d_touch, n_events));
    FMK_TRY(down(ctx, ret, d_ret, n_events));
    FMK_TRY(down(ctx, max_rb_ratio, d_ratio, n_events));
    FMK_TRY(down(ctx, n_skipped, d_skip, 1));
    return FMK_OK;
}

int fmk_trend_scanning(fmk_ctx *ctx, const double *y, int64_t n, const int64_t *event_idx, int64_t n_events, int64_t min_len,
                       int64_t max_len, int64_t step, int8_t *labels, double *t_value, int64_t *touch_idx, double *ret,
                       int64_t *n_skipped)
{
    FMK_TRY(fmk_rule_trend(ctx, min_len, max_len, step));
    if (n_events < 0 || n < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    if (n_skipped) *n_skipped = 0;
    if (n_events == 0) return FMK_OK;
    if (n == 0) return fmk_set_error(ctx, FMK_E_ARG, "trend_scanning: event indices outside the (empty) series");
    DevBag bag(ctx);
    double *d_y, *d_t, *d_ret;
    int64_t *d_ev, *d_touch, *d_skip;
    int8_t *d_lab;
    FMK_TRY(bag.up(y, n, &d_y));
    FMK_TRY(bag.up(event_idx, n_events, &d_ev));
    FMK_TRY(bag.out(n_events, &d_lab));
    FMK_TRY(bag.out(n_events, &d_t));
    FMK_TRY(bag.out(n_events, &d_touch));
    FMK_TRY(bag.out(n_events, &d_ret));
    FMK_TRY(bag.out(1, &d_skip));
    FMK_TRY(fmk_memset(ctx, d_skip, 0, sizeof(int64_t)));
    FMK_TRY(fmk_trend_scanning_dev(ctx, d_y, n, d_ev, n_events, min_len, max_len, step, d_lab, d_t, d_touch, d_ret, d_skip));
    FMK_TRY(down(ctx, labels, d_lab, n_events));
    FMK_TRY(down(ctx, t_value, d_t, n_events));
    FMK_TRY(down(ctx, touch_idx, d_touch, n_events));
    FMK_TRY(down(ctx, ret, d_ret, n_events));
    FMK_TRY(down(ctx, n_skipped, d_skip, 1));
    return FMK_OK;
}

int fmk_label_concurrency(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, int64_t n_events, int64_t n,
                          int16_t *concurrency)
{
    DevBag bag(ctx);
    int64_t *d_ev, *d_touch;
    int16_t *d_c;
    FMK_TRY(bag.up(event_idx, n_events, &d_ev));
    FMK_TRY(bag.up(touch_idx, n_events, &d_touch));
    FMK_TRY(bag.out(n, &d_c));
    FMK_TRY(fmk_label_concurrency_dev(ctx, d_ev, d_touch, n_events, n, d_c));
    FMK_TRY(down(ctx, concurrency, d_c, n));
    return FMK_OK;
}

int fmk_label_weights(fmk_ctx *ctx, const double *close_, const int16_t *concurrency, int64_t n, const int64_t *event_idx,
                      const int64_t *touch_idx, int64_t n_events, double *avg_uniqueness, double *return_attribution)
{
    DevBag bag(ctx);
    int64_t *d_ev, *d_touch;
    int16_t *d_c;
    double *d_p = nullptr, *d_u = nullptr, *d_a = nullptr;
    if (close_) FMK_TRY(bag.up(close_, n, &d_p));
    FMK_TRY(bag.up(concurrency, n, &d_c));
    FMK_TRY(bag.up(event_idx, n_events, &d_ev));
    FMK_TRY(bag.up(touch_idx, n_events, &d_touch));
    if (avg_uniqueness) FMK_TRY(bag.out(n_events, &d_u));
    if (return_attribution) FMK_TRY(bag.out(n_events, &d_a));
    FMK_TRY(fmk_label_weights_dev(ctx, d_p, d_c, n, d_ev, d_touch, n_events, d_u, d_a));
    FMK_TRY(down(ctx, avg_uniqueness, d_u, n_events));
    FMK_TRY(down(ctx, return_attribution, d_a, n_events));
    return FMK_OK;
}

int fmk_bet_size_path(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, const double *signal, int64_t n_events,
                      int64_t n, double step, double *out_value, int16_t *out_count)
{
    FMK_TRY(fmk_rule_bet(ctx, "bet_size_path", n_events, n, step));
    DevBag bag(ctx);
    int64_t *d_ev, *d_touch;
    double *d_sig, *d_v;
    int16_t *d_c = nullptr;
    FMK_TRY(bag.up(event_idx, n_events, &d_ev));
    FMK_TRY(bag.up(touch_idx, n_events, &d_touch));
    FMK_TRY(bag.up(signal, n_events, &d_sig));
    FMK_TRY(bag.out(n, &d_v));
    if (out_count) FMK_TRY(bag.out(n, &d_c));
    FMK_TRY(fmk_bet_size_path_dev(ctx, d_ev, d_touch, d_sig, n_events, n, step, d_v, d_c));
    FMK_TRY(down(ctx, out_value, (const double *)d_v, n));
    FMK_TRY(down(ctx, out_count, (const int16_t *)d_c, n));
    return FMK_OK;
}

int fmk_bet_size_at(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, const double *signal, int64_t n_events,
                    int64_t n, double step, const int64_t *idx, int64_t n_idx, double *out)
{
    FMK_TRY(fmk_rule_bet(ctx, "bet_size_at", n_events, n, step));
    if (n_idx < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    DevBag bag(ctx);
    int64_t *d_ev, *d_touch, *d_idx;
    double *d_sig, *d_o;
    FMK_TRY(bag.up(event_idx, n_events, &d_ev));
    FMK_TRY(bag.up(touch_idx, n_events, &d_touch));
    FMK_TRY(bag.up(signal, n_events, &d_sig));
    FMK_TRY(bag.up(idx, n_idx, &d_idx));
    FMK_TRY(bag.out(n_idx, &d_o));
    FMK_TRY(fmk_bet_size_at_dev(ctx, d_ev, d_touch, d_sig, n_events, n, step, d_idx, n_idx, d_o));
    FMK_TRY(down(ctx, out, (const double *)d_o, n_idx));
    return FMK_OK;
}

int fmk_bet_size_budget(fmk_ctx *ctx, const int64_t *event_idx, const int64_t *touch_idx, const int8_t *side, int64_t n_events,
                        int64_t n, double *out_m, int64_t *out_max2)
{
    FMK_TRY(fmk_rule_bet(ctx, "bet_size_budget", n_events, n, 0.0));
    DevBag bag(ctx);
    int64_t *d_ev, *d_touch, *d_max;
    int8_t *d_sd;
    double *d_m;
    FMK_TRY(bag.up(event_idx, n_events, &d_ev));
    FMK_TRY(bag.up(touch_idx, n_events, &d_touch));
    FMK_TRY(bag.up(side, n_events, &d_sd));
    FMK_TRY(bag.out(n, &d_m));
    FMK_TRY(bag.out(2, &d_max));
    FMK_TRY(fmk_bet_size_budget_dev(ctx, d_ev, d_touch, d_sd, n_events, n, d_m, d_max));
    FMK_TRY(down(ctx, out_m, (const double *)d_m, n));
    FMK_TRY(down(ctx, out_max2, (const int64_t *)d_max, 2));
    return FMK_OK;
}

int fmk_cusum_filter(fmk_ctx *ctx, const double *x, int64_t n, const double *thr, int64_t n_thr, int64_t *out, int64_t capacity,
                     int64_t *n_out)
{
    if (n <= 1) return fmk_set_error(ctx, FMK_E_ARG, "Input time series must have at least 2 elements.");
    if (n_thr != 1 && n_thr != n)
        return fmk_set_error(ctx, FMK_E_ARG, "Threshold array must either contain 1 const. element or len(raw_time_series) elements.");
    DevBag bag(ctx);
    double *d_x, *d_thr;
    int64_t *d_o = nullptr;
    FMK_TRY(bag.up(x, n, &d_x));
    FMK_TRY(bag.up(thr, n_thr, &d_thr));
    if (out) FMK_TRY(bag.out(n - 1, &d_o));                       // at most one event per tick from 1 on
    int64_t m = 0;
    FMK_TRY(fmk_cusum_filter_dev(ctx, d_x, n, d_thr, n_thr, d_o, out ? n - 1 : 0, &m, nullptr));
    if (n_out) *n_out = m;
    if (!out) return FMK_OK;
    if (capacity < m)
        return fmk_set_error(ctx, FMK_E_CAPACITY, "cusum_filter: %lld event indices, capacity %lld", (long long)m, (long long)capacity);
    return down(ctx, out, (const int64_t *)d_o, m);
}

// both flavours of the CSW CUSUM test: window_size < 0 selects developing
static int cusum_test_host(fmk_ctx *ctx, const double *x, int64_t n, int64_t window_size, int64_t warmup_period, double *up,
                           double *dn, double *crit_up, double *crit_down)
{
    DevBag bag(ctx);
    double *d_x, *d_o;
    FMK_TRY(bag.up(x, n, &d_x));
    FMK_TRY(bag.out(4 * n, &d_o));
    if (window_size < 0)
        FMK_TRY(fmk_cusum_test_developing_dev(ctx, d_x, n, warmup_period, d_o, d_o + n, d_o + 2 * n, d_o + 3 * n));
    else
        FMK_TRY(fmk_cusum_test_rolling_dev(ctx, d_x, n, window_size, warmup_period, d_o, d_o + n, d_o + 2 * n, d_o + 3 * n));
    FMK_TRY(down(ctx, up, (const double *)d_o, n));
    FMK_TRY(down(ctx, dn, (const double *)d_o + n, n));
    FMK_TRY(down(ctx, crit_up, (const double *)d_o + 2 * n, n));
    return down(ctx, crit_down, (const double *)d_o + 3 * n, n);
}

int fmk_cusum_test_rolling(fmk_ctx *ctx, const double *x, int64_t n, int64_t window_size, int64_t warmup_period, double *up,
                           double *dn, double *crit_up, double *crit_down)
{
    if (warmup_period < 2) return fmk_set_error(ctx, FMK_E_ARG, "warmup_period must be at least 2.");
    return cusum_test_host(ctx, x, n, window_size < 0 ? 0 : window_size, warmup_period, up, dn, crit_up, crit_down);
}

int fmk_cusum_test_developing(fmk_ctx *ctx, const double *x, int64_t n, int64_t warmup_period, double *up, double *dn,
                              double *crit_up, double *crit_down)
{
    if (warmup_period < 2) return fmk_set_error(ctx, FMK_E_ARG, "warmup_period must be at least 2.");
    return cusum_test_host(ctx, x, n, -1, warmup_period, up, dn, crit_up, crit_down);
}

// the rolling-window moments (fmk_rolling.hip) and order statistics (fmk_order.hip) through series_host
int fmk_sma(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out)
{
    return series_host(ctx, fmk_rule_window(ctx, nullptr, window), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_sma_dev(ctx, d_x, n, window, d_o); });
}

int fmk_zscore(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, int64_t ddof, double *out)
{
    FMK_TRY(fmk_rule_window(ctx, nullptr, window));
    return series_host(ctx, fmk_rule_zscore(ctx, window, ddof), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_zscore_dev(ctx, d_x, n, window, ddof, d_o); });
}

int fmk_rolling_variance(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, int64_t ddof, int64_t min_periods, double *out)
{
    return series_host(ctx, fmk_rule_window(ctx, nullptr, window), x, n, out, [=](const double *d_x, double *d_o) {
        return fmk_rolling_variance_dev(ctx, d_x, n, window, ddof, min_periods, d_o);
    });
}

int fmk_variance_ratio_1_4(fmk_ctx *ctx, const double *price, int64_t n, int64_t window, int64_t ddof, int is_log, double *out)
{
    return series_host(ctx, fmk_rule_window(ctx, nullptr, window), price, n, out, [=](const double *d_x, double *d_o) {
        return fmk_variance_ratio_1_4_dev(ctx, d_x, n, window, ddof, is_log != 0, d_o);
    });
}

int fmk_burst_ratio(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out)
{
    return series_host(ctx, fmk_rule_window(ctx, nullptr, window), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_burst_ratio_dev(ctx, d_x, n, window, d_o); });
}

int fmk_roc(fmk_ctx *ctx, const double *x, int64_t n, int64_t period, double *out)
{
    return series_host(ctx, fmk_rule_roc(ctx, period), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_roc_dev(ctx, d_x, n, period, d_o); });
}

int fmk_pct_change(fmk_ctx *ctx, const double *x, int64_t n, int64_t periods, double *out)
{
    return series_host(ctx, fmk_rule_pct_change(ctx, periods), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_pct_change_dev(ctx, d_x, n, periods, d_o); });
}

int fmk_stoch_k(fmk_ctx *ctx, const double *close, const double *low, const double *high, int64_t n, int64_t length, double *out)
{
    return hlc_host(ctx, fmk_rule_stoch_k(ctx, length), close, low, high, n, out,
                    [=](const double *c, const double *l, const double *h, double *o) { return fmk_stoch_k_dev(ctx, c, l, h, n, length, o); });
}

// the recursive indicators (fmk_recur.hip)
int fmk_ewma(fmk_ctx *ctx, const double *y, int64_t n, double span, double *out)
{
    FMK_TRY(fmk_rule_ewma(ctx, span));
    return series_host(ctx, fmk_series_check(ctx, "ewma", n), y, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_ewma_dev(ctx, d_x, n, span, d_o); });
}

int fmk_rsi_wilder(fmk_ctx *ctx, const double *close, int64_t n, int64_t window, double *out)
{
    FMK_TRY(fmk_rule_rsi_wilder(ctx, window));
    return series_host(ctx, fmk_series_check(ctx, "rsi_wilder", n), close, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_rsi_wilder_dev(ctx, d_x, n, window, d_o); });
}

int fmk_true_range(fmk_ctx *ctx, const double *high, const double *low, const double *close, int64_t n, double *out)
{
    return hlc_host(ctx, fmk_series_check(ctx, "true_range", n), high, low, close, n, out,
                    [=](const double *h, const double *l, const double *c, double *o) { return fmk_true_range_dev(ctx, h, l, c, n, o); });
}

int fmk_atr(fmk_ctx *ctx, const double *high, const double *low, const double *close, int64_t n, int64_t window, int ema_based,
            int normalize, double *out)
{
    FMK_TRY(fmk_rule_atr(ctx, window));
    return hlc_host(ctx, fmk_series_check(ctx, "atr", n), high, low, close, n, out,
                    [=](const double *h, const double *l, const double *c, double *o) {
                        return fmk_atr_dev(ctx, h, l, c, n, window, ema_based, normalize, o);
                    });
}

int fmk_adx(fmk_ctx *ctx, const double *high, const double *low, const double *close, int64_t n, int64_t length, double *out)
{
    FMK_TRY(fmk_rule_adx(ctx, length));
    return hlc_host(ctx, fmk_series_check(ctx, "adx_core", n), high, low, close, n, out,
                    [=](const double *h, const double *l, const double *c, double *o) { return fmk_adx_dev(ctx, h, l, c, n, length, o); });
}

// the running-sum indicators (fmk_runsum.hip)
int fmk_bollinger_percent_b(fmk_ctx *ctx, const double *close, int64_t n, int64_t window, double num_std, double *out)
{
    FMK_TRY(fmk_rule_bollinger(ctx, window));
    return series_host(ctx, fmk_series_check(ctx, "bollinger_percent_b", n), close, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_bollinger_percent_b_dev(ctx, d_x, n, window, num_std, d_o); });
}

int fmk_vwap_distance(fmk_ctx *ctx, const double *close, const double *volume, int64_t n, int64_t n_periods, int is_log, double *out)
{
    FMK_TRY(fmk_rule_vwap_distance(ctx, n_periods));
    return pair_host(ctx, fmk_series_check(ctx, "vwap_distance", n), close, volume, n, out,
                     [=](const double *c, const double *v, double *o) { return fmk_vwap_distance_dev(ctx, c, v, n, n_periods, is_log, o); });
}

int fmk_flow_acceleration(fmk_ctx *ctx, const double *volumes, int64_t n, int64_t window, int64_t recent_periods, double *out)
{
    FMK_TRY(fmk_rule_flow_acceleration(ctx, recent_periods));
    return series_host(ctx, fmk_series_check(ctx, "comp_flow_acceleration", n), volumes, n, out, [=](const double *d_x, double *d_o) {
        return fmk_flow_acceleration_dev(ctx, d_x, n, window, recent_periods, d_o);
    });
}

int fmk_vpin(fmk_ctx *ctx, const double *volume_buy, const double *volume_sell, int64_t n, int64_t window, float *out)
{
    FMK_TRY(fmk_rule_vpin(ctx, window));
    return pair_host(ctx, fmk_series_check(ctx, "vpin", n), volume_buy, volume_sell, n, out,
                     [=](const double *b, const double *s, float *o) { return fmk_vpin_dev(ctx, b, s, n, window, o); });
}

int fmk_parkinson_range(fmk_ctx *ctx, const double *high, const double *low, int64_t n, double *out)
{
    return pair_host(ctx, fmk_series_check(ctx, "parkinson_range", n), high, low, n, out,
                     [=](const double *h, const double *l, double *o) { return fmk_parkinson_range_dev(ctx, h, l, n, o); });
}

// the rolling price-volume correlation (fmk_corr.hip)
int fmk_price_volume_corr(fmk_ctx *ctx, const double *price, const double *volume, int64_t n, int64_t window, double *out)
{
    FMK_TRY(fmk_rule_window(ctx, "rolling_price_volume_correlation", window));
    return pair_host(ctx, fmk_series_check(ctx, "rolling_price_volume_correlation", n), price, volume, n, out,
                     [=](const double *p, const double *v, double *o) { return fmk_price_volume_corr_dev(ctx, p, v, n, window, o); });
}

// the window statistics (fmk_shape.hip)
int fmk_rolling_kurtosis(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out)
{
    return series_host(ctx, fmk_rule_window(ctx, nullptr, window), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_rolling_kurtosis_dev(ctx, d_x, n, window, d_o); });
}

int fmk_trend_slope(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out)
{
    return series_host(ctx, fmk_rule_window(ctx, nullptr, window), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_trend_slope_dev(ctx, d_x, n, window, d_o); });
}

int fmk_hurst_exponent(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out)
{
    FMK_TRY(fmk_rule_window(ctx, nullptr, window));
    return series_host(ctx, fmk_rule_hurst(ctx, window), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_hurst_exponent_dev(ctx, d_x, n, window, d_o); });
}

int fmk_bipower_variation(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, double *out)
{
    return series_host(ctx, fmk_rule_window(ctx, nullptr, window), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_bipower_variation_dev(ctx, d_x, n, window, d_o); });
}

// the approximate entropy (fmk_entropy.hip)
int fmk_approximate_entropy(fmk_ctx *ctx, const double *x, int64_t n, int64_t window, int64_t m, double tolerance, double *out)
{
    return series_host(ctx, fmk_rule_apen(ctx, window, m, tolerance), x, n, out,
                       [=](const double *d_x, double *d_o) { return fmk_approximate_entropy_dev(ctx, d_x, n, window, m, tolerance, d_o); });
}

// the bar clock, run lengths and the opening range (fmk_clock.hip)
int fmk_bar_duration(fmk_ctx *ctx, const int64_t *ts, int64_t n, int64_t periods, double *out)
{
    FMK_TRY(fmk_series_check(ctx, "bar_duration", n));
    DevBag bag(ctx);
    int64_t *d_ts;
    double *d_o;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_bar_duration_dev(ctx, d_ts, n, periods, d_o));
    return down(ctx, out, (const double *)d_o, n);
}

int fmk_bar_duration_ewma(fmk_ctx *ctx, const int64_t *ts, int64_t n, double span, double *out)
{
    FMK_TRY(fmk_rule_ewma(ctx, span));
    FMK_TRY(fmk_series_check(ctx, "bar_duration_ewma", n));
    DevBag bag(ctx);
    int64_t *d_ts;
    double *d_o;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_bar_duration_ewma_dev(ctx, d_ts, n, span, d_o));
    return down(ctx, out, (const double *)d_o, n);
}

int fmk_bar_rate(fmk_ctx *ctx, const int64_t *ts, int64_t n, double window_sec, int64_t window_ns, double *out)
{
    FMK_TRY(fmk_rule_bar_rate(ctx, window_ns));
    FMK_TRY(fmk_series_check(ctx, "bar_rate", n));
    DevBag bag(ctx);
    int64_t *d_ts;
    double *d_o;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_bar_rate_dev(ctx, d_ts, n, window_sec, window_ns, d_o));
    return down(ctx, out, (const double *)d_o, n);
}

int fmk_dir_run_len(fmk_ctx *ctx, const double *x, int64_t n, int8_t *out)
{
    FMK_TRY(fmk_series_check(ctx, "dir_run_len", n));
    DevBag bag(ctx);
    double *d_x;
    int8_t *d_o;
    FMK_TRY(bag.up(x, n, &d_x));
    FMK_TRY(bag.out(n, &d_o));
    FMK_TRY(fmk_dir_run_len_dev(ctx, d_x, n, d_o));
    return down(ctx, out, (const int8_t *)d_o, n);
}

int fmk_orb_break(fmk_ctx *ctx, const int64_t *ts, const double *high, const double *low, const double *close, int64_t n,
                  uint8_t *orb_long, uint8_t *orb_short)
{
    FMK_TRY(fmk_series_check(ctx, "orb_break", n));
    DevBag bag(ctx);
    int64_t *d_ts;
    double *d_h, *d_l, *d_c;
    uint8_t *d_lg, *d_sh;
    FMK_TRY(bag.up(ts, n, &d_ts));
    FMK_TRY(bag.up(high, n, &d_h));
    FMK_TRY(bag.up(low, n, &d_l));
    FMK_TRY(bag.up(close, n, &d_c));
    FMK_TRY(bag.out(n, &d_lg));
    FMK_TRY(bag.out(n, &d_sh));
    FMK_TRY(fmk_orb_break_dev(ctx, d_ts, d_h, d_l, d_c, n, d_lg, d_sh));
    FMK_TRY(down(ctx, orb_long, (const uint8_t *)d_lg, n));
    return down(ctx, orb_short, (const uint8_t *)d_sh, n);
}

// the causal FIR filter (fmk_fir.hip): w stays a host array, the _dev entry uploads it
int fmk_fir(fmk_ctx *ctx, const double *x, int64_t n, const double *w, int64_t width, double *out)
{
    FMK_TRY(fmk_rule_fir(ctx, w, width, x, out));
    FMK_TRY(fmk_series_check(ctx, "fir", n));
    if (n == 0) return FMK_OK;
    return series_host(ctx, FMK_OK, x, n, out, [=](const double *d_x, double *d_o) { return fmk_fir_dev(ctx, d_x, n, w, width, d_o); });
}

// the ADF / SADF statistic (fmk_sadf.hip); end_idx == NULL: end point e is element e
int fmk_sadf(fmk_ctx *ctx, const double *y, int64_t n, const int64_t *end_idx, int64_t n_end, int64_t min_len, int64_t max_len,
             int64_t step, int64_t lags, int trend, double *stat, int64_t *start, int64_t *n_skipped)
{
    FMK_TRY(fmk_rule_sadf(ctx, min_len, max_len, step, lags, trend, y, stat, start));
    if (n_end < 0 || n < 0) return fmk_set_error(ctx, FMK_E_ARG, "negative dimensions are not allowed");
    if (n_skipped) *n_skipped = 0;
    if (n_end == 0) return FMK_OK;
    if (n == 0) return fmk_set_error(ctx, FMK_E_ARG, "sadf: end points outside the (empty) series");
    DevBag bag(ctx);
    double *d_y, *d_stat;
    int64_t *d_ev = nullptr, *d_start, *d_skip;
    FMK_TRY(bag.up(y, n, &d_y));
    if (end_idx) FMK_TRY(bag.up(end_idx, n_end, &d_ev));
    FMK_TRY(bag.out(n_end, &d_stat));
    FMK_TRY(bag.out(n_end, &d_start));
    FMK_TRY(bag.out(1, &d_skip));
    FMK_TRY(fmk_memset(ctx, d_skip, 0, sizeof(int64_t)));
    FMK_TRY(fmk_sadf_dev(ctx, d_y, n, d_ev, n_end, min_len, max_len, step, lags, trend, d_stat, d_start, d_skip));
    FMK_TRY(down(ctx, stat, d_stat, n_end));
    FMK_TRY(down(ctx, start, d_start, n_end));
    FMK_TRY(down(ctx, n_skipped, d_skip, 1));
    return FMK_OK;
}

// the encoded-series entropies (fmk_lz.hip): edges stays a host array, the _dev entry uploads it
int fmk_encode(fmk_ctx *ctx, const double *x, int64_t n, const double *edges, int64_t n_edges, uint8_t *codes)
{
    FMK_TRY(fmk_rule_encode(ctx, edges, n_edges));
    FMK_TRY(fmk_series_check(ctx, "encode", n));
    return lz_host(ctx, x, n, codes, [=](const double *d_x, uint8_t *d_c) { return fmk_encode_dev(ctx, d_x, n, edges, n_edges, d_c); });
}

int fmk_plugin_entropy(fmk_ctx *ctx, const uint8_t *codes, int64_t n, int64_t window, int64_t word, int64_t alphabet, double *out)
{
    FMK_TRY(fmk_rule_plugin_entropy(ctx, window, word, alphabet));
    FMK_TRY(fmk_series_check(ctx, "plugin_entropy", n));
    return lz_host(ctx, codes, n, out,
                   [=](const uint8_t *d_c, double *d_o) { return fmk_plugin_entropy_dev(ctx, d_c, n, window, word, alphabet, d_o); });
}

int fmk_match_lengths(fmk_ctx *ctx, const uint8_t *codes, int64_t n, int64_t lookback, uint16_t *len)
{
    FMK_TRY(fmk_rule_match_lengths(ctx, lookback));
    FMK_TRY(fmk_series_check(ctx, "match_lengths", n));
    return lz_host(ctx, codes, n, len, [=](const uint8_t *d_c, uint16_t *d_l) { return fmk_match_lengths_dev(ctx, d_c, n, lookback, d_l); });
}

int fmk_kontoyiannis_entropy(fmk_ctx *ctx, const uint8_t *codes, int64_t n, int64_t window, int64_t lookback, double *out)
{
    FMK_TRY(fmk_rule_kontoyiannis(ctx, window, lookback));
    FMK_TRY(fmk_series_check(ctx, "kontoyiannis_entropy", n));
    return lz_host(ctx, codes, n, out,
                   [=](const uint8_t *d_c, double *d_o) { return fmk_kontoyiannis_entropy_dev(ctx, d_c, n, window, lookback, d_o); });
}

}  // extern "C"
