// fmk_recur.hip -- the indicators of the reference that carry state from bar to bar, on resident float64 series: ewma
// (feature/core/ma.py), rsi_wilder (feature/core/momentum.py), true_range and atr (feature/core/volatility.py), adx_core
// (feature/core/trend.py).  DESIGN.md section 7e.
//
// All but true_range and the SMA mode of atr are a first-order recurrence s[t] = a * s[t-1] + b[t] with one constant a, on K <= 3
// channels that share it, seeded at one index by a sum over the elements before it and followed by an elementwise map:
//   ewma        K = 2  u = y + (1 - alpha) * u, v = 1 + (1 - alpha) * v, seed (y[0], 1) at 0, out = u / v
//   rsi_wilder  K = 2  avg = ((w - 1) * avg + x) / w over the gains and the losses of close, seeded at w by the first window's sums
//               over w, out = 100 - 100 / (1 + g / l) where l > 0, NaN otherwise
//   atr (EMA)   K = 1  atr = ((w - 1) * atr + tr) / w, seeded at w - 1 by the mean of the non-NaN true ranges before it
//   adx_core    K = 3  s = s - s / L + x over true range, +DM and -DM, seeded at L by their sums; out = dx (a scratch series); then
//               K = 1  adx = (adx * (L - 1) + dx) / L, seeded at 2L - 1 by the mean of dx[L .. 2L)
// The inputs of the recurrences (gain / loss, true range, +-DM) are computed inside the passes from the price series and never stored.
//
// Schedule: a device-wide scan in three launches on the context's stream, no workgroup waits for another.  A tile is RC_THREADS
// threads x RC_ITEMS consecutive elements; a thread reads its elements straight from memory, 16 bytes per load.
//   k_rc_tiles   reads the inputs of every element once (8 B per element and series) and writes one map (a^len, B_k) per tile: what
//                the tile's elements do to the state that enters it.  Elements before the seed are the identity, the seed element is
//                the constant map to the seed value, so every call starts from a zero state.  The workgroup that holds the seed
//                index sums the seed (in index order, one lane adding) and leaves it in the scratch for the third launch.
//   k_fmk_agg_scan (fmk_wgscan.h) one workgroup; reads and rewrites the tile maps in place (8 (K + 1) B per tile, RC_AGG_UNIT maps per
//                trip): the exclusive scan, map t becoming the composition of the maps 0 .. t - 1.
//   k_rc_apply   reads the inputs again (8 B per element and series) and writes the output (8 B per element): the state that enters a
//                thread is the scanned tile map composed with the maps of the threads before it; from there the thread steps through
//                its elements with the reference's own expression.  Only that carried-in state is not the reference's arithmetic.
// true_range is an elementwise kernel and the SMA mode of atr a lockstep window walk (fmk_window.h) over true ranges computed on the
// fly: both are the reference's bits.  Outside the contract: infinities in the inputs of the scans (a^len underflows to zero and
// 0 * inf is not inf), and a state that has decayed below 2^-969 over elements that add nothing to it (969, 1 657, 9 063 of them in
// a row at windows 2, 3, 14), until every channel has taken a non-zero term again: there the reference stalls at the smallest
// subnormals for windows >= 3 (((w - 1) * 5e-324) / w rounds back to 5e-324; rsi_wilder reads 50.0 off them) and reaches 0.0 for
// windows <= 2, while the composed a^len underflows to 0.0 here (rsi_wilder NaN until the next loss).  Up to that line exact zeros
// and NaN positions are the reference's and the values within the tolerance; tests/test_gpu_recur_runs.py pins both sides.
#include <math.h>

#include "fmk_common.h"
#include "fmk_dpp.h"
#include "fmk_recur_core.h"
#include "fmk_window.h"

#define ATR_OPL 4                    // SMA mode: outputs per lane of the window walk
#define ATR_TILE (RC_THREADS * ATR_OPL)

namespace {

// ---- the inputs of the recurrences, as the reference writes them
// Python's max(a, b, c): the first of the largest, a NaN staying where it is first
__device__ __forceinline__ double rc_max3(double a, double b, double c)
{
    double m = a;
    if (b > m) m = b;
    if (c > m) m = c;
    return m;
}
// true_range (volatility.py:223-253) of bar i from its high and low and the close before it; first: bar 0
__device__ __forceinline__ double rc_tr(double hi, double lo, double cp, bool first)
{
    if (first) return (hi != hi || lo != lo) ? NAN : hi - lo;
    if (hi != hi || lo != lo || cp != cp) return NAN;
    return rc_max3(hi - lo, fabs(hi - cp), fabs(lo - cp));
}
__device__ __forceinline__ double rc_tr_at(const double *__restrict__ h, const double *__restrict__ l, const double *__restrict__ c,
                                           int64_t i)
{
    return rc_tr(h[i], l[i], i > 0 ? c[i - 1] : 0.0, i == 0);
}
// atr's normalisation (volatility.py:431-435)
__device__ __forceinline__ double rc_normalize(double v, double hi, double lo)
{
    const double mid = (hi + lo) / 2.0;
    return (v == v && mid == mid && mid > 0.0) ? v / mid : v;
}
// adx_core's inputs of bar i >= 1 (trend.py:30-52): no NaN checks
__device__ __forceinline__ void rc_dm(double hi, double lo, double hp, double lp, double cp, double (&x)[3])
{
    x[0] = rc_max3(hi - lo, fabs(hi - cp), fabs(lo - cp));
    const double hd = hi - hp, ld = lp - lo;
    x[1] = (hd > ld && hd > 0.0) ? hd : 0.0;
    x[2] = (ld > hd && ld > 0.0) ? ld : 0.0;
}

// ---- the recurrences.  A spec gives: K, the coefficient a, the seed index; In / load(): the thread's elements; x(): the inputs of
// element j (index i > seed); lin(): the b of the linear form for an input; step(): the reference's expression; emit(): the output;
// before(): the output in front of the seed; and the seed: term() of the elements seed_lo .. seed_hi, added in index order by acc()
// from zero, closed by fin().
struct RcEwma {
    static constexpr int K = 2;
    const double *y;
    double a;                        // 1.0 - alpha
    int64_t seed;                    // 0
    struct In { double y[RC_ITEMS]; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const { rc_load8(y, i0, n, whole, in.y); }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const { x[0] = in.y[j]; x[1] = 1.0; }
    __device__ __forceinline__ double lin(double x) const { return x; }
    __device__ __forceinline__ double step(double s, double x) const { return x + a * s; }
    __device__ __forceinline__ double emit(const double (&s)[K], const In &, int) const { return s[0] / s[1]; }
    __device__ __forceinline__ double before() const { return NAN; }
    __device__ __forceinline__ int64_t seed_lo() const { return 0; }
    __device__ __forceinline__ int64_t seed_hi() const { return 0; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { t[0] = y[i]; t[1] = 1.0; }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &, const double (&t)[K]) const { s[0] = t[0]; s[1] = t[1]; }
    __device__ __forceinline__ void fin(double (&)[K], int64_t) const {}
};

struct RcRsi {
    static constexpr int K = 2;
    const double *c;
    double a, wm1, w;                // (w - 1) / w, w - 1, w
    int64_t seed;                    // window
    struct In { double c[RC_ITEMS]; double cp; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        rc_load8(c, i0, n, whole, in.c);
        in.cp = rc_prev(c, i0, n);
    }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const
    {
        const int p = j ? j - 1 : 0;
        const double d = in.c[j] - (j ? in.c[p] : in.cp);
        x[0] = d > 0.0 ? d : 0.0;                                    // a NaN difference: no gain and no loss
        x[1] = d < 0.0 ? -d : 0.0;
    }
    __device__ __forceinline__ double lin(double x) const { return x / w; }
    __device__ __forceinline__ double step(double s, double x) const { return (wm1 * s + x) / w; }
    __device__ __forceinline__ double emit(const double (&s)[K], const In &, int) const
    {
        return s[1] > 0.0 ? 100.0 - 100.0 / (1.0 + s[0] / s[1]) : NAN;
    }
    __device__ __forceinline__ double before() const { return NAN; }
    __device__ __forceinline__ int64_t seed_lo() const { return 1; }
    __device__ __forceinline__ int64_t seed_hi() const { return seed; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { t[0] = c[i] - c[i - 1]; t[1] = 0.0; }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &, const double (&t)[K]) const
    {
        if (t[0] > 0.0) s[0] += t[0];
        else s[1] += -t[0];                                          // a NaN difference poisons the losses for good
    }
    __device__ __forceinline__ void fin(double (&s)[K], int64_t) const { s[0] = s[0] / w; s[1] = s[1] / w; }
};

struct RcAtr {
    static constexpr int K = 1;
    const double *h, *l, *c;
    double a, wm1, w;
    int64_t seed;                    // window - 1
    int normalize;
    struct In { double h[RC_ITEMS], l[RC_ITEMS], c[RC_ITEMS]; double cp; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        rc_load8(h, i0, n, whole, in.h);
        rc_load8(l, i0, n, whole, in.l);
        rc_load8(c, i0, n, whole, in.c);
        in.cp = rc_prev(c, i0, n);
    }
    __device__ __forceinline__ void x(const In &in, int j, int64_t i, double (&x)[K]) const
    {
        const int p = j ? j - 1 : 0;
        x[0] = rc_tr(in.h[j], in.l[j], j ? in.c[p] : in.cp, i == 0);
    }
    __device__ __forceinline__ double lin(double x) const { return x / w; }
    // NaN where the true range or the value before is NaN: the arithmetic gives that by itself
    __device__ __forceinline__ double step(double s, double x) const { return (wm1 * s + x) / w; }
    __device__ __forceinline__ double emit(const double (&s)[K], const In &in, int j) const
    {
        return normalize ? rc_normalize(s[0], in.h[j], in.l[j]) : s[0];
    }
    __device__ __forceinline__ double before() const { return NAN; }
    __device__ __forceinline__ int64_t seed_lo() const { return 0; }
    __device__ __forceinline__ int64_t seed_hi() const { return seed; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { t[0] = rc_tr_at(h, l, c, i); }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &cnt, const double (&t)[K]) const
    {
        if (t[0] == t[0]) { s[0] += t[0]; ++cnt; }
    }
    __device__ __forceinline__ void fin(double (&s)[K], int64_t cnt) const { s[0] = cnt > 0 ? s[0] / (double)cnt : NAN; }
};

struct RcAdxSums {                   // out: dx
    static constexpr int K = 3;
    const double *h, *l, *c;
    double a, L;                     // 1 - 1 / L, L
    int64_t seed;                    // length
    struct In { double h[RC_ITEMS], l[RC_ITEMS], c[RC_ITEMS]; double hp, lp, cp; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        rc_load8(h, i0, n, whole, in.h);
        rc_load8(l, i0, n, whole, in.l);
        rc_load8(c, i0, n, whole, in.c);
        in.hp = rc_prev(h, i0, n);
        in.lp = rc_prev(l, i0, n);
        in.cp = rc_prev(c, i0, n);
    }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const
    {
        const int p = j ? j - 1 : 0;
        rc_dm(in.h[j], in.l[j], j ? in.h[p] : in.hp, j ? in.l[p] : in.lp, j ? in.c[p] : in.cp, x);
    }
    __device__ __forceinline__ double lin(double x) const { return x; }
    __device__ __forceinline__ double step(double s, double x) const { return s - s / L + x; }
    __device__ __forceinline__ double emit(const double (&s)[K], const In &, int) const
    {
        double pdi = 0.0, mdi = 0.0;
        if (s[0] > 0.0) { pdi = 100.0 * (s[1] / s[0]); mdi = 100.0 * (s[2] / s[0]); }
        return (pdi + mdi) > 0.0 ? 100.0 * (fabs(pdi - mdi) / (pdi + mdi)) : 0.0;
    }
    __device__ __forceinline__ double before() const { return 0.0; }
    __device__ __forceinline__ int64_t seed_lo() const { return 1; }
    __device__ __forceinline__ int64_t seed_hi() const { return seed; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { rc_dm(h[i], l[i], h[i - 1], l[i - 1], c[i - 1], t); }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &, const double (&t)[K]) const
    {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += t[k];
    }
    __device__ __forceinline__ void fin(double (&)[K], int64_t) const {}
};

struct RcAdxLast {
    static constexpr int K = 1;
    const double *dx;
    double a, Lm1, L;                // (L - 1) / L, L - 1, L
    int64_t seed;                    // 2 * length - 1
    struct In { double dx[RC_ITEMS]; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const { rc_load8(dx, i0, n, whole, in.dx); }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const { x[0] = in.dx[j]; }
    __device__ __forceinline__ double lin(double x) const { return x / L; }
    __device__ __forceinline__ double step(double s, double x) const { return (s * Lm1 + x) / L; }
    __device__ __forceinline__ double emit(const double (&s)[K], const In &, int) const { return s[0]; }
    __device__ __forceinline__ double before() const { return 0.0; }
    __device__ __forceinline__ int64_t seed_lo() const { return seed - ((int64_t)L - 1); }
    __device__ __forceinline__ int64_t seed_hi() const { return seed; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { t[0] = dx[i]; }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &, const double (&t)[K]) const { s[0] += t[0]; }
    __device__ __forceinline__ void fin(double (&s)[K], int64_t) const { s[0] = s[0] / L; }
};

__global__ __launch_bounds__(256) void k_true_range(const double *__restrict__ h, const double *__restrict__ l, const double *__restrict__ c,
                                                    int64_t n, double *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = rc_tr_at(h, l, c, i);
}

// atr, SMA mode (volatility.py:407-428): per output t >= window - 1 the mean of the non-NaN true ranges of bars t - window + 1 .. t,
// added left to right from 0.0; NaN when there is none, and at t == 2 when high, low and close of bar 2 are all NaN
struct AtrSmaArgs {
    const double *h, *l, *c;
    double *out;
    int64_t n, window;
    int normalize;
    int slab;
};

__global__ __launch_bounds__(RC_THREADS) void k_atr_sma(AtrSmaArgs a)
{
    extern __shared__ double atr_lds[];
    const int64_t t0 = a.window - 1 + (int64_t)blockIdx.x * ATR_TILE;
    const int64_t t1 = t0 + ATR_TILE < a.n ? t0 + ATR_TILE : a.n;
    const int64_t lo = t0 - (a.window - 1), span = t1 - lo;          // the tile reads the true ranges of bars lo .. t1 - 1
    const double *h = a.h, *l = a.l, *c = a.c;
    auto load = [h, l, c, lo](int64_t i) { return rc_tr_at(h, l, c, lo + i); };
    double s[ATR_OPL];
    int cnt[ATR_OPL];
#pragma unroll
    for (int r = 0; r < ATR_OPL; ++r) { s[r] = 0.0; cnt[r] = 0; }
    fmk_window_walk<RC_THREADS, ATR_OPL>(atr_lds, span, a.window, a.slab, true, load, [&](int r, double v) {
        const bool ok = v == v;                                      // NaN skipped by select
        const double sum = s[r] + v;
        s[r] = ok ? sum : s[r];
        cnt[r] += ok ? 1 : 0;
    });
#pragma unroll
    for (int r = 0; r < ATR_OPL; ++r) {
        const int64_t t = t0 + r * RC_THREADS + threadIdx.x;
        if (t >= t1) continue;
        double o = cnt[r] > 0 ? s[r] / (double)cnt[r] : NAN;
        const double hi = h[t], lw = l[t];
        if (t == 2 && hi != hi && lw != lw && c[t] != c[t]) o = NAN;
        a.out[t] = a.normalize ? rc_normalize(o, hi, lw) : o;
    }
}

}  // namespace

extern "C" int fmk_ewma_dev(fmk_ctx *ctx, const double *d_y, int64_t n, double span, double *d_out)
{
    FMK_TRY(fmk_rule_ewma(ctx, span));
    FMK_TRY(fmk_series_check(ctx, "ewma", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    RcEwma sp;
    sp.y = d_y;
    sp.a = 1.0 - 2.0 / (span + 1.0);
    sp.seed = 0;
    return rc_scan(ctx, sp, n, d_out, NAN);
}

extern "C" int fmk_rsi_wilder_dev(fmk_ctx *ctx, const double *d_close, int64_t n, int64_t window, double *d_out)
{
    FMK_TRY(fmk_rule_rsi_wilder(ctx, window));
    FMK_TRY(fmk_series_check(ctx, "rsi_wilder", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    RcRsi sp;
    sp.c = d_close;
    sp.w = (double)window;
    sp.wm1 = (double)(window - 1);
    sp.a = sp.wm1 / sp.w;
    sp.seed = window;
    return rc_scan(ctx, sp, n, d_out, NAN);
}

extern "C" int fmk_true_range_dev(fmk_ctx *ctx, const double *d_high, const double *d_low, const double *d_close, int64_t n, double *d_out)
{
    FMK_TRY(fmk_series_check(ctx, "true_range", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    k_true_range<<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>(d_high, d_low, d_close, n, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_atr_dev(fmk_ctx *ctx, const double *d_high, const double *d_low, const double *d_close, int64_t n, int64_t window,
                           int ema_based, int normalize, double *d_out)
{
    FMK_TRY(fmk_rule_atr(ctx, window));
    FMK_TRY(fmk_series_check(ctx, "atr", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    if (window == 0 || window > n) return rc_fill(ctx, d_out, n, NAN);   // window 0: every window of the reference is empty
    if (ema_based) {
        RcAtr sp;
        sp.h = d_high; sp.l = d_low; sp.c = d_close;
        sp.w = (double)window;
        sp.wm1 = (double)(window - 1);
        sp.a = sp.wm1 / sp.w;
        sp.seed = window - 1;
        sp.normalize = normalize != 0;
        return rc_scan(ctx, sp, n, d_out, NAN);
    }
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    AtrSmaArgs a;
    a.h = d_high; a.l = d_low; a.c = d_close; a.out = d_out; a.n = n; a.window = window; a.normalize = normalize != 0;
    a.slab = fmk_slab(window, ATR_TILE);
    const int64_t tiles = fmk_ceil_div(n - (window - 1), ATR_TILE);
    k_atr_sma<<<(unsigned)tiles, RC_THREADS, (size_t)a.slab * sizeof(double), ctx->stream>>>(a);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_adx_dev(fmk_ctx *ctx, const double *d_high, const double *d_low, const double *d_close, int64_t n, int64_t length,
                           double *d_out)
{
    FMK_TRY(fmk_rule_adx(ctx, length));
    FMK_TRY(fmk_series_check(ctx, "adx_core", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    if (length > n / 2) return rc_fill(ctx, d_out, n, 0.0);          // n < 2 * length (without the product): no first ADX, zero everywhere
    void *work;
    FMK_TRY(fmk_alloc(ctx, (size_t)n * sizeof(double), &work));
    double *dx = (double *)work;
    RcAdxSums s1;
    s1.h = d_high; s1.l = d_low; s1.c = d_close;
    s1.L = (double)length;
    s1.a = 1.0 - 1.0 / s1.L;
    s1.seed = length;
    int rc = rc_scan(ctx, s1, n, dx, 0.0);
    if (rc == FMK_OK) {
        RcAdxLast s2;
        s2.dx = dx;
        s2.L = (double)length;
        s2.Lm1 = (double)(length - 1);
        s2.a = s2.Lm1 / s2.L;
        s2.seed = 2 * length - 1;
        rc = rc_scan(ctx, s2, n, d_out, 0.0);
    }
    const int frc = fmk_free(ctx, work);                             // stream-ordered: the next user comes after the kernels
    return rc != FMK_OK ? rc : frc;
}
