// fmk_runsum.hip -- the bar-level indicators of the reference that carry a running sum, on resident float64 series:
// bollinger_percent_b and parkinson_range (feature/core/volatility.py), vwap_distance (feature/core/reversion.py),
// comp_flow_acceleration and vpin (feature/core/volume.py).  DESIGN.md section 7f.
//
// A running sum is the recurrence of fmk_recur_core.h with a = 1: a tile's a^len is exactly 1, and the state that enters a thread's
// 8 elements is an ordinary sum in another order.  Every step and every output is the reference's own expression.
//   bollinger_percent_b  K = 2  sum += c[i] - c[i-w], sumsq += c[i]^2 - c[i-w]^2, seeded at w - 1 by the in-order sums
//   vwap_distance        K = 2  wsum += c[i] v[i] - c[i-w] v[i-w], vsum += v[i] - v[i-w], seeded at w - 1; where vsum > 0 is false the
//                               output is the one before it: a launch of its own (k_rs_hold) after the scan
//   comp_flow_accel.     K = 2  the prefix sum S[i+1] and the count of bars that are not zero (4 bytes each) as two scratch series,
//                               then an elementwise kernel on their differences
//   vpin                 K = 7  the prefix sums of buy, sell and |buy - sell|, the counts of their terms that are not zero and the
//                               NaN count (float64 channels: counts are exact there) as five scratch series, the counts two to a
//                               series, then an elementwise kernel that writes float32
//   parkinson_range             elementwise
// Zero-volume bars: the reference differences sequential prefix sums, and adding 0.0 changes no bit of one, so its sum over a window
// part whose terms are all 0.0 is exactly 0.0 and its outputs there are log(1e-12 / (past + 1e-12)), log((recent + 1e-12) / 1e-12)
// and vpin's NaN.  Two prefix sums of this scan may differ in their last bits across a thread's edge although nothing but zeros
// lies between them, so the elementwise kernels take 0.0 where the window's count of non-zero terms is 0 (rs_window).
// No workgroup waits for another: every cross-tile dependence is a launch boundary.  log is the host's (fmk_log.h).  Outside the
// contract: infinite inputs to the four scans (0 * inf in the composed maps is not inf).
#include <math.h>

#include "fmk_common.h"
#include "fmk_log.h"
#include "fmk_recur_core.h"

namespace {

// src[i0 - lag .. i0 - lag + 8): 0.0 for what lies in front of element 0 or beyond the series
__device__ __forceinline__ void rs_load8_lag(const double *__restrict__ src, int64_t i0, int64_t lag, int64_t n, bool whole,
                                             double (&v)[RC_ITEMS])
{
    const int64_t b = i0 - lag;
    if (whole && b >= 0) {                                           // whole: i0 + 8 <= n
        const rc_d2 *q = (const rc_d2 *)(src + b);
#pragma unroll
        for (int k = 0; k < RC_ITEMS / 2; ++k) { const rc_d2 t = q[k]; v[2 * k] = t.x; v[2 * k + 1] = t.y; }
    } else {
#pragma unroll
        for (int k = 0; k < RC_ITEMS; ++k) v[k] = (b + k >= 0 && b + k < n) ? src[b + k] : 0.0;
    }
}

// bollinger_percent_b (volatility.py:289-338)
struct RsBoll {
    static constexpr int K = 2;
    const double *c;
    double a, w, wm1, num_std;       // 1.0, window, window - 1
    int64_t seed, lag;               // window - 1, window
    struct In { double c[RC_ITEMS], cl[RC_ITEMS]; int64_t i0; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        rc_load8(c, i0, n, whole, in.c);
        rs_load8_lag(c, i0, lag, n, whole, in.cl);
        in.i0 = i0;
    }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const
    {
        x[0] = in.c[j] - in.cl[j];
        x[1] = in.c[j] * in.c[j] - in.cl[j] * in.cl[j];
    }
    __device__ __forceinline__ double lin(double x) const { return x; }
    __device__ __forceinline__ double step(double s, double x) const { return s + x; }
    __device__ __forceinline__ double emit(const double (&s)[K], const In &in, int j) const
    {
        const double mean = s[0] / w;
        // the reference writes window * mean * mean for the first window and window * mean ** 2 after it
        const double t = in.i0 + j == seed ? w * mean * mean : w * (mean * mean);
        const double var = (s[1] - t) / wm1;
        const double sd = sqrt(0.0 > var ? 0.0 : var);               // Python's max(var, 0.0): a NaN stays
        const double lower = mean - num_std * sd, upper = mean + num_std * sd;
        return upper > lower ? (in.c[j] - lower) / (upper - lower) : NAN;
    }
    __device__ __forceinline__ double before() const { return NAN; }
    __device__ __forceinline__ int64_t seed_lo() const { return 0; }
    __device__ __forceinline__ int64_t seed_hi() const { return seed; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { t[0] = c[i]; t[1] = c[i] * c[i]; }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &, const double (&t)[K]) const { s[0] += t[0]; s[1] += t[1]; }
    __device__ __forceinline__ void fin(double (&)[K], int64_t) const {}
};

// what the hold launch needs to know about a tile of vwap_distance: the last index with vsum > 0 (-1: none) and whether an
// element from the seed on has none
struct RsTile {
    int64_t last;
    int64_t bad;
};

// vwap_distance (reversion.py:9-56).  An element where vsum > 0 is false gets NaN here and its bit in the thread's mask (low byte:
// elements with a value, high byte: elements to fill); k_rs_hold fills it.
struct RsVwap {
    static constexpr int K = 2;
    const double *c, *v;
    double a;                        // 1.0
    int64_t seed, lag;               // n_periods - 1, n_periods
    int is_log;
    RsTile *tile;
    uint16_t *mask;                  // one per thread
    struct In { double c[RC_ITEMS], v[RC_ITEMS], cl[RC_ITEMS], vl[RC_ITEMS]; int64_t i0; mutable unsigned ok; };
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        rc_load8(c, i0, n, whole, in.c);
        rc_load8(v, i0, n, whole, in.v);
        rs_load8_lag(c, i0, lag, n, whole, in.cl);
        rs_load8_lag(v, i0, lag, n, whole, in.vl);
        in.i0 = i0;
        in.ok = 0;
    }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const
    {
        x[0] = in.c[j] * in.v[j] - in.cl[j] * in.vl[j];
        x[1] = in.v[j] - in.vl[j];
    }
    __device__ __forceinline__ double lin(double x) const { return x; }
    __device__ __forceinline__ double step(double s, double x) const { return s + x; }
    __device__ __forceinline__ double emit(const double (&s)[K], const In &in, int j) const
    {
        if (!(s[1] > 0.0)) return NAN;
        in.ok |= 1u << j;
        const double q = in.c[j] / (s[0] / s[1]);
        return (is_log && in.i0 + j != seed) ? fmk_log_host(q) : q - 1.0;   // the first window is the simple form in either mode
    }
    __device__ __forceinline__ double before() const { return NAN; }
    __device__ __forceinline__ int64_t seed_lo() const { return 0; }
    __device__ __forceinline__ int64_t seed_hi() const { return seed; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { t[0] = c[i] * v[i]; t[1] = v[i]; }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &, const double (&t)[K]) const { s[0] += t[0]; s[1] += t[1]; }
    __device__ __forceinline__ void fin(double (&)[K], int64_t) const {}
    __device__ __forceinline__ void tile_end(const In &in, int64_t n) const
    {
        __shared__ int s_last, s_bad;
        if (threadIdx.x == 0) { s_last = -1; s_bad = 0; }
        __syncthreads();
        unsigned live = 0;
#pragma unroll
        for (int j = 0; j < RC_ITEMS; ++j)
            if (in.i0 + j >= seed && in.i0 + j < n) live |= 1u << j;
        const unsigned ok = in.ok & live, bad = live & ~in.ok;
        mask[(int64_t)blockIdx.x * RC_THREADS + threadIdx.x] = (uint16_t)(ok | bad << 8);
        if (ok) atomicMax(&s_last, (int)threadIdx.x * RC_ITEMS + 31 - __clz((int)ok));
        if (bad) atomicOr(&s_bad, 1);
        __syncthreads();
        if (threadIdx.x == 0) {
            RsTile t;
            t.last = s_last >= 0 ? (int64_t)blockIdx.x * RC_TILE + s_last : -1;
            t.bad = s_bad;
            tile[blockIdx.x] = t;
        }
    }
};

// The hold of vwap_distance, in place: an element without a value takes the value at the last index in front of it that has one,
// NaN when there is none.  Elements with a value are never written, so the fill reads what the scan left.  A tile with nothing
// to fill returns at once; the others find the index carried into them by looking back over the tile records, 256 at a time.
__global__ __launch_bounds__(RC_THREADS) void k_rs_hold(double *out, const RsTile *__restrict__ tile, const uint16_t *__restrict__ mask)
{
    __shared__ int last[RC_THREADS];
    __shared__ long long s_carry;
    const int64_t t = blockIdx.x;
    if (!tile[t].bad) return;                                        // uniform over the workgroup
    const int tid = (int)threadIdx.x;
    const unsigned m = mask[t * RC_THREADS + tid], ok = m & 0xFFu, bad = m >> 8;
    last[tid] = ok ? tid * RC_ITEMS + 31 - __clz((int)ok) : -1;
    long long carry = -1;
    for (int64_t base = t - 1; base >= 0 && carry < 0; base -= RC_THREADS) {      // carry is uniform: so is the loop
        if (tid == 0) s_carry = -1;
        __syncthreads();
        const int64_t tt = base - tid;
        const long long l = tt >= 0 ? (long long)tile[tt].last : -1;
        if (l >= 0) atomicMax(&s_carry, l);
        __syncthreads();
        carry = s_carry;
        __syncthreads();
    }
    __syncthreads();
    if (!bad) return;
    int64_t prev = carry;
    for (int k = tid - 1; k >= 0; --k)
        if (last[k] >= 0) { prev = t * RC_TILE + last[k]; break; }
    const int64_t i0 = t * RC_TILE + (int64_t)tid * RC_ITEMS;
#pragma unroll
    for (int j = 0; j < RC_ITEMS; ++j) {
        if (ok >> j & 1u) prev = i0 + j;
        else if (bad >> j & 1u) out[i0 + j] = prev >= 0 ? out[prev] : NAN;
    }
}

// Two exact counts below 2^31 in one 8-byte element of a scratch series: a count is a float64 channel of the scan (sums of 1.0 are
// exact in any order); its prefix is stored as an integer beside another one, so that two counts cost one series.
__device__ __forceinline__ double rs_pack(double hi, double lo)
{
    return __longlong_as_double((long long)hi << 32 | (long long)lo);
}
__device__ __forceinline__ int64_t rs_hi(double p) { return (int64_t)(__double_as_longlong(p) >> 32); }
__device__ __forceinline__ int64_t rs_lo(double p) { return (int64_t)(__double_as_longlong(p) & 0xFFFFFFFFll); }

typedef int rs_i4 __attribute__((ext_vector_type(4), aligned(8)));             // as rc_d2: the counts lie behind n float64

// the prefix sum of comp_flow_acceleration (volume.py:596-600): out[i] = S[i + 1], and beside it cnt[i], the number of bars up to
// i that are not zero (below 2^31: 4 bytes each, written by tile_end).  Adding 0.0 leaves the reference's S as it is in every bit,
// so a window part of zero bars has a sum of exactly 0.0 there; here S[i + 1] and S[i] may come from different orders of addition,
// and the count says what the difference is.
struct RsPrefix {
    static constexpr int K = 2;
    const double *v;
    int32_t *cnt;
    double a;                        // 1.0
    int64_t seed;                    // 0
    struct In { double v[RC_ITEMS]; int64_t i0; int32_t c[RC_ITEMS]; };          // c: the counts, from emit to tile_end
    __device__ __forceinline__ static void bar(double v, double (&x)[K])
    {
        x[0] = v;
        x[1] = v != 0.0 ? 1.0 : 0.0;                                 // (a NaN counts; what decides behind one is rs_window)
    }
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        rc_load8(v, i0, n, whole, in.v);
        in.i0 = i0;
    }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const { bar(in.v[j], x); }
    __device__ __forceinline__ double lin(double x) const { return x; }
    __device__ __forceinline__ double step(double s, double x) const { return s + x; }
    __device__ __forceinline__ double emit(const double (&s)[K], In &in, int j) const
    {
        in.c[j] = (int32_t)s[1];
        return s[0];
    }
    __device__ __forceinline__ double before() const { return NAN; }
    __device__ __forceinline__ int64_t seed_lo() const { return 0; }
    __device__ __forceinline__ int64_t seed_hi() const { return 0; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { bar(v[i], t); }
    __device__ __forceinline__ void acc(double (&s)[K], int64_t &, const double (&t)[K]) const { s[0] += t[0]; s[1] += t[1]; }   // S[0] = 0.0
    __device__ __forceinline__ void fin(double (&)[K], int64_t) const {}
    __device__ __forceinline__ void tile_end(const In &in, int64_t n) const
    {
        if (rc_whole(blockIdx.x, n)) {
            rs_i4 *q = (rs_i4 *)(cnt + in.i0);
#pragma unroll
            for (int k = 0; k < RC_ITEMS / 4; ++k) {
                rs_i4 t;
                t.x = in.c[4 * k];
                t.y = in.c[4 * k + 1];
                t.z = in.c[4 * k + 2];
                t.w = in.c[4 * k + 3];
                q[k] = t;
            }
        } else {
#pragma unroll
            for (int k = 0; k < RC_ITEMS; ++k)
                if (in.i0 + k < n) cnt[in.i0 + k] = in.c[k];
        }
    }
};

// the prefix sums of vpin (volume.py:616-632): series 0 to 2 of the output are the sums of buy, sell and |buy - sell| at i + 1,
// series 3 the counts of buy and of sell terms that are not zero, series 4 those of |buy - sell| terms that are not zero and of
// bars with a NaN (rs_pack).  The counts are what the window differences are decided by: a sum over terms that are all 0.0 is
// exactly 0.0 in the reference, and a bar with a NaN in the window gives NaN.
struct RsVpin {
    static constexpr int K = 7;
    static constexpr int NOUT = 5;
    const double *b, *s;
    double a;                        // 1.0
    int64_t seed;                    // 0
    struct In { double b[RC_ITEMS], s[RC_ITEMS]; };
    __device__ __forceinline__ static void bar(double vb, double vs, double (&x)[K])
    {
        const bool nan = vb != vb || vs != vs;                       // such a bar adds nothing to the sums and 1 to the count
        x[0] = nan ? 0.0 : vb;
        x[1] = nan ? 0.0 : vs;
        x[2] = nan ? 0.0 : fabs(vb - vs);
        x[3] = x[0] != 0.0 ? 1.0 : 0.0;
        x[4] = x[1] != 0.0 ? 1.0 : 0.0;
        x[5] = x[2] != 0.0 ? 1.0 : 0.0;
        x[6] = nan ? 1.0 : 0.0;
    }
    __device__ __forceinline__ void load(int64_t i0, int64_t n, bool whole, In &in) const
    {
        rc_load8(b, i0, n, whole, in.b);
        rc_load8(s, i0, n, whole, in.s);
    }
    __device__ __forceinline__ void x(const In &in, int j, int64_t, double (&x)[K]) const { bar(in.b[j], in.s[j], x); }
    __device__ __forceinline__ double lin(double x) const { return x; }
    __device__ __forceinline__ double step(double st, double x) const { return st + x; }
    __device__ __forceinline__ void emit(const double (&st)[K], const In &, int, double (&r)[NOUT]) const
    {
        r[0] = st[0];
        r[1] = st[1];
        r[2] = st[2];
        r[3] = rs_pack(st[3], st[4]);
        r[4] = rs_pack(st[5], st[6]);
    }
    __device__ __forceinline__ double before() const { return NAN; }
    __device__ __forceinline__ int64_t seed_lo() const { return 0; }
    __device__ __forceinline__ int64_t seed_hi() const { return 0; }
    __device__ __forceinline__ void term(int64_t i, double (&t)[K]) const { bar(b[i], s[i], t); }
    __device__ __forceinline__ void acc(double (&st)[K], int64_t &, const double (&t)[K]) const
    {
#pragma unroll
        for (int k = 0; k < K; ++k) st[k] += t[k];                   // from 0.0, as the reference's cum[1] = cum[0] + x
    }
    __device__ __forceinline__ void fin(double (&)[K], int64_t) const {}
};

// S[k] of a prefix sum stored as q[i] = S[i + 1]
__device__ __forceinline__ double rs_prefix(const double *__restrict__ q, int64_t k) { return k > 0 ? q[k - 1] : 0.0; }

// a - b of a prefix sum where `terms` of the elements between them are not zero: exactly 0.0 where none is, as long as the prefix
// sum is a number.  Behind a NaN or an infinity in the series every S of the reference is NaN or infinite for good, and so is every
// difference of two of them, over zero bars as well (NaN - NaN): there the plain difference is the reference's.
__device__ __forceinline__ double rs_window(double a, double b, int64_t terms)
{
    return terms != 0 || !__builtin_isfinite(a) ? a - b : 0.0;
}

// the count that goes with S[k]
__device__ __forceinline__ int64_t rs_count(const int32_t *__restrict__ c, int64_t k) { return k > 0 ? c[k - 1] : 0; }

// comp_flow_acceleration (volume.py:602-605); 0 <= recent < window <= n; q, qc: the prefix sum and the count of RsPrefix
__global__ __launch_bounds__(256) void k_flow_acc(const double *__restrict__ q, const int32_t *__restrict__ qc, int64_t n, int64_t window,
                                                  int64_t recent, double *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (i < window - 1) { out[i] = NAN; continue; }
        const double mid = rs_prefix(q, i + 1 - recent);
        const int64_t cmid = rs_count(qc, i + 1 - recent);
        const double recent_sum = rs_window(q[i], mid, qc[i] - cmid);
        const double past_sum = rs_window(mid, rs_prefix(q, i + 1 - window), cmid - rs_count(qc, i + 1 - window));
        out[i] = fmk_log_host((recent_sum + 1e-12) / (past_sum + 1e-12));
    }
}

// vpin (volume.py:634-640); 1 <= window <= n; q: the five series of RsVpin, n elements each
__global__ __launch_bounds__(256) void k_vpin(const double *__restrict__ q, int64_t n, int64_t window, float *__restrict__ out)
{
    const double *qb = q, *qs = q + n, *qa = q + 2 * n, *qbs = q + 3 * n, *qan = q + 4 * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float o = NAN;
        const int64_t k = i + 1 - window;
        if (k >= 0) {
            const double an1 = qan[i], an0 = rs_prefix(qan, k);
            if (rs_lo(an1) - rs_lo(an0) == 0) {
                const double bs1 = qbs[i], bs0 = rs_prefix(qbs, k);
                const double tot = rs_window(qb[i], rs_prefix(qb, k), rs_hi(bs1) - rs_hi(bs0)) +
                                   rs_window(qs[i], rs_prefix(qs, k), rs_lo(bs1) - rs_lo(bs0));
                if (tot > 1e-9) o = (float)(rs_window(qa[i], rs_prefix(qa, k), rs_hi(an1) - rs_hi(an0)) / tot);
            }
        }
        out[i] = o;
    }
}

__global__ __launch_bounds__(256) void k_rs_fill_f32(float *out, int64_t n, float v)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = v;
}

// parkinson_range (volatility.py:341-349)
__global__ __launch_bounds__(256) void k_parkinson(const double *__restrict__ h, const double *__restrict__ l, int64_t n,
                                                   double *__restrict__ out)
{
    const double ln2x4 = 0x1.62e42fefa39efp-1 * 4.0;                 // the host's log(2.0), times 4
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double lg = fmk_log_host(h[i] / l[i]);
        out[i] = (lg * lg) / ln2x4;
    }
}

}  // namespace

extern "C" int fmk_bollinger_percent_b_dev(fmk_ctx *ctx, const double *d_close, int64_t n, int64_t window, double num_std, double *d_out)
{
    FMK_TRY(fmk_rule_bollinger(ctx, window));
    FMK_TRY(fmk_series_check(ctx, "bollinger_percent_b", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    RsBoll sp;
    sp.c = d_close;
    sp.a = 1.0;
    sp.w = (double)window;
    sp.wm1 = (double)(window - 1);
    sp.num_std = num_std;
    sp.seed = window - 1;
    sp.lag = window;
    return rc_scan(ctx, sp, n, d_out, NAN);                          // n < window: NaN everywhere
}

extern "C" int fmk_vwap_distance_dev(fmk_ctx *ctx, const double *d_close, const double *d_volume, int64_t n, int64_t n_periods,
                                     int is_log, double *d_out)
{
    FMK_TRY(fmk_rule_vwap_distance(ctx, n_periods));
    FMK_TRY(fmk_series_check(ctx, "vwap_distance", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    if (n_periods > n) return rc_fill(ctx, d_out, n, NAN);
    const int64_t tiles = fmk_ceil_div(n, RC_TILE);
    void *work;
    FMK_TRY(fmk_alloc(ctx, (size_t)tiles * (sizeof(RsTile) + RC_THREADS * sizeof(uint16_t)), &work));
    RsVwap sp;
    sp.c = d_close;
    sp.v = d_volume;
    sp.a = 1.0;
    sp.seed = n_periods - 1;
    sp.lag = n_periods;
    sp.is_log = is_log != 0;
    sp.tile = (RsTile *)work;
    sp.mask = (uint16_t *)(sp.tile + tiles);
    int rc = rc_scan(ctx, sp, n, d_out, NAN);
    if (rc == FMK_OK) {
        k_rs_hold<<<(unsigned)tiles, RC_THREADS, 0, ctx->stream>>>(d_out, sp.tile, sp.mask);
        if (hipGetLastError() != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "vwap_distance: the hold launch failed");
    }
    const int frc = fmk_free(ctx, work);                             // stream-ordered: the next user comes after the kernels
    return rc != FMK_OK ? rc : frc;
}

extern "C" int fmk_flow_acceleration_dev(fmk_ctx *ctx, const double *d_volumes, int64_t n, int64_t window, int64_t recent_periods,
                                         double *d_out)
{
    FMK_TRY(fmk_rule_flow_acceleration(ctx, recent_periods));
    FMK_TRY(fmk_series_check(ctx, "comp_flow_acceleration", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    if (n < window || recent_periods >= window) return rc_fill(ctx, d_out, n, NAN);
    void *work;
    FMK_TRY(fmk_alloc(ctx, (size_t)n * (sizeof(double) + sizeof(int32_t)), &work));
    RsPrefix sp;
    sp.v = d_volumes;
    sp.cnt = (int32_t *)((double *)work + n);
    sp.a = 1.0;
    sp.seed = 0;
    int rc = rc_scan(ctx, sp, n, (double *)work, NAN);
    if (rc == FMK_OK) {
        k_flow_acc<<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>((const double *)work, sp.cnt, n, window, recent_periods, d_out);
        if (hipGetLastError() != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "comp_flow_acceleration: the launch failed");
    }
    const int frc = fmk_free(ctx, work);
    return rc != FMK_OK ? rc : frc;
}

extern "C" int fmk_vpin_dev(fmk_ctx *ctx, const double *d_volume_buy, const double *d_volume_sell, int64_t n, int64_t window,
                            float *d_out)
{
    FMK_TRY(fmk_rule_vpin(ctx, window));
    FMK_TRY(fmk_series_check(ctx, "vpin", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    if (window == 0 || window > n) {                                 // window 0: the reference's total is 0.0 everywhere
        k_rs_fill_f32<<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>(d_out, n, NAN);
        FMK_LAUNCH_CHECK(ctx);
        return FMK_OK;
    }
    void *work;
    FMK_TRY(fmk_alloc(ctx, (size_t)n * RsVpin::NOUT * sizeof(double), &work));
    RsVpin sp;
    sp.b = d_volume_buy;
    sp.s = d_volume_sell;
    sp.a = 1.0;
    sp.seed = 0;
    int rc = rc_scan(ctx, sp, n, (double *)work, NAN);
    if (rc == FMK_OK) {
        k_vpin<<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>((const double *)work, n, window, d_out);
        if (hipGetLastError() != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "vpin: the launch failed");
    }
    const int frc = fmk_free(ctx, work);
    return rc != FMK_OK ? rc : frc;
}

extern "C" int fmk_parkinson_range_dev(fmk_ctx *ctx, const double *d_high, const double *d_low, int64_t n, double *d_out)
{
    FMK_TRY(fmk_series_check(ctx, "parkinson_range", n));
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return FMK_OK;
    k_parkinson<<<fmk_grid_blocks(ctx, n), 256, 0, ctx->stream>>>(d_high, d_low, n, d_out);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}
