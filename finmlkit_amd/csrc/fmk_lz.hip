// fmk_lz.hip -- entropy of an encoded series (Lopez de Prado, Advances in Financial Machine Learning, ch. 18): the encoding of a
// float64 series into uint8 codes, the rolling plug-in entropy of its words and Kontoyiannis' sliding-window Lempel-Ziv estimator.
// The reference has none of them; the definitions are this project's (include/fmk.h).  What decides a value
// -- the code of an element, the invalid rule, the id of a word, the run read from equality masks -- is fmk_lz_rule.h.
//
// encode            one lane per element, the edges in LDS, a binary search.
// match lengths     L[p] = 1 + max over d = 1 .. n of min(n, matches in a row from p on at lag d).  The match length belongs to the
//                   position, not to the rolling window it is read through, so it is taken once per element.  A workgroup of four
//                   waves owns 256 positions and stages codes[lo - n .. lo + 192 + 64 nw), nw = 1 + (n + 62) / 64 mask words per
//                   wave; outside the series a staged code is invalid.  A prefix count of the invalid codes over the staged span
//                   tells every lane whether codes[p - n .. p + n) holds one (then L[p] = 0; that covers p < n and p > N - n too).
//                   Per lag a wave forms its nw equality words with __ballot, last word first, carrying the ones that run on from
//                   the words behind (fmk_lz_cont): the words stay in scalar registers, a lane's run starts at its own bit of
//                   word 0 (fmk_lz_run).  nw ballots per wave and lag whatever the data: a constant message costs what a random
//                   one does.
// Kontoyiannis      H[t] = log2(n + 1) / count * sum of 1 / L[p] over the count = window - 2 n + 1 positions p = t - window + 1 + n
//                   .. t - n + 1, oldest first: the lockstep walk of fmk_window.h over 1 / L, NaN where L is 0.  L lives in a block
//                   of the context's pool for the length of the call.
// plug-in           a workgroup is ONE wave and owns 256 consecutive outputs.  The state is integer: the histogram of the word ids
//                   of the window in LDS (built once with LDS adds whose results nobody reads, then one word leaves and one enters
//                   per output) and the number of words that hold an invalid code.  Per output the wave sums c(v) * (log2 M -
//                   log2 c(v)) over the word ids v, lane l taking v = l, l + 64, .. ascending, then a butterfly: the order is a
//                   function of the alphabet and the word alone.  Divided by M and by the word length that is
//                   (log2 M - (1 / M) sum_c N_c log2 c) / word, and exactly 0.0 where every word is the same: log2 M - log2 c
//                   comes from one table (one small launch in front: k_lz_logtab), whose entry M is 0.0.
#include <math.h>

#include "fmk_common.h"
#include "fmk_lz_rule.h"
#include "fmk_window.h"

#define LZ_BLOCK 256                 // lanes per workgroup of encode, match lengths and the Kontoyiannis mean
#define LZ_TILE 256                  // positions per workgroup of the match lengths: one per lane
#define LZ_MAX_NW (1 + (FMK_LZ_MAX_LOOKBACK + 62) / 64)
#define LZ_MAX_SPAN (FMK_LZ_MAX_LOOKBACK + LZ_TILE - 64 + 64 * LZ_MAX_NW)
#define LZ_MEAN_OPL 4                // outputs per lane of the Kontoyiannis mean
#define LZ_MEAN_TILE (LZ_BLOCK * LZ_MEAN_OPL)
#define LZ_PLUG_RUN 256              // consecutive outputs per wave of the plug-in entropy

namespace {

__host__ __device__ __forceinline__ int lz_mask_words(int n) { return 1 + (n + 62) / 64; }
__host__ __device__ __forceinline__ int lz_span(int n) { return n + LZ_TILE - 64 + 64 * lz_mask_words(n); }
static_assert(LZ_MAX_SPAN == 2304, "k_lz_match's static LDS");
static_assert(FMK_LZ_MAX_EDGES == 254 && FMK_LZ_MAX_ALPHABET == 255 && FMK_LZ_MAX_WORDS == 4096 && FMK_LZ_MAX_WINDOW == 4096 &&
                  FMK_LZ_MAX_LOOKBACK == 1024,
              "the rules of fmk_common.h spell the limits out in their messages");

__global__ __launch_bounds__(LZ_BLOCK) void k_lz_encode(const double *__restrict__ x, int64_t n, const double *__restrict__ edges, int n_edges,
                                                        uint8_t *__restrict__ out)
{
    __shared__ double e[FMK_LZ_MAX_EDGES];
    for (int i = threadIdx.x; i < n_edges; i += LZ_BLOCK) e[i] = edges[i];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * LZ_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LZ_BLOCK)
        out[i] = fmk_lz_code(e, n_edges, x[i]);
}

__global__ __launch_bounds__(LZ_BLOCK) void k_lz_match(const uint8_t *__restrict__ codes, int64_t N, int n, uint16_t *__restrict__ out)
{
    __shared__ uint8_t cds[LZ_MAX_SPAN];                             // cds[i] = codes[lo - n + i]
    __shared__ uint16_t pre[LZ_MAX_SPAN + 1];                        // pre[i] = invalid codes among cds[0 .. i)
    __shared__ int wave_total[LZ_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = lz_mask_words(n), span = lz_span(n);
    const int64_t lo = (int64_t)blockIdx.x * LZ_TILE;
    for (int i = tid; i < span; i += LZ_BLOCK) {
        const int64_t g = lo - n + i;
        cds[i] = g >= 0 && g < N ? codes[g] : (uint8_t)FMK_LZ_INVALID;
    }
    __syncthreads();
    // the prefix count: a lane counts a chunk, a scan over the wave, the waves' totals through LDS
    const int chunk = (span + LZ_BLOCK - 1) / LZ_BLOCK;
    const int a = tid * chunk < span ? tid * chunk : span, b = a + chunk < span ? a + chunk : span;
    int cnt = 0;
    for (int i = a; i < b; ++i) cnt += fmk_lz_invalid(cds[i], FMK_LZ_INVALID) ? 1 : 0;
    const int incl = fmk_wave_iscan(cnt);
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int run = incl - cnt;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
    if (tid == 0) pre[0] = 0;
    for (int i = a; i < b; ++i) {
        run += fmk_lz_invalid(cds[i], FMK_LZ_INVALID) ? 1 : 0;
        pre[i + 1] = (uint16_t)run;
    }
    __syncthreads();

    const int at = n + wave * 64 + lane;                             // this lane's position in the staged span; at + n <= span
    const bool invalid = pre[at + n] != pre[at - n];
    const uint8_t *mine = cds + at;                                  // mine[64 j] is bit `lane` of word j; mine[64 j - d] lies in the span
    int best = 0;
    for (int d = 1; d <= n; ++d) {
        int cont = 0;
        for (int j = nw - 1; j >= 1; --j) cont = fmk_lz_cont(__ballot(mine[64 * j] == mine[64 * j - d]), cont);
        const int r = fmk_lz_run(__ballot(mine[0] == mine[-d]), lane, cont, n);
        best = r > best ? r : best;
    }
    const int64_t p = lo + wave * 64 + lane;
    if (p < N) out[p] = fmk_lz_lambda(best, invalid);
}

struct LzMeanArgs {
    const uint16_t *lam;
    double *out;
    int64_t n;
    int window, lookback, count;     // count = window - 2 lookback + 1 terms per output
    double scale;                    // log2(lookback + 1) / count
    int slab;
};

__global__ __launch_bounds__(LZ_BLOCK) void k_lz_mean(LzMeanArgs a)
{
    extern __shared__ double lz_lds[];
    const int64_t t0 = a.window - 1 + (int64_t)blockIdx.x * LZ_MEAN_TILE;
    const int64_t t1 = t0 + LZ_MEAN_TILE < a.n ? t0 + LZ_MEAN_TILE : a.n;
    const int64_t lo = t0 - a.window + 1 + a.lookback;               // the first position output t0 reads; t1 - 1 reads up to t1 - lookback
    const int64_t span = (t1 - t0) + a.count - 1;
    const uint16_t *lam = a.lam;
    auto load = [lam, lo](int64_t i) {
        const uint16_t v = lam[lo + i];
        return v ? 1.0 / (double)v : (double)NAN;
    };
    double s[LZ_MEAN_OPL];
#pragma unroll
    for (int r = 0; r < LZ_MEAN_OPL; ++r) s[r] = 0.0;
    fmk_window_walk<LZ_BLOCK, LZ_MEAN_OPL>(lz_lds, span, a.count, a.slab, true, load, [&](int r, double v) { s[r] += v; });
#pragma unroll
    for (int r = 0; r < LZ_MEAN_OPL; ++r) {
        const int64_t t = t0 + r * LZ_BLOCK + threadIdx.x;
        if (t < t1) a.out[t] = a.scale * s[r];
    }
}

// tab[c] = log2 M - log2 c for c = 1 .. M, tab[0] = 0.0 (an empty bin adds 0 * tab[0])
__global__ __launch_bounds__(LZ_BLOCK) void k_lz_logtab(double *tab, int M)
{
    const int c = blockIdx.x * LZ_BLOCK + threadIdx.x;
    if (c <= M) tab[c] = c ? log2((double)M) - log2((double)c) : 0.0;
}

struct LzPlugArgs {
    const uint8_t *codes;
    const double *tab;
    double *out;
    int64_t n;
    int window, word, alphabet, bins;
};

// LDS of one workgroup: the table (M + 1 doubles), the histogram (bins words), the codes of the run (window + LZ_PLUG_RUN - 1 bytes)
size_t lz_plug_lds(int window, int word, int bins)
{
    return sizeof(double) * (size_t)(window - word + 2) + sizeof(unsigned) * (size_t)bins + (size_t)(window + LZ_PLUG_RUN - 1);
}

__global__ __launch_bounds__(64) void k_lz_plugin(LzPlugArgs a)
{
    extern __shared__ double lz_lds[];
    const int lane = threadIdx.x;
    const int M = a.window - a.word + 1;                             // words per window
    double *tab = lz_lds;
    unsigned *hist = (unsigned *)(tab + M + 1);
    uint8_t *cds = (uint8_t *)(hist + a.bins);
    const int64_t t0 = a.window - 1 + (int64_t)blockIdx.x * LZ_PLUG_RUN;
    const int64_t t1 = t0 + LZ_PLUG_RUN < a.n ? t0 + LZ_PLUG_RUN : a.n;
    const int64_t lo = t0 - a.window + 1;                            // cds[i] = codes[lo + i], i < t1 - lo <= window + LZ_PLUG_RUN - 1
    const int ncodes = (int)(t1 - lo);
    for (int c = lane; c <= M; c += 64) tab[c] = a.tab[c];
    for (int v = lane; v < a.bins; v += 64) hist[v] = 0;
    for (int i = lane; i < ncodes; i += 64) cds[i] = a.codes[lo + i];
    __syncthreads();
    int bad = 0;                                                     // words of the window that hold an invalid code
    for (int i = lane; i < M; i += 64) {
        const int id = fmk_lz_word_id(cds + i, a.word, a.alphabet);
        if (id < 0) ++bad;
        else atomicAdd(&hist[id], 1u);                               // (integer, the result unused: no order to depend on)
    }
    bad = fmk_wave_sum(bad);
    __syncthreads();
    const double div_m = (double)M, div_w = (double)a.word;
    double keep = 0.0;                                               // lane s & 63 keeps output s until the wave stores 64 of them
    const int runs = (int)(t1 - t0);
    for (int s = 0; s < runs; ++s) {
        if (s > 0) {                                                 // word s - 1 leaves, word s - 1 + M enters
            const int leaves = fmk_lz_word_id(cds + s - 1, a.word, a.alphabet);
            const int enters = fmk_lz_word_id(cds + s - 1 + M, a.word, a.alphabet);
            bad += (enters < 0 ? 1 : 0) - (leaves < 0 ? 1 : 0);
            if (lane == 0) {
                if (leaves >= 0) hist[leaves] -= 1u;
                if (enters >= 0) hist[enters] += 1u;
            }
            __syncthreads();
        }
        double acc = 0.0;
        for (int v = lane; v < a.bins; v += 64) {
            const unsigned c = hist[v];
            acc += (double)c * tab[c];
        }
        __syncthreads();                                             // the histogram is read: the next output may change it
        const double h = bad ? (double)NAN : fmk_wave_sum(acc) / div_m / div_w;
        if (lane == (s & 63)) keep = h;
        if ((s & 63) == 63 || s == runs - 1) {
            if (lane <= (s & 63)) a.out[t0 + (s & ~63) + lane] = keep;
        }
    }
}

}  // namespace

extern "C" int fmk_encode_dev(fmk_ctx *ctx, const double *d_x, int64_t n, const double *edges, int64_t n_edges, uint8_t *d_codes)
{
    FMK_TRY(fmk_rule_encode(ctx, edges, n_edges));
    FMK_TRY(fmk_series_check(ctx, "encode", n));
    if (n == 0) return FMK_OK;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    void *d_e;
    FMK_TRY(fmk_alloc(ctx, sizeof(double) * (size_t)n_edges, &d_e));
    int rc = fmk_h2d(ctx, d_e, edges, sizeof(double) * (size_t)n_edges);     // in the stream's order; edges is the caller's again on return
    if (rc == FMK_OK) {
        k_lz_encode<<<fmk_grid_blocks(ctx, n), LZ_BLOCK, 0, ctx->stream>>>(d_x, n, (const double *)d_e, (int)n_edges, d_codes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "k_lz_encode launch failed: %s", hipGetErrorString(e));
    }
    const int rf = fmk_free(ctx, d_e);                               // the allocator follows the stream: the kernel is ahead
    return rc != FMK_OK ? rc : rf;
}

extern "C" int fmk_match_lengths_dev(fmk_ctx *ctx, const uint8_t *d_codes, int64_t n, int64_t lookback, uint16_t *d_len)
{
    FMK_TRY(fmk_rule_match_lengths(ctx, lookback));
    FMK_TRY(fmk_series_check(ctx, "match_lengths", n));
    if (n == 0) return FMK_OK;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    k_lz_match<<<(unsigned)fmk_ceil_div(n, LZ_TILE), LZ_BLOCK, 0, ctx->stream>>>(d_codes, n, (int)lookback, d_len);
    FMK_LAUNCH_CHECK(ctx);
    return FMK_OK;
}

extern "C" int fmk_kontoyiannis_entropy_dev(fmk_ctx *ctx, const uint8_t *d_codes, int64_t n, int64_t window, int64_t lookback,
                                            double *d_out)
{
    FMK_TRY(fmk_rule_kontoyiannis(ctx, window, lookback));
    FMK_TRY(fmk_series_check(ctx, "kontoyiannis_entropy", n));
    if (n == 0) return FMK_OK;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    if (window > n) return FMK_OK;
    void *d_lam;
    FMK_TRY(fmk_alloc(ctx, sizeof(uint16_t) * (size_t)n, &d_lam));
    int rc = fmk_match_lengths_dev(ctx, d_codes, n, lookback, (uint16_t *)d_lam);
    if (rc == FMK_OK) {
        LzMeanArgs a;
        a.lam = (const uint16_t *)d_lam; a.out = d_out; a.n = n; a.window = (int)window; a.lookback = (int)lookback;
        a.count = (int)(window - 2 * lookback + 1);
        a.scale = log2((double)(lookback + 1)) / (double)a.count;
        a.slab = fmk_slab(a.count, LZ_MEAN_TILE);
        const int64_t tiles = fmk_ceil_div(n - (window - 1), LZ_MEAN_TILE);
        k_lz_mean<<<(unsigned)tiles, LZ_BLOCK, (size_t)a.slab * sizeof(double), ctx->stream>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "k_lz_mean launch failed: %s", hipGetErrorString(e));
    }
    const int rf = fmk_free(ctx, d_lam);                             // the allocator follows the stream: the kernels are ahead
    return rc != FMK_OK ? rc : rf;
}

extern "C" int fmk_plugin_entropy_dev(fmk_ctx *ctx, const uint8_t *d_codes, int64_t n, int64_t window, int64_t word, int64_t alphabet,
                                      double *d_out)
{
    FMK_TRY(fmk_rule_plugin_entropy(ctx, window, word, alphabet));
    FMK_TRY(fmk_series_check(ctx, "plugin_entropy", n));
    if (n == 0) return FMK_OK;
    FMK_HIP(ctx, hipSetDevice(ctx->device));
    FMK_TRY(fmk_nan_head(ctx, d_out, n, window));
    if (window > n) return FMK_OK;
    const int M = (int)(window - word + 1);
    void *d_tab;
    FMK_TRY(fmk_alloc(ctx, sizeof(double) * (size_t)(M + 1), &d_tab));
    k_lz_logtab<<<(unsigned)fmk_ceil_div(M + 1, LZ_BLOCK), LZ_BLOCK, 0, ctx->stream>>>((double *)d_tab, M);
    LzPlugArgs a;
    a.codes = d_codes; a.tab = (const double *)d_tab; a.out = d_out; a.n = n;
    a.window = (int)window; a.word = (int)word; a.alphabet = (int)alphabet; a.bins = fmk_lz_bins(alphabet, word);
    const int64_t runs = fmk_ceil_div(n - (window - 1), LZ_PLUG_RUN);
    k_lz_plugin<<<(unsigned)runs, 64, lz_plug_lds(a.window, a.word, a.bins), ctx->stream>>>(a);
    const hipError_t e = hipGetLastError();
    int rc = FMK_OK;
    if (e != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "k_lz_plugin launch failed: %s", hipGetErrorString(e));
    const int rf = fmk_free(ctx, d_tab);                             // the allocator follows the stream: the kernels are ahead
    return rc != FMK_OK ? rc : rf;
}
