// fmk_otr.hip -- the optimal trading rules of Advances in Financial Machine Learning, chapter 13: many paths of a
// discrete Ornstein-Uhlenbeck process, each closed at a profit-taking level, a stop-loss level or the maximum holding period, for every
// pair of a mesh of levels; the mean, the deviation and the Sharpe ratio of every pair.  Every bit is fmk_otr_rule.h's.
//   k_otr_walk   one workgroup (one wave) per (parameter set, block of FMK_OTR_BLOCK paths).  The block goes tile by tile, 64 paths
//                each.  Phase 1: a lane walks one path ONCE and leaves, for every level the path passes, the step and the value at
//                which it first did (the levels are sorted: two counters per lane) -- in LDS, step as 16 bits, value as float64,
//                one row per level; it stops at max_hp or when all levels of one side are passed.  Phase 2: the lanes own nodes
//                (NPL of them each, in registers) and go over the tile's paths in path order, which is the definition's summing
//                order: node (i, j) exits at the earlier of record i and record n_pt + j, else at max_hp with the path's last
//                value.  After the last tile: one partial (S1, S2) per node to memory, the three integer sums by atomics.
//   k_otr_final  one thread per (parameter set, node): the partials in block order, then the statistics.
// The rows are padded (33 dwords of steps, 65 float64 of values), so that the 32 levels a wave may read at one path fall on
// different banks.  LDS is (n_pt + n_sl) * 652 B + 1 KiB, 42 KiB at 32 + 32 levels: three workgroups per CU at the least.
#include <vector>

#include "fmk_common.h"
#include "fmk_otr_rule.h"

namespace {

constexpr int OTR_STEP_ROW = FMK_OTR_TILE + 2;       // uint16 per level: 33 dwords
constexpr int OTR_VAL_ROW = FMK_OTR_TILE + 1;        // float64 per level
constexpr int OTR_MAX_NPL = FMK_OTR_MAX_LEVELS * FMK_OTR_MAX_LEVELS / FMK_OTR_TILE;
constexpr size_t OTR_PARTIAL_CAP = (size_t)256 << 20;  // partials of one launch (more parameter sets: more launches)
constexpr int64_t OTR_MAX_GRID_X = ((int64_t)1 << 31) - 1;

static_assert(FMK_OTR_BLOCK % FMK_OTR_TILE == 0 && FMK_OTR_TILE == FMK_WAVE, "a block is whole tiles, a tile is one wave");
static_assert((int64_t)FMK_OTR_BLOCK * FMK_OTR_MAX_HP < ((int64_t)1 << 31), "a block's sum of exit steps is 32-bit in the kernel");
static_assert(FMK_OTR_MAX_HP < FMK_OTR_NONE, "a step fits a record");
static_assert(FMK_OTR_MAX_PATHS / FMK_OTR_BLOCK <= OTR_MAX_GRID_X, "one grid row holds the blocks of a parameter set");

struct OtrArgs {
    const double *cfg;                     // [n_cfg][3]: forecast, phi, sigma
    const double *levels;                  // pt[n_pt] | sl[n_sl]
    const double *normals;                 // [n_paths][max_hp] or null
    double2 *partial;                      // [cfgs of the launch][blocks][nodes]: S1, S2
    unsigned long long *n_profit, *n_stop, *hold;      // [n_cfg][nodes]
    uint64_t seed;
    int64_t n_paths, n_blocks;
    int c0;                                // first parameter set of the launch
    int n_pt, n_sl, max_hp;
};

size_t otr_lds_bytes(int L) { return (size_t)L * (OTR_VAL_ROW * 8 + OTR_STEP_ROW * 2) + (size_t)FMK_OTR_TILE * 8 + 2 * FMK_OTR_MAX_LEVELS * 8; }

template <int NPL, bool GEN>
__global__ __launch_bounds__(FMK_OTR_TILE) void k_otr_walk(const OtrArgs a)
{
    extern __shared__ double s_mem[];
    const int n_pt = a.n_pt, n_sl = a.n_sl, L = n_pt + n_sl, nodes = n_pt * n_sl, max_hp = a.max_hp;
    double *s_val = s_mem;                                           // [L][OTR_VAL_ROW]
    double *s_last = s_val + (size_t)L * OTR_VAL_ROW;                // [TILE]
    double *s_pt = s_last + FMK_OTR_TILE;                            // [MAX_LEVELS]
    double *s_sl = s_pt + FMK_OTR_MAX_LEVELS;                        // [MAX_LEVELS]
    uint16_t *s_step = (uint16_t *)(s_sl + FMK_OTR_MAX_LEVELS);      // [L][OTR_STEP_ROW]
    const int lane = threadIdx.x;
    const int c = a.c0 + (int)blockIdx.y;
    const int64_t b = blockIdx.x;

    if (lane < n_pt) s_pt[lane] = a.levels[lane];
    if (lane < n_sl) s_sl[lane] = a.levels[n_pt + lane];
    const double forecast = a.cfg[c * 3], phi = a.cfg[c * 3 + 1], sigma = a.cfg[c * 3 + 2];
    const double c0 = fmk_otr_c0(forecast, phi);

    // the nodes of this lane: node = lane + 64 q -> the rows of its two records
    int row_pt[NPL], row_sl[NPL];
    double S1[NPL], S2[NPL];
    uint32_t n_profit[NPL], n_stop[NPL], hold[NPL];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int node = lane + FMK_OTR_TILE * q;
        row_pt[q] = node < nodes ? node / n_sl : -1;
        row_sl[q] = node < nodes ? n_pt + node % n_sl : -1;
        S1[q] = 0.0; S2[q] = 0.0;
        n_profit[q] = 0; n_stop[q] = 0; hold[q] = 0;
    }
    __syncthreads();

    const int64_t p_begin = b * FMK_OTR_BLOCK;
    const int64_t p_end = p_begin + FMK_OTR_BLOCK < a.n_paths ? p_begin + FMK_OTR_BLOCK : a.n_paths;
    for (int64_t p0 = p_begin; p0 < p_end; p0 += FMK_OTR_TILE) {
        const int cnt = p_end - p0 < FMK_OTR_TILE ? (int)(p_end - p0) : FMK_OTR_TILE;
        // ---- phase 1: lane = path
        for (int r = 0; r < L; ++r) s_step[r * OTR_STEP_ROW + lane] = (uint16_t)FMK_OTR_NONE;
        if (lane < cnt) {
            const uint64_t p = (uint64_t)(p0 + lane);
            const double *zrow = GEN ? nullptr : a.normals + (size_t)p * (size_t)max_hp;
            auto rec = [&](int r, uint32_t h, double P) {
                s_step[r * OTR_STEP_ROW + lane] = (uint16_t)h;
                s_val[r * OTR_VAL_ROW + lane] = P;
            };
            double P = 0.0;
            int ip = 0, is = 0;
            for (int h = 1; h <= max_hp; h += 2) {
                double z0, z1 = 0.0;
                if constexpr (GEN) (void)fmk_otr_pair(a.seed, p, (uint32_t)((h - 1) >> 1), &z0, &z1);
                else { z0 = zrow[h - 1]; if (h < max_hp) z1 = zrow[h]; }
                P = fmk_otr_step(c0, phi, sigma, P, z0);
                fmk_otr_cross(P, (uint32_t)h, s_pt, n_pt, s_sl, n_sl, &ip, &is, rec);
                if (fmk_otr_done(ip, n_pt, is, n_sl) || h == max_hp) break;
                P = fmk_otr_step(c0, phi, sigma, P, z1);
                fmk_otr_cross(P, (uint32_t)(h + 1), s_pt, n_pt, s_sl, n_sl, &ip, &is, rec);
                if (fmk_otr_done(ip, n_pt, is, n_sl)) break;
            }
            s_last[lane] = P;
        }
        __syncthreads();
        // ---- phase 2: lane = nodes, the tile's paths in order
        for (int t = 0; t < cnt; ++t) {
            const double last = s_last[t];
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                if (row_pt[q] < 0) continue;
                const uint32_t h_pt = s_step[row_pt[q] * OTR_STEP_ROW + t], h_sl = s_step[row_sl[q] * OTR_STEP_ROW + t];
                const int kind = fmk_otr_kind(h_pt, h_sl);
                const double x = kind == FMK_OTR_PROFIT ? s_val[row_pt[q] * OTR_VAL_ROW + t]
                                 : kind == FMK_OTR_STOP ? s_val[row_sl[q] * OTR_VAL_ROW + t] : last;
                fmk_otr_add(x, &S1[q], &S2[q]);
                n_profit[q] += kind == FMK_OTR_PROFIT;
                n_stop[q] += kind == FMK_OTR_STOP;
                hold[q] += fmk_otr_exit_step(kind, h_pt, h_sl, (uint32_t)max_hp);
            }
        }
        __syncthreads();
    }

    double2 *part = a.partial + ((size_t)blockIdx.y * (size_t)a.n_blocks + (size_t)b) * (size_t)nodes;
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int node = lane + FMK_OTR_TILE * q;
        if (node >= nodes) continue;
        part[node] = make_double2(S1[q], S2[q]);
        const size_t o = (size_t)c * (size_t)nodes + (size_t)node;
        if (n_profit[q]) atomicAdd(a.n_profit + o, (unsigned long long)n_profit[q]);
        if (n_stop[q]) atomicAdd(a.n_stop + o, (unsigned long long)n_stop[q]);
        atomicAdd(a.hold + o, (unsigned long long)hold[q]);
    }
}

struct OtrFinal {
    const double2 *partial;
    double *mean, *std, *sharpe;
    const int64_t *n_profit, *n_stop;
    int64_t *n_time;
    int64_t n_paths, n_blocks;
    int c0, n_cfg_launch, nodes;
};

__global__ __launch_bounds__(256) void k_otr_final(const OtrFinal f)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)f.n_cfg_launch * f.nodes) return;
    const int cl = (int)(i / f.nodes), node = (int)(i % f.nodes);
    const double2 *part = f.partial + (size_t)cl * (size_t)f.n_blocks * (size_t)f.nodes + (size_t)node;
    double S1 = 0.0, S2 = 0.0;
    for (int64_t b = 0; b < f.n_blocks; ++b) {
        const double2 v = part[(size_t)b * (size_t)f.nodes];
        S1 = S1 + v.x;
        S2 = S2 + v.y;
    }
    const size_t o = (size_t)(f.c0 + cl) * (size_t)f.nodes + (size_t)node;
    fmk_otr_stats(S1, S2, (double)f.n_paths, &f.mean[o], &f.std[o], &f.sharpe[o]);
    f.n_time[o] = f.n_paths - f.n_profit[o] - f.n_stop[o];
}

template <int NPL>
void otr_launch(const OtrArgs &a, dim3 grid, size_t lds, hipStream_t st)
{
    if (a.normals) k_otr_walk<NPL, false><<<grid, FMK_OTR_TILE, lds, st>>>(a);
    else k_otr_walk<NPL, true><<<grid, FMK_OTR_TILE, lds, st>>>(a);
}

bool otr_finite(double x) { return x - x == 0.0; }

int otr_check_levels(fmk_ctx *ctx, const char *name, const double *v, int64_t n)
{
    if (n < 1 || n > FMK_OTR_MAX_LEVELS) return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: between 1 and 32 %s levels.", name);
    if (!v) return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: a null input");
    for (int64_t i = 0; i < n; ++i)
        if (!(v[i] >= 0.0) || (i && !(v[i - 1] <= v[i])))
            return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: the %s levels must be non-negative and non-decreasing, without NaN.", name);
    return FMK_OK;
}

}  // namespace

extern "C" int fmk_otr_geometry(int64_t *out4)
{
    out4[0] = FMK_OTR_BLOCK;
    out4[1] = FMK_OTR_TILE;
    out4[2] = FMK_OTR_MAX_LEVELS;
    out4[3] = FMK_OTR_MAX_HP;
    return FMK_OK;
}

extern "C" int fmk_otr_mesh(fmk_ctx *ctx, const double *forecast, const double *phi, const double *sigma, int64_t n_cfg,
                            const double *pt, int64_t n_pt, const double *sl, int64_t n_sl, int64_t max_hp, int64_t n_paths,
                            uint64_t seed, const double *normals, double *mean, double *std_, double *sharpe, int64_t *n_profit,
                            int64_t *n_stop, int64_t *n_time, int64_t *hold)
{
    if (n_cfg < 1 || n_cfg > FMK_OTR_MAX_CFG) return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: between 1 and 1024 parameter sets.");
    if (max_hp < 1 || max_hp > FMK_OTR_MAX_HP) return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: max_hp must be between 1 and 4096.");
    if (n_paths < 1 || n_paths > FMK_OTR_MAX_PATHS) return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: n_paths must be between 1 and 2^32.");
    FMK_TRY(otr_check_levels(ctx, "profit-taking", pt, n_pt));
    FMK_TRY(otr_check_levels(ctx, "stop-loss", sl, n_sl));
    if (!forecast || !phi || !sigma) return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: a null input");
    for (int64_t c = 0; c < n_cfg; ++c) {
        if (!otr_finite(forecast[c]) || !otr_finite(sigma[c]) || !(phi[c] >= 0.0 && phi[c] <= 1.0) || !(sigma[c] >= 0.0))
            return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: parameter set %lld: forecast and sigma finite, 0 <= phi <= 1, sigma >= 0.",
                                 (long long)c);
    }
    const size_t n_normals = normals ? (size_t)n_paths * (size_t)max_hp : 0;
    for (size_t i = 0; i < n_normals; ++i)
        if (!otr_finite(normals[i])) return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: the normals must be finite.");
    if (!ctx) return fmk_set_error(ctx, FMK_E_ARG, "otr_mesh: a null context");

    const int nodes = (int)(n_pt * n_sl), L = (int)(n_pt + n_sl);
    const int64_t n_blocks = fmk_ceil_div(n_paths, FMK_OTR_BLOCK);
    const size_t cells = (size_t)n_cfg * (size_t)nodes;
    // parameter sets per launch: what keeps the partials under the cap (one set's partials are taken whatever their size)
    const size_t per_cfg = (size_t)n_blocks * (size_t)nodes * sizeof(double2);
    int64_t cpl = (int64_t)(OTR_PARTIAL_CAP / per_cfg);
    cpl = cpl < 1 ? 1 : cpl > n_cfg ? n_cfg : cpl;

    FMK_HIP(ctx, hipSetDevice(ctx->device));
    // one block: the parameter sets | the levels | the seven outputs | the partials | the normals
    const size_t b_cfg = (size_t)n_cfg * 24, b_lev = (size_t)L * 8, b_out = cells * 8, b_part = (size_t)cpl * per_cfg;
    const size_t o_lev = b_cfg, o_out = (o_lev + b_lev + 15) & ~(size_t)15, o_part = (o_out + 7 * b_out + 15) & ~(size_t)15, o_nrm = o_part + b_part;
    void *blk;
    FMK_TRY(fmk_alloc(ctx, o_nrm + n_normals * 8, &blk));
    char *base = (char *)blk;
    std::vector<double> h_in((size_t)n_cfg * 3 + (size_t)L);
    for (int64_t c = 0; c < n_cfg; ++c) { h_in[(size_t)c * 3] = forecast[c]; h_in[(size_t)c * 3 + 1] = phi[c]; h_in[(size_t)c * 3 + 2] = sigma[c]; }
    for (int64_t i = 0; i < n_pt; ++i) h_in[(size_t)n_cfg * 3 + (size_t)i] = pt[i];
    for (int64_t j = 0; j < n_sl; ++j) h_in[(size_t)n_cfg * 3 + (size_t)n_pt + (size_t)j] = sl[j];
    double *d_out[7];
    for (int k = 0; k < 7; ++k) d_out[k] = (double *)(base + o_out + (size_t)k * b_out);   // mean std sharpe | n_profit n_stop n_time hold
    int rc = fmk_h2d(ctx, base, h_in.data(), h_in.size() * 8);
    if (rc == FMK_OK && normals) rc = fmk_h2d(ctx, base + o_nrm, normals, n_normals * 8);
    if (rc == FMK_OK) rc = fmk_memset(ctx, d_out[3], 0, 4 * b_out);
    if (rc == FMK_OK) {
        OtrArgs a;
        a.cfg = (const double *)base;
        a.levels = (const double *)(base + o_lev);
        a.normals = normals ? (const double *)(base + o_nrm) : nullptr;
        a.partial = (double2 *)(base + o_part);
        a.n_profit = (unsigned long long *)d_out[3];
        a.n_stop = (unsigned long long *)d_out[4];
        a.hold = (unsigned long long *)d_out[6];
        a.seed = seed;
        a.n_paths = n_paths; a.n_blocks = n_blocks;
        a.n_pt = (int)n_pt; a.n_sl = (int)n_sl; a.max_hp = (int)max_hp;
        OtrFinal f;
        f.partial = a.partial;
        f.mean = d_out[0]; f.std = d_out[1]; f.sharpe = d_out[2];
        f.n_profit = (const int64_t *)d_out[3]; f.n_stop = (const int64_t *)d_out[4]; f.n_time = (int64_t *)d_out[5];
        f.n_paths = n_paths; f.n_blocks = n_blocks; f.nodes = nodes;
        const size_t lds = otr_lds_bytes(L);
        const int npl = (int)fmk_ceil_div(nodes, FMK_OTR_TILE);
        for (int64_t c0 = 0; c0 < n_cfg && rc == FMK_OK; c0 += cpl) {
            const int nc = (int)(n_cfg - c0 < cpl ? n_cfg - c0 : cpl);
            a.c0 = f.c0 = (int)c0;
            f.n_cfg_launch = nc;
            const dim3 grid((unsigned)n_blocks, (unsigned)nc);
            if (npl <= 1) otr_launch<1>(a, grid, lds, ctx->stream);
            else if (npl <= 4) otr_launch<4>(a, grid, lds, ctx->stream);
            else if (npl <= 8) otr_launch<8>(a, grid, lds, ctx->stream);
            else otr_launch<OTR_MAX_NPL>(a, grid, lds, ctx->stream);
            k_otr_final<<<(unsigned)fmk_ceil_div((int64_t)nc * nodes, 256), 256, 0, ctx->stream>>>(f);
            if (hipGetLastError() != hipSuccess) rc = fmk_set_error(ctx, FMK_E_HIP, "otr_mesh: launch");
        }
    }
    void *const h_out[7] = {mean, std_, sharpe, n_profit, n_stop, n_time, hold};
    for (int k = 0; k < 7 && rc == FMK_OK; ++k)
        if (h_out[k]) rc = fmk_d2h(ctx, h_out[k], d_out[k], b_out);
    if (rc == FMK_OK) rc = fmk_wait(ctx, hipSuccess);            // also with every output null: the call has run when it returns
    else (void)hipStreamSynchronize(ctx->stream);                // nothing of the call is left in flight behind a failure
    (void)fmk_free(ctx, blk);
    return rc;
}
