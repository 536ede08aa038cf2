// fmk_otr_rule.h -- everything of the optimal-trading-rule mesh (fmk_otr.hip) that decides a bit: the counter index of
// a random word, the uniform it becomes, the polar pair of normal variates, the step of the discrete Ornstein-Uhlenbeck path, the
// levels a step newly passes (the hitting records), a node's exit from two records, and the statistics of a node's sums.  Plain
// C++17, every floating-point operation rounded on its own (the library and the tool are built without contraction), so that the
// kernel and a host program (tools/otr_check.cpp) run the same text.  The logarithm is the host's (fmk_log.h), which under hipcc
// exists on the device alone: the functions here are qualified like its own, not __host__ __device__.
#pragma once

#include <math.h>
#include <stdint.h>

#include "fmk_log.h"
#include "fmk_seqboot_rule.h"

#ifdef __HIPCC__
#define FMK_OTR_FN __device__ __forceinline__
#else
#define FMK_OTR_FN static inline
#endif

#define FMK_OTR_MAX_LEVELS 32                        // profit-taking levels, and stop-loss levels, of a mesh
#define FMK_OTR_MAX_HP 4096                          // steps of a path: a record's step fits 16 bits, a pair's number 12
#define FMK_OTR_MAX_PATHS ((int64_t)1 << 32)
#define FMK_OTR_MAX_CFG 1024
#define FMK_OTR_BLOCK 512                            // B: paths of one block of the sums (a constant of the library)
#define FMK_OTR_TILE 64                              // paths walked at once: one per lane
#define FMK_OTR_ATTEMPTS 64                          // polar attempts before a pair is (0, 0)
#define FMK_OTR_NONE 0xFFFFu                         // the step of a level that was not passed

#define FMK_OTR_PROFIT 0
#define FMK_OTR_STOP 1
#define FMK_OTR_TIME 2

// the counter of word w (0: u, 1: v) of attempt a at pair k of path p
FMK_OTR_FN uint64_t fmk_otr_index(uint64_t p, uint32_t k, uint32_t a, uint32_t w)
{
    return ((((p << 12) | (uint64_t)k) << 6 | (uint64_t)a) << 1) | (uint64_t)w;
}

// 53 bits of the word -> [-1, 1), exact
FMK_OTR_FN double fmk_otr_uniform(uint64_t word) { return (double)(word >> 11) * 0x1p-52 - 1.0; }

// Marsaglia's polar method on the counter words: the pair of pair k of path p -> the attempts made (FMK_OTR_ATTEMPTS + 1: none
// was accepted and the pair is (0, 0))
FMK_OTR_FN int fmk_otr_pair(uint64_t seed, uint64_t p, uint32_t k, double *z0, double *z1)
{
    for (uint32_t a = 0; a < FMK_OTR_ATTEMPTS; ++a) {
        const double u = fmk_otr_uniform(fmk_sb_word(seed, fmk_otr_index(p, k, a, 0)));
        const double v = fmk_otr_uniform(fmk_sb_word(seed, fmk_otr_index(p, k, a, 1)));
        const double uu = u * u, vv = v * v;
        const double s = uu + vv;
        if (s < 1.0 && s != 0.0) {
            const double f = sqrt((-2.0 * fmk_log_host(s)) / s);
            *z0 = u * f;
            *z1 = v * f;
            return (int)a + 1;
        }
    }
    *z0 = 0.0;
    *z1 = 0.0;
    return FMK_OTR_ATTEMPTS + 1;
}

FMK_OTR_FN double fmk_otr_c0(double forecast, double phi) { return (1.0 - phi) * forecast; }

// P_h = (c0 + phi * P_{h-1}) + sigma * z_h
FMK_OTR_FN double fmk_otr_step(double c0, double phi, double sigma, double P, double z)
{
    const double drift = phi * P;
    const double mean = c0 + drift;
    const double shock = sigma * z;
    return mean + shock;
}

// The levels that P = P_h newly passes: ip / is are the next profit-taking / stop-loss level not passed so far (the lists are
// sorted, so the running maximum passes pt[0], pt[1], ... in order and the running minimum the sl levels); rec(record, h, P) is
// called for every level passed at this step, records 0 .. n_pt-1 for pt and n_pt .. n_pt+n_sl-1 for sl.  The inequalities are
// strict (snippet 13.2): a value on a level does not pass it, and +inf is never passed.
template <class Rec>
FMK_OTR_FN void fmk_otr_cross(double P, uint32_t h, const double *pt, int n_pt, const double *sl, int n_sl, int *ip, int *is, Rec &&rec)
{
    while (*ip < n_pt && P > pt[*ip]) { rec(*ip, h, P); ++*ip; }
    while (*is < n_sl && P < -sl[*is]) { rec(n_pt + *is, h, P); ++*is; }
}
// no node is alive once all the levels of one side are passed
FMK_OTR_FN bool fmk_otr_done(int ip, int n_pt, int is, int n_sl) { return ip >= n_pt || is >= n_sl; }

// Node (i, j) from the steps of its two records (FMK_OTR_NONE: not passed): the earlier one is its exit.  Equal steps are two
// FMK_OTR_NONE (pt, sl >= 0: one value cannot pass both), the time exit at max_hp with the path's last value.
FMK_OTR_FN int fmk_otr_kind(uint32_t h_pt, uint32_t h_sl) { return h_pt < h_sl ? FMK_OTR_PROFIT : h_sl < h_pt ? FMK_OTR_STOP : FMK_OTR_TIME; }
FMK_OTR_FN uint32_t fmk_otr_exit_step(int kind, uint32_t h_pt, uint32_t h_sl, uint32_t max_hp)
{
    return kind == FMK_OTR_PROFIT ? h_pt : kind == FMK_OTR_STOP ? h_sl : max_hp;
}

// one result into a node's block sums: the product is rounded, then added
FMK_OTR_FN void fmk_otr_add(double x, double *s1, double *s2)
{
    const double xx = x * x;
    *s1 = *s1 + x;
    *s2 = *s2 + xx;
}

// the statistics of a node from its totals over n paths
FMK_OTR_FN void fmk_otr_stats(double S1, double S2, double n, double *mean, double *std, double *sharpe)
{
    const double m = S1 / n;
    const double ex2 = S2 / n;
    const double mm = m * m;
    double var = ex2 - mm;
    if (var < 0.0) var = 0.0;
    const double sd = sqrt(var);
    *mean = m;
    *std = sd;
    *sharpe = m / sd;
}
