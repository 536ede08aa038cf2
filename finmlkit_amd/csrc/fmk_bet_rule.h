// fmk_bet_rule.h -- everything of bet sizing (fmk_bet.hip) that decides a bit: the signal in units of 2^-30, the pair
// (sum, count) the scan carries, the value of a tick from that pair, the discretisation and the budget value.  Plain C++17, so that
// the kernels and a host program (tools/bet_check.cpp) run the same text.  The sums in between are exact integer sums, so their
// order is free; every floating-point step is one correctly rounded IEEE operation (the library and the tool are built with
// -ffp-contract=off, and nothing here could be fused anyway: a product is never followed by a sum).
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define FMK_BET_FN __host__ __device__ __forceinline__
#else
#define FMK_BET_FN static inline
#endif

#define FMK_BET_UNIT 1073741824.0                     // 2^30: the bootstrap's UNIT
#define FMK_BET_MAX_CONC 32767                        // int16 concurrency, label_concurrency's bound
#define FMK_BET_MAX_EVENTS (((int64_t)1 << 31) - 1)   // a count (int32) never wraps; |sum| <= (2^31 - 1) * 2^30 < 2^61
#define FMK_BET_MAX_AXIS ((int64_t)1 << 32)

// q = rint(m * 2^30): the product is exact (a power of two), rint rounds once, ties to even.  false: NaN or outside [-1, 1]
FMK_BET_FN bool fmk_bet_quantise(double m, int64_t *q)
{
    if (!(m >= -1.0 && m <= 1.0)) { *q = 0; return false; }
    *q = (int64_t)rint(m * FMK_BET_UNIT);
    return true;
}

// what the scan carries: the sum of the open events' units and their number.  Two fields of their own width: with at most
// 2^31 - 1 events neither can wrap, whatever the events are, so a concurrency above the bound is always SEEN
struct FmkBetAcc {
    int64_t s;
    int32_t c;
    int32_t pad;
};
FMK_BET_FN FmkBetAcc fmk_bet_combine(const FmkBetAcc &first, const FmkBetAcc &then)
{
    FmkBetAcc r;
    r.s = (int64_t)((uint64_t)first.s + (uint64_t)then.s);
    r.c = (int32_t)((uint32_t)first.c + (uint32_t)then.c);
    r.pad = 0;
    return r;
}

// the average of the active signals: fl(S / c) * 2^-30 (one division; the scaling is exact), +0.0 where nothing is open.  For
// c <= 32767 |S| < 2^45 converts exactly.  S == 0 gives +0.0: -0.0 never appears
FMK_BET_FN double fmk_bet_value(int64_t S, int32_t c)
{
    if (c <= 0) return 0.0;
    return ((double)S / (double)c) * (1.0 / FMK_BET_UNIT);
}

FMK_BET_FN bool fmk_bet_step_ok(double step) { return step == 0.0 || (step > 0.0 && step <= 1.0); }

// snippet 10.3: min(1, max(-1, rint(v / step) * step)), one operation at a time; step == 0: v as it is
FMK_BET_FN double fmk_bet_discretise(double v, double step)
{
    if (step == 0.0) return v;
    const double k = rint(v / step);
    double r = k * step;
    r = r < -1.0 ? -1.0 : r;                          // max(-1, r) and min(1, r) on values that are never NaN
    r = r > 1.0 ? 1.0 : r;
    return r;
}

// the budget approach (§10.2): the two side counts and their maxima
struct FmkBetSides {
    int32_t l, s;
};
FMK_BET_FN FmkBetSides fmk_bet_sides_combine(const FmkBetSides &first, const FmkBetSides &then)
{
    FmkBetSides r;
    r.l = (int32_t)((uint32_t)first.l + (uint32_t)then.l);
    r.s = (int32_t)((uint32_t)first.s + (uint32_t)then.s);
    return r;
}
FMK_BET_FN double fmk_bet_budget_value(int32_t cl, int32_t cs, int32_t max_l, int32_t max_s)
{
    const double a = max_l > 0 ? (double)cl / (double)max_l : 0.0;
    const double b = max_s > 0 ? (double)cs / (double)max_s : 0.0;
    return a - b;
}
