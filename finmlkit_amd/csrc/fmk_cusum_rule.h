// fmk_cusum_rule.h -- what every CUSUM kernel shares (fmk_cusum.hip with fmk_cusum_onepass.h and fmk_cusum_filter.h, fmk_cusum_chain.hip):
// the two-component state, the two per-tick rules, the loop inputs of the bar indexer and the lane broadcast.  Each of them decides
// closes bit for bit, so each stands here once.  The two tick rules are plain C++, so that a host program can check them against the
// reference's branching loops (tools/cusumrule_check.cpp); the loop inputs need the device logarithm and are device code.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include "fmk_common.h"
#include "fmk_log.h"
#define FMK_HD __host__ __device__ __forceinline__
#else
#define FMK_HD static inline
#endif

// One tick of _cusum_bar_indexer's loop (finmlkit/bar/logic.py:199-219) as selects -> 1 if the tick closes a bar.  The states are
// never NaN and never -0.0: every zero is the literal 0.0 of a clamp or a reset.  A NaN lam is "this tick cannot close".
FMK_HD unsigned cs_tick(double &sp, double &sn, double r, double lam)
{
    const double a = sp + r, b = sn + r;
    sp = a > 0.0 ? a : 0.0;                                              // max(0.0, s_pos + ret): NaN -> 0.0
    sn = b < 0.0 ? b : 0.0;                                              // min(0.0, s_neg + ret)
    const bool cp = sp >= lam;
    const bool cn = !cp && sn <= -lam;                                   // elif: the positive side first
    sp = cp ? 0.0 : sp;
    sn = cn ? 0.0 : sn;
    return (cp | cn) ? 1u : 0u;
}

// One tick of the symmetric CUSUM event filter (finmlkit/sampling/filters.py:7-70) as selects -> 1 if the tick is an event
FMK_HD unsigned cf_tick(double &sp, double &sn, double r, double l)
{
    const double a = sp + r, b = sn + r;
    sp = a > 0.0 ? a : 0.0;                                              // max(0.0, s_pos + ret): NaN -> 0.0
    sn = b < 0.0 ? b : 0.0;                                              // min(0.0, s_neg + ret)
    const bool cn = sn < -l;                                             // the negative side first, strict
    const bool cp = !cn && sp > l;
    sn = cn ? 0.0 : sn;
    sp = cp ? 0.0 : sp;
    return (cn | cp) ? 1u : 0u;
}

#ifdef __HIPCC__
struct CsState { double sp, sn; };

__device__ __forceinline__ bool cs_same(CsState a, CsState b)
{
    return __double_as_longlong(a.sp) == __double_as_longlong(b.sp) && __double_as_longlong(a.sn) == __double_as_longlong(b.sn);
}

// value of lane `src` (wave-uniform index) broadcast to the wave
__device__ __forceinline__ double cs_lane(double v, int src)
{
    return __longlong_as_double(fmk_readlane((int64_t)__double_as_longlong(v), src));
}

// The bar indexer's loop inputs of tick i from the raw columns (p = price[i], pm = price[i - 1], sg = sigma[i], tsi = ts[i],
// tsn = ts[i + 1] where has_next says there is one):
//   r   = log(p_i / p_{i-1})                                                (logic.py:200)
//   lam = max(sigma_mult * sigma_i, sigma_floor), NaN inside a same-timestamp print block (logic.py:206-211): a NaN threshold can
//         never be reached, which is exactly "this tick cannot close a bar"; a NaN sigma gives a NaN lam as well
__device__ __forceinline__ void cs_input(double p, double pm, double sg, int64_t tsi, int64_t tsn, bool has_next, double sigma_floor,
                                         double sigma_mult, double &r, double &lam)
{
    r = fmk_log_ratio(p, pm);
    lam = NAN;
    if (!(has_next && tsi == tsn)) {
        lam = sigma_mult * sg;
        lam = sigma_floor > lam ? sigma_floor : lam;                     // max(lam, floor): a NaN lam stays NaN
    }
}
#endif
