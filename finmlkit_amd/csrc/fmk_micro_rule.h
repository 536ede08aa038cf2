// fmk_micro_rule.h -- the arithmetic of comp_bar_microstructure_features (fmk_micro.hip) that decides bits: the
// per-tick terms of a bar's differences and what becomes of the bar's moments.  Plain C++17, so that the kernels and a host program
// (tools/micro_check.cpp) run the same text.  The sums in between are the kernel's: float64, in any order that is a function of the
// bar alone.  Nothing here may be contracted into an FMA (the library is built with -ffp-contract=off; the host program too).
#pragma once

#include <math.h>
#include <stdint.h>

#include "fmk_log.h"

#ifdef __HIPCC__
#define FMK_MICRO_FN __device__ __forceinline__      // (fmk_log.h is device code there)
#else
#define FMK_MICRO_FN static inline
#endif

#define FMK_MICRO_EXACT_FIT 0x1p-26        // u = 1 - r^2 at or below this: the fit is exact (label/trend_scanning's constant)
#define FMK_MICRO_COLS 8                   // kyle_lambda, kyle_t, amihud_lambda, amihud_t, hasbrouck_lambda, hasbrouck_t, serial_cov, roll_spread

// The terms of tick t of a bar, t past the bar's first tick: p = price[t], pm = price[t - 1], v = the amount as float64, sd = the
// side as float64 (-1, 0, +1).
struct FmkMicroTerm {
    double d;                              // p - pm
    double r;                              // log(p / pm): the quotient rounded, then the host's logarithm of it (fmk_log.h)
    double xk, xa, xh;                     // sd * v;  p * v;  sd * sqrt(p * v), the product rounded, the root correctly rounded
};
FMK_MICRO_FN FmkMicroTerm fmk_micro_term(double p, double pm, double v, double sd)
{
    FmkMicroTerm t;
    t.d = p - pm;
    t.r = fmk_log_host(p / pm);
    t.xk = sd * v;
    t.xa = p * v;
    t.xh = sd * sqrt(t.xa);
    return t;
}

// The nine sums of a bar: Kyle (d on xk), Amihud (|r| on xa), Hasbrouck (r on xh; its Syy is Amihud's: |r| |r| and r r are the same
// float64), and the products d_t d_{t-1}.
struct FmkMicroSums {
    double kxx, kxy, kyy, axx, axy, ryy, hxx, hxy, q;
};
FMK_MICRO_FN void fmk_micro_zero(FmkMicroSums &s) { s.kxx = s.kxy = s.kyy = s.axx = s.axy = s.ryy = s.hxx = s.hxy = s.q = 0.0; }
// one tick's terms onto the sums; dm = the d of the tick before, has_q: that tick has one (the bar's third tick and later)
FMK_MICRO_FN void fmk_micro_add(FmkMicroSums &s, const FmkMicroTerm &t, double dm, bool has_q)
{
    const double ar = fabs(t.r);
    s.kxx += t.xk * t.xk; s.kxy += t.xk * t.d; s.kyy += t.d * t.d;
    s.axx += t.xa * t.xa; s.axy += t.xa * ar; s.ryy += t.r * t.r;
    s.hxx += t.xh * t.xh; s.hxy += t.xh * t.r;
    if (has_q) s.q += t.d * dm;
}

FMK_MICRO_FN bool fmk_micro_finite(double x) { return x - x == 0.0; }

// One regression through the origin over m differences -> slope and its t-value.  The first rule that holds:
//   1. m < 2, a moment that is not finite, or Sxx == 0   -> NaN, NaN
//   2. Syy == 0                                          -> 0.0, 0.0
//   3. u = 1 - Sxy Sxy / (Sxx Syy) <= 2^-26              -> Sxy / Sxx, copysign(inf, Sxy)
//   4. otherwise                                         -> Sxy / Sxx, Sxy / sqrt(Sxx Syy) * sqrt((m - 1) / u)
FMK_MICRO_FN void fmk_micro_regression(int64_t m, double sxx, double sxy, double syy, double &lam, double &tv)
{
    if (m < 2 || !fmk_micro_finite(sxx) || !fmk_micro_finite(sxy) || !fmk_micro_finite(syy) || sxx == 0.0) { lam = NAN; tv = NAN; return; }
    if (syy == 0.0) { lam = 0.0; tv = 0.0; return; }
    lam = sxy / sxx;
    const double den = sxx * syy;
    const double u = 1.0 - sxy * sxy / den;
    if (u <= FMK_MICRO_EXACT_FIT) { tv = copysign(INFINITY, sxy); return; }
    tv = sxy / sqrt(den) * sqrt((double)(m - 1) / u);
}

// Roll: gamma = sum(q) / (m - 1) over the m - 1 products (NaN for m < 2); the spread 2 sqrt(-gamma) where gamma < 0, 0.0 where
// gamma >= 0, NaN where gamma is
FMK_MICRO_FN void fmk_micro_roll(int64_t m, double sq, double &gamma, double &spread)
{
    gamma = m >= 2 ? sq / (double)(m - 1) : NAN;
    spread = gamma < 0.0 ? 2.0 * sqrt(-gamma) : (gamma >= 0.0 ? 0.0 : NAN);
}

// a bar of L ticks (m = L - 1 differences) from its sums -> the eight columns in their order
FMK_MICRO_FN void fmk_micro_finish(int64_t L, const FmkMicroSums &s, double (&o)[FMK_MICRO_COLS])
{
    const int64_t m = L - 1;
    fmk_micro_regression(m, s.kxx, s.kxy, s.kyy, o[0], o[1]);
    fmk_micro_regression(m, s.axx, s.axy, s.ryy, o[2], o[3]);
    fmk_micro_regression(m, s.hxx, s.hxy, s.ryy, o[4], o[5]);
    fmk_micro_roll(m, s.q, o[6], o[7]);
}
