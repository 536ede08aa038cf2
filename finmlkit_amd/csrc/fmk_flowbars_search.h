// fmk_flowbars_search.h -- the plain C++ of the imbalance / run bar indexer (fmk_flowbars.hip): the quantum of an increment, the
// exactness certificate, and the first-exit search over one 512-tick block and over block summaries.  No HIP in here:
// tools/flowbars_check.cpp runs it on the host against the brute-force loops (under ASan / UBSan).
//
// Both rules are one search.  A bar that starts behind tick j closes at the first m > j with
//     U[m] >= U[j] + T   or   V[m] <= V[j] - T
//   imbalance:  U = V = P, the inclusive prefix of x = side * size         (|P[m] - P[j]| >= T)
//   run:        U = Bp, the prefix of the buy sizes; V = -Sp, minus the prefix of the sell sizes   (max(Bp - Bp[j], Sp - Sp[j]) >= T)
// Over an aligned segment the test is "max U >= hi or min V <= lo", and the maxima / minima do not depend on j: a pyramid over
// 8-tick and 64-tick segments per block, (max, min) per block beyond it.  For the run rule U and V are monotone and a segment's
// maximum is its last element; the search does not use that.
//
// Certificate ("Imbalance and run bars"): q = 2^qexp is the lowest set bit over all nonzero increments of the
// tape, so every increment is a multiple of q.  T = ceil(thr / q) q: a multiple of q reaches thr exactly when it reaches T.  If
//     sum |x| + T < 2^53 q
// every partial sum of increments, in any order and over any range, and every U[j] + T, V[j] - T is a multiple of q below 2^53 q:
// representable, so computed without rounding.  A prefix difference then IS the theta of the sequential loop.  The sum itself is
// formed in floating point in an unspecified order; additions of non-negative terms never round downwards past the representable
// bound 2^53 q, so a sum that is really too large is also computed as too large.
#pragma once

#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define FB_HD __host__ __device__ __forceinline__
#else
#define FB_HD static inline
#endif

#define FB_BLOCK 512                    // ticks per block: 64 segments of 8, 8 segments of 64
#define FB_MAX_LS 22                    // table spans beyond 2^22 ticks are refused (as vol_global_tables does)
// 64-block rounds of look-ahead per tick: a link that has not closed within them is longer than 2^22 ticks
#define FB_MAX_ROUNDS (((1 << FB_MAX_LS) / FB_BLOCK) / 64 + 1)

// binary exponent of the lowest set bit of x (x = k 2^e with k odd -> e); INT_MAX for zero.  Meaningless for inf / NaN.
FB_HD int fb_low_bit_exp(double x)
{
    uint64_t b;
    memcpy(&b, &x, 8);
    if ((b << 1) == 0) return INT_MAX;
    const int e = (int)((b >> 52) & 0x7FF);
    const uint64_t m = b & (((uint64_t)1 << 52) - 1);
    if (e == 0) return -1074 + __builtin_ctzll(m);
    return e - 1075 + __builtin_ctzll(m | ((uint64_t)1 << 52));
}

// the size of a tick by kind: 0 one per tick, 1 the amount, 2 price * amount (one rounded float64 product)
FB_HD double fb_size(int kind, double price, double amount) { return kind == 0 ? 1.0 : kind == 1 ? amount : price * amount; }

// -> certified; *T = the threshold rounded up to the tape's quantum.  qexp == INT_MAX: no nonzero increment at all.
FB_HD bool fb_certificate(double sum_abs, int qexp, double thr, double *T)
{
    *T = thr;
    if (!(thr > 0.0 && thr < INFINITY) || !(sum_abs >= 0.0 && sum_abs < INFINITY)) return false;
    if (qexp == INT_MAX) qexp = 0;
    if (qexp < -1074 || qexp > 1023) return false;
    double c = ceil(ldexp(thr, -qexp));                 // thr / q: a power-of-two scaling
    if (c < 1.0) c = 1.0;                               // thr > 0, and an underflow of the scaling must not make T zero
    if (!(c < 9007199254740992.0)) return false;
    *T = ldexp(c, qexp);
    return sum_abs + *T < ldexp(1.0, 53 + qexp);
}

FB_HD bool fb_out(double u, double v, double hi, double lo) { return u >= hi || v <= lo; }

// (max U, min V) over the 64 8-tick and the 8 64-tick segments of one block (the kernel builds the same by lanes)
FB_HD void fb_pyramid(const double *U, const double *V, double *mx8, double *mn8, double *mx64, double *mn64)
{
    for (int s = 0; s < FB_BLOCK / 8; ++s) {
        double a = U[8 * s], b = V[8 * s];
        for (int i = 1; i < 8; ++i) { a = U[8 * s + i] > a ? U[8 * s + i] : a; b = V[8 * s + i] < b ? V[8 * s + i] : b; }
        mx8[s] = a; mn8[s] = b;
    }
    for (int s = 0; s < FB_BLOCK / 64; ++s) {
        double a = mx8[8 * s], b = mn8[8 * s];
        for (int i = 1; i < 8; ++i) { a = mx8[8 * s + i] > a ? mx8[8 * s + i] : a; b = mn8[8 * s + i] < b ? mn8[8 * s + i] : b; }
        mx64[s] = a; mn64[s] = b;
    }
}

// First i in [from, FB_BLOCK) with U[i] >= hi or V[i] <= lo; FB_BLOCK: none.  All FB_BLOCK entries are read: the caller pads a
// short block with its last valid entry (a copy fires only if the original does, which comes first).  Every loop is bounded and
// every index stays inside the arrays whatever the arrays hold; FB_BLOCK + 1: the pyramid contradicts the ticks (garbage input).
FB_HD int fb_first_exit(const double *U, const double *V, const double *mx8, const double *mn8, const double *mx64, const double *mn64,
                        int from, double hi, double lo)
{
    int i = from < 0 ? 0 : from;
    for (; i < FB_BLOCK && (i & 7); ++i)                        // the rest of from's own 8-segment, tick by tick
        if (fb_out(U[i], V[i], hi, lo)) return i;
    bool seg8 = false;
    for (; i < FB_BLOCK && (i & 63); i += 8)                    // aligned 8-segments to the end of the 64-segment
        if (fb_out(mx8[i >> 3], mn8[i >> 3], hi, lo)) { seg8 = true; break; }
    if (!seg8) {
        for (; i < FB_BLOCK; i += 64)                           // 64-segments to the end of the block
            if (fb_out(mx64[i >> 6], mn64[i >> 6], hi, lo)) break;
        if (i >= FB_BLOCK) return FB_BLOCK;
        const int e = i + 64;                                   // descend 64 -> 8
        for (; i < e; i += 8)
            if (fb_out(mx8[i >> 3], mn8[i >> 3], hi, lo)) break;
        if (i >= e) return FB_BLOCK + 1;
    }
    for (int e = i + 8; i < e; ++i)                             // descend 8 -> 1
        if (fb_out(U[i], V[i], hi, lo)) return i;
    return FB_BLOCK + 1;
}

// first of nv block summaries (max U, min V over the block) that a tick with (hi, lo) exits in; nv: none
FB_HD int fb_first_block(const double *smx, const double *smn, int nv, double hi, double lo)
{
    for (int i = 0; i < nv; ++i)
        if (fb_out(smx[i], smn[i], hi, lo)) return i;
    return nv;
}

// One step of the sequential loops that DEFINE the bars, shared by the serial kernel and the host check.  The
// run rule's max(up, dn) >= thr is written as two comparisons: a NaN total never closes, the other side still does.
struct FbState { double theta, up, dn; };
FB_HD bool fb_step(FbState &s, bool run, int side, double size, double thr, bool may_close)
{
    bool close;
    if (!run) {
        s.theta += (double)side * size;
        close = fabs(s.theta) >= thr;
    } else {
        if (side > 0) s.up += size;
        else if (side < 0) s.dn += size;
        close = s.up >= thr || s.dn >= thr;
    }
    close = close && may_close;
    if (close) s.theta = s.up = s.dn = 0.0;
    return close;
}
