// micro_check.cpp -- the plain C++ of the per-bar microstructure features (finmlkit_amd/csrc/fmk_micro_rule.h) on the host: the
// per-tick terms, the four rules of a regression through the origin and the Roll tail, against a long double evaluation.  Fails when
//   - a term is not the rounded float64 operation it is defined as (the difference, the products, the root within half an ulp of
//     the long double value; the logarithm within one ulp of logl of the rounded quotient);
//   - a rule's branch gives another value than written down (NaN / 0.0 / +-inf cases bit for bit, every branch entered);
//   - on random bars (a walk on a price grid, lognormal sizes, sides -1 / 0 / +1, 3 .. 400 ticks) lambda, serial_cov or a t-value
//     leaves the bound that float64 sums of m terms and a float64 evaluation of the rules allow against long double sums of the same
//     terms and a long double evaluation of the rules;
//   - a hand-built bar misses its known answer (d = c xk on dyadic values, alternating and monotone prices, a flat bar, side 0).
//     g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o micro_check tools/micro_check.cpp && ./micro_check
// (any argument: a quick run with fewer random bars)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../finmlkit_amd/csrc/fmk_micro_rule.h"

static long long g_failed, g_bars, g_terms;
static int g_branch[5];                               // regressions that took rule 1, 2, 3 (+inf), 3 (-inf), 4

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            if (g_failed++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                           \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd64()                               // splitmix64
{
    uint64_t x = (g_rng += 0x9E3779B97F4A7C15ULL);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
static double rnd01() { return (double)(rnd64() >> 11) * 0x1p-53; }
static double rndn() { double s = 0.0; for (int k = 0; k < 12; ++k) s += rnd01(); return s - 6.0; }
static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0 || (a != a && b != b); }
static const double EPS = 0x1p-53;

struct Bar { std::vector<double> p, v, sd; };

// the walk of k_micro_lanes over one bar -> the eight columns; the terms' long double sums on the side
struct LdSums { long double kxx, kxy, kyy, axx, axy, ryy, hxx, hxy, q, qabs; };
static void walk(const Bar &b, double (&out)[FMK_MICRO_COLS], LdSums *ld)
{
    FmkMicroSums acc;
    fmk_micro_zero(acc);
    LdSums l = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t L = (int64_t)b.p.size();
    double dm = 0.0;
    for (int64_t i = 1; i < L; ++i) {
        const FmkMicroTerm t = fmk_micro_term(b.p[i], b.p[i - 1], b.v[i], b.sd[i]);
        fmk_micro_add(acc, t, dm, i >= 2);
        l.kxx += (long double)(t.xk * t.xk); l.kxy += (long double)(t.xk * t.d); l.kyy += (long double)(t.d * t.d);
        l.axx += (long double)(t.xa * t.xa); l.axy += (long double)(t.xa * fabs(t.r)); l.ryy += (long double)(t.r * t.r);
        l.hxx += (long double)(t.xh * t.xh); l.hxy += (long double)(t.xh * t.r);
        if (i >= 2) { l.q += (long double)(t.d * dm); l.qabs += fabsl((long double)(t.d * dm)); }
        dm = t.d;
        ++g_terms;
    }
    fmk_micro_finish(L, acc, out);
    if (ld) *ld = l;
    ++g_bars;
}

// the rules in long double -> branch taken (1, 2, 3, 4), lambda, t, u
static int rule_ld(int64_t m, long double sxx, long double sxy, long double syy, long double &lam, long double &tv, long double &u)
{
    lam = tv = u = NAN;
    if (m < 2 || !(sxx - sxx == 0) || !(sxy - sxy == 0) || !(syy - syy == 0) || sxx == 0) return 1;
    if (syy == 0) { lam = tv = 0; return 2; }
    lam = sxy / sxx;
    u = 1 - sxy * sxy / (sxx * syy);
    if (u <= 0x1p-26L) { tv = copysignl(INFINITY, sxy); return 3; }
    tv = sxy / sqrtl(sxx * syy) * sqrtl((long double)(m - 1) / u);
    return 4;
}

static void check_regression(const char *name, int64_t m, long double sxx, long double sxy, long double syy, double lam, double tv,
                             bool hand)
{
    long double wl, wt, u;
    const int br = rule_ld(m, sxx, sxy, syy, wl, wt, u);
    g_branch[br == 3 ? (wt > 0 ? 2 : 3) : (br == 4 ? 4 : br - 1)]++;
    if (br == 1) { CHECK(lam != lam && tv != tv, "%s rule 1: %g %g", name, lam, tv); return; }
    if (br == 2) { CHECK(same_bits(lam, 0.0) && same_bits(tv, 0.0), "%s rule 2: %g %g", name, lam, tv); return; }
    // float64 sums of m terms against the long double ones: DESIGN.md §7m's bound on lambda
    const long double lb = 4.0L * (long double)m * EPS * sqrtl(syy / sxx);
    CHECK(fabsl((long double)lam - wl) <= lb, "%s lambda %.17g want %.17Lg bound %.3Lg", name, lam, wl, lb);
    if (!hand && u > 0 && u < 0x1p-20L) return;       // inside the band around the exact-fit switch: either side is right
    if (br == 3) { CHECK(same_bits(tv, (double)wt), "%s rule 3: t %g want %Lg", name, tv, wt); return; }
    // the moments err by m eps each relative to sqrt(Sxx Syy) -- Sxy, which may cancel, absolutely so -- and u by that over u
    const long double rel = 8.0L * (long double)(m + 4) * EPS * (1.0L + 1.0L / u);
    const long double bound = rel * fabsl(wt) + 4.0L * (long double)m * EPS * sqrtl((long double)(m - 1) / u);
    CHECK(fabsl((long double)tv - wt) <= bound, "%s t %.17g want %.17Lg bound %.3Lg", name, tv, wt, bound);
}

static void check_bar(const Bar &b, bool hand)
{
    double o[FMK_MICRO_COLS];
    LdSums l;
    walk(b, o, &l);
    const int64_t m = (int64_t)b.p.size() - 1;
    check_regression("kyle", m, l.kxx, l.kxy, l.kyy, o[0], o[1], hand);
    check_regression("amihud", m, l.axx, l.axy, l.ryy, o[2], o[3], hand);
    check_regression("hasbrouck", m, l.hxx, l.hxy, l.ryy, o[4], o[5], hand);
    if (m < 2) { CHECK(o[6] != o[6] && o[7] != o[7], "roll of a short bar: %g %g", o[6], o[7]); return; }
    const long double g = l.q / (long double)(m - 1);
    if (g != g) { CHECK(o[6] != o[6] && o[7] != o[7], "roll of a NaN bar: %g %g", o[6], o[7]); return; }
    CHECK(fabsl((long double)o[6] - g) <= 2.0L * (long double)m * EPS * l.qabs / (long double)(m - 1), "serial_cov %.17g want %.17Lg", o[6], g);
    const double want = o[6] < 0.0 ? 2.0 * sqrt(-o[6]) : 0.0;
    CHECK(same_bits(o[7], want), "roll_spread %.17g of serial_cov %.17g", o[7], o[6]);
}

static void check_terms(double p, double pm, double v, double sd)
{
    const FmkMicroTerm t = fmk_micro_term(p, pm, v, sd);
    const long double dl = (long double)p - (long double)pm;
    CHECK(fabsl((long double)t.d - dl) <= fabsl(dl) * EPS, "d(%a, %a) = %a", p, pm, t.d);
    const double qt = p / pm;
    const long double lr = logl((long double)qt);
    CHECK(fabsl((long double)t.r - lr) <= fabsl(lr) * 0x1p-52L + 0x1p-1074L, "log(%a) = %a want %La", qt, t.r, lr);
    CHECK(same_bits(t.xk, sd * v), "xk");
    const long double pa = (long double)p * (long double)v;
    CHECK(fabsl((long double)t.xa - pa) <= fabsl(pa) * EPS, "xa(%a, %a) = %a", p, v, t.xa);
    const long double rt = sqrtl((long double)t.xa);
    if (sd == 0.0) CHECK(t.xh == 0.0, "xh(%a) at side 0 = %a", t.xa, t.xh);
    else CHECK(fabsl((long double)fabs(t.xh) - rt) <= rt * EPS && (t.xh > 0) == (sd > 0), "xh(%a) = %a", t.xa, t.xh);
}

static Bar random_bar(int L, bool f32)
{
    Bar b;
    double p = 100.0 + 900.0 * rnd01();
    const double grid = rnd01() < 0.5 ? 0.01 : 0.5;
    for (int i = 0; i < L; ++i) {
        p += grid * (double)((int)(rnd64() % 7) - 3);
        if (p < 1.0) p = 1.0;
        const double pg = grid * (double)(long long)(p / grid + 0.5);
        double v = exp(0.8 * rndn() - 1.0);
        if (f32) v = (double)(float)v;
        const unsigned s = (unsigned)(rnd64() % 20);
        b.p.push_back(pg); b.v.push_back(v); b.sd.push_back(s == 0 ? 0.0 : (s & 1 ? 1.0 : -1.0));
    }
    return b;
}

static void hand_built()
{
    double o[FMK_MICRO_COLS];
    // d = c xk on dyadic values: lambda == c, t == copysign(inf, c)
    for (double c : {0.25, -0.5}) {
        Bar b;
        double p = 64.0;
        const double vs[] = {1.0, 2.0, 0.5, 4.0, 1.5, 3.0, 2.5, 1.0, 0.75}, ss[] = {1, 1, -1, 1, -1, -1, 1, -1, 1};
        b.p.push_back(p); b.v.push_back(1.0); b.sd.push_back(1.0);
        for (int i = 0; i < 9; ++i) { p += c * ss[i] * vs[i]; b.p.push_back(p); b.v.push_back(vs[i]); b.sd.push_back(ss[i]); }
        walk(b, o, nullptr);
        CHECK(same_bits(o[0], c) && same_bits(o[1], copysign(INFINITY, c)), "exact Kyle fit c = %g: %.17g %g", c, o[0], o[1]);
        check_bar(b, true);
    }
    {   // alternating +-1 price changes: gamma == -1, spread == 2
        Bar b;
        for (int i = 0; i < 40; ++i) { b.p.push_back(100.0 + (i & 1)); b.v.push_back(1.0 + (i % 3)); b.sd.push_back(i % 5 ? 1.0 : -1.0); }
        walk(b, o, nullptr);
        CHECK(same_bits(o[6], -1.0) && same_bits(o[7], 2.0), "alternating: %.17g %.17g", o[6], o[7]);
        check_bar(b, true);
    }
    {   // a monotone ramp: gamma > 0, spread == 0.0
        Bar b;
        for (int i = 0; i < 40; ++i) { b.p.push_back(100.0 + 0.5 * i); b.v.push_back(1.0 + (i % 3)); b.sd.push_back(i % 5 ? 1.0 : -1.0); }
        walk(b, o, nullptr);
        CHECK(o[6] > 0.0 && same_bits(o[7], 0.0), "ramp: %.17g %.17g", o[6], o[7]);
        check_bar(b, true);
    }
    {   // a flat bar: rule 2 everywhere, gamma == 0
        Bar b;
        for (int i = 0; i < 17; ++i) { b.p.push_back(250.0); b.v.push_back(1.0 + (i % 4)); b.sd.push_back(i & 1 ? 1.0 : -1.0); }
        walk(b, o, nullptr);
        for (int k = 0; k < 6; ++k) CHECK(same_bits(o[k], 0.0), "flat bar column %d: %g", k, o[k]);
        CHECK(same_bits(o[6], 0.0) && same_bits(o[7], 0.0), "flat bar roll: %g %g", o[6], o[7]);
        check_bar(b, true);
    }
    {   // all sides 0: rule 1 for Kyle and Hasbrouck, Amihud finite
        Bar b = random_bar(50, false);
        for (auto &s : b.sd) s = 0.0;
        walk(b, o, nullptr);
        CHECK(o[0] != o[0] && o[1] != o[1] && o[4] != o[4] && o[5] != o[5] && o[2] - o[2] == 0.0 && o[3] - o[3] == 0.0,
              "side 0: %g %g %g %g %g %g", o[0], o[1], o[2], o[3], o[4], o[5]);
        check_bar(b, true);
    }
    // bars of 0, 1 and 2 ticks: NaN rows
    for (int L = 0; L <= 2; ++L) {
        Bar b = random_bar(L, false);
        walk(b, o, nullptr);
        for (int k = 0; k < FMK_MICRO_COLS; ++k) CHECK(o[k] != o[k], "%d-tick bar column %d: %g", L, k, o[k]);
    }
    // a bad tick anywhere: exactly the regressions that see it are NaN (rule 1)
    const double bad_p[] = {NAN, 0.0, -5.0};
    for (double bp : bad_p)
        for (int at : {0, 7, 19}) {
            Bar b = random_bar(20, false);
            b.p[at] = bp;
            walk(b, o, nullptr);
            for (int k = 2; k < 6; ++k) CHECK(o[k] != o[k], "price %g at %d column %d: %g", bp, at, k, o[k]);
            check_bar(b, true);
        }
    for (double bv : {(double)INFINITY, (double)NAN})
        for (int at : {1, 7, 19}) {
            Bar b = random_bar(20, false);
            b.v[at] = bv; b.sd[at] = 1.0;
            walk(b, o, nullptr);
            for (int k = 0; k < 6; ++k) CHECK(o[k] != o[k], "amount %g at %d column %d: %g", bv, at, k, o[k]);
            CHECK(o[6] - o[6] == 0.0, "amount %g: serial_cov %g", bv, o[6]);
            check_bar(b, true);
        }
    // the rules on written-out moments, every branch
    double lam, tv;
    fmk_micro_regression(1, 1.0, 1.0, 1.0, lam, tv); CHECK(lam != lam && tv != tv, "m < 2");
    fmk_micro_regression(5, INFINITY, 1.0, 1.0, lam, tv); CHECK(lam != lam && tv != tv, "Sxx inf");
    fmk_micro_regression(5, 1.0, NAN, 1.0, lam, tv); CHECK(lam != lam && tv != tv, "Sxy NaN");
    fmk_micro_regression(5, 1.0, 1.0, INFINITY, lam, tv); CHECK(lam != lam && tv != tv, "Syy inf");
    fmk_micro_regression(5, 0.0, 0.0, 1.0, lam, tv); CHECK(lam != lam && tv != tv, "Sxx == 0");
    fmk_micro_regression(5, 2.0, 0.0, 0.0, lam, tv); CHECK(same_bits(lam, 0.0) && same_bits(tv, 0.0), "Syy == 0");
    fmk_micro_regression(5, 4.0, 2.0, 1.0, lam, tv); CHECK(lam == 0.5 && same_bits(tv, INFINITY), "exact fit +");
    fmk_micro_regression(5, 4.0, -2.0, 1.0, lam, tv); CHECK(lam == -0.5 && same_bits(tv, -INFINITY), "exact fit -");
    fmk_micro_regression(5, 4.0, 2.0, 1.0 + 0x1p-26, lam, tv); CHECK(same_bits(tv, INFINITY), "u just below 2^-26");
    fmk_micro_regression(5, 4.0, 2.0, 1.0 + 0x1p-24, lam, tv); CHECK(tv - tv == 0.0 && tv > 1000.0, "u just above 2^-26: %g", tv);
    fmk_micro_regression(5, 4.0, 1.0, 1.0, lam, tv);          // u = 3/4: t = (1/2) sqrt(4 / (3/4))
    CHECK(lam == 0.25 && fabs(tv - 0.5 * sqrt(16.0 / 3.0)) <= 4 * EPS * tv, "rule 4: %.17g", tv);
    double g, sp;
    fmk_micro_roll(1, 0.0, g, sp); CHECK(g != g && sp != sp, "roll m < 2");
    fmk_micro_roll(5, -16.0, g, sp); CHECK(g == -4.0 && sp == 4.0, "roll negative");
    fmk_micro_roll(5, 16.0, g, sp); CHECK(g == 4.0 && same_bits(sp, 0.0), "roll positive");
    fmk_micro_roll(5, NAN, g, sp); CHECK(g != g && sp != sp, "roll NaN");
}

int main(int argc, char **argv)
{
    const bool quick = argc > 1;
    hand_built();
    const int nbars = quick ? 4000 : 60000;
    for (int k = 0; k < nbars; ++k) {
        const int L = 3 + (int)(rnd64() % (k % 10 == 0 ? 398 : 60));
        check_bar(random_bar(L, (k & 1) != 0), false);
    }
    for (int k = 0; k < (quick ? 20000 : 400000); ++k) {
        const double pm = 1.0 + 4000.0 * rnd01();
        const double p = rnd01() < 0.8 ? pm * (1.0 + 0.002 * rndn()) : 1.0 + 4000.0 * rnd01();
        check_terms(p, pm, exp(2.0 * rndn()), (double)((int)(rnd64() % 3) - 1));
    }
    check_terms(1.0, 1.0, 1.0, 1.0);
    check_terms(5e-324, 1.0, 1e300, -1.0);
    for (int k = 0; k < 5; ++k) CHECK(g_branch[k] > 0, "no regression took branch %d", k);
    printf("bars %lld terms %lld branches %d %d %d %d %d failed checks %lld\n", g_bars, g_terms, g_branch[0], g_branch[1], g_branch[2],
           g_branch[3], g_branch[4], g_failed);
    return g_failed ? 1 : 0;
}
