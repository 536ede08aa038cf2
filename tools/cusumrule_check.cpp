// Host check of the two per-tick CUSUM rules of finmlkit_amd/csrc/fmk_cusum_rule.h (cs_tick: the bar indexer, cf_tick: the event
// filter), which the kernels run as selects:  g++ -O2 -std=c++17 tools/cusumrule_check.cpp -o cusumrule_check && ./cusumrule_check
// Each is compared with the branching form written in the order of the reference loop -- finmlkit/bar/logic.py:199-219 as restated in
// oracle/fmk_oracle.c (orc_cusum_bar_indexer), finmlkit/sampling/filters.py:7-70 as restated in tests/_filter_ref.py -- on
//   * the cross product of special values for both states, the return and the threshold: +-0.0, subnormals, the smallest normal,
//     ordinary magnitudes, DBL_MAX, +-inf, NaN (negative thresholds included), and for every (state, return) also the four thresholds
//     that make an exact tie: s_pos == lam, s_neg == -lam and their negatives; the bar rule also with the tick inside a same-timestamp
//     block (the kernels pass a NaN threshold for "cannot close");
//   * 1 000 000 seeded random (s_pos, s_neg, return) triples, a third of them with a tie threshold.
// s_pos, s_neg and the fired bit must be equal bit for bit.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../finmlkit_amd/csrc/fmk_cusum_rule.h"

// max(0.0, v) / min(0.0, v) of the reference loops: the first argument stays unless the second is greater / smaller (a NaN never is)
static double ref_max0(double v) { double m = 0.0; if (v > m) m = v; return m; }
static double ref_min0(double v) { double m = 0.0; if (v < m) m = v; return m; }

// logic.py:199-219: clamp both sides; a tick followed by one of the same timestamp cannot close; else the positive side, elif the negative
static unsigned ref_bar(double &s_pos, double &s_neg, double ret, bool block, double lam)
{
    s_pos = ref_max0(s_pos + ret);
    s_neg = ref_min0(s_neg + ret);
    if (block) return 0;
    if (s_pos >= lam) { s_pos = 0.0; return 1; }
    else if (s_neg <= -lam) { s_neg = 0.0; return 1; }
    return 0;
}

// filters.py:7-70: the negative side first, strict comparisons
static unsigned ref_filter(double &s_pos, double &s_neg, double ret, double thr)
{
    s_pos = ref_max0(s_pos + ret);
    s_neg = ref_min0(s_neg + ret);
    if (s_neg < -thr) { s_neg = 0.0; return 1; }
    else if (s_pos > thr) { s_pos = 0.0; return 1; }
    return 0;
}

static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

static long checked = 0, failed = 0;

static void check(double sp, double sn, double r, double lam)
{
    for (int block = 0; block < 2; ++block) {
        double a = sp, b = sn, c = sp, d = sn;
        const unsigned want = ref_bar(a, b, r, block != 0, lam);
        const unsigned got = cs_tick(c, d, r, block ? (double)NAN : lam);
        ++checked;
        if (want != got || bits(a) != bits(c) || bits(b) != bits(d)) ++failed;
    }
    double a = sp, b = sn, c = sp, d = sn;
    const unsigned want = ref_filter(a, b, r, lam);
    const unsigned got = cf_tick(c, d, r, lam);
    ++checked;
    if (want != got || bits(a) != bits(c) || bits(b) != bits(d)) ++failed;
}

// the thresholds at which (sp, sn, r) is an exact tie on either side, and their negatives
static void check_ties(double sp, double sn, double r)
{
    const double p = ref_max0(sp + r), q = ref_min0(sn + r);
    check(sp, sn, r, p);
    check(sp, sn, r, -q);
    check(sp, sn, r, -p);
    check(sp, sn, r, q);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rng()
{
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ULL);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
static double uni() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
    const double pos[] = {0.0, den, 1000 * den, DBL_MIN, 1e-300, 2e-4, 2e-3, 1.0, DBL_MAX, inf};
    double v[2 * 10 + 1];
    int nv = 0;
    for (double x : pos) { v[nv++] = x; v[nv++] = -x; }
    v[nv++] = NAN;
    for (int i = 0; i < nv; ++i)
        for (int j = 0; j < nv; ++j)
            for (int k = 0; k < nv; ++k) {
                for (int l = 0; l < nv; ++l) check(v[i], v[j], v[k], v[l]);
                check_ties(v[i], v[j], v[k]);
            }
    for (int it = 0; it < 1000000; ++it) {
        // states as the walks hold them (s_pos >= 0 >= s_neg, often exactly 0.0), returns of a tick, thresholds of both regimes
        const double scale = (rng() & 1) ? 2e-3 : 2.0;
        const double sp = (rng() & 3) == 0 ? 0.0 : uni() * scale, sn = (rng() & 3) == 0 ? 0.0 : -uni() * scale;
        const double r = (uni() - 0.5) * scale;
        if (it % 3 == 0) check_ties(sp, sn, r);
        else check(sp, sn, r, (rng() & 15) == 0 ? -uni() * scale : uni() * scale);
    }
    printf("cusum rules checked: %ld, failed checks: %ld\n", checked, failed);
    return failed != 0;
}
