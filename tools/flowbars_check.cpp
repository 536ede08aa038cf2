// flowbars_check.cpp -- the plain C++ of the imbalance / run bar indexer (finmlkit_amd/csrc/fmk_flowbars_search.h) on the host: the
// quantum of an increment, the certificate, the first-exit search over (prefix, pyramid, block summaries) for both rules.  Random
// tapes -- sides -1 / 0 / +1, dyadic sizes, stretches of side 0, one-sided stretches, lengths that end inside an 8-segment, a
// 64-segment and a block -- are taken through the steps of the kernels (block-local prefixes, bases, absolute (max, min) per
// block, the pyramid of the tick's own block, summaries 64 at a time, the pyramid of the block that fires).  Fails when
//   - a link nxt(j), or the first close, differs from the sequential loop (fb_step) started behind tick j;
//   - a tape of dyadic sizes does not certify, or one whose sums cannot be exact (2^-40 beside 2^20) does;
//   - the threshold rounded up to the quantum decides differently from the threshold on a multiple of the quantum;
//   - fb_low_bit_exp disagrees with frexp-by-division on random doubles.
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o flowbars_check tools/flowbars_check.cpp && ./flowbars_check
// (any argument: a quick run without the two long tapes per rule)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../finmlkit_amd/csrc/fmk_flowbars_search.h"

static long long g_links, g_tapes, g_failed;

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
static uint32_t rnd(uint32_t below) { return (uint32_t)((rnd64() >> 33) % below); }

struct Tape {
    bool run;
    int64_t n;
    double thr;
    std::vector<int> side;
    std::vector<double> size;
};

// the sequential loop from a fresh state behind tick j (j = -1: from tick 0, which cannot close) -> close or -1
static int64_t brute(const Tape &t, int64_t j)
{
    FbState s = {0.0, 0.0, 0.0};
    for (int64_t i = j + 1; i < t.n; ++i)
        if (fb_step(s, t.run, t.side[i], t.size[i], t.thr, i > 0)) return i;
    return -1;
}

struct Blocks {                                       // what k_fb_prefix and k_fb_scan leave
    int64_t nblk;
    std::vector<double> LU, LV, baseU, baseV, gmx, gmn;
    double sum_abs;
    int qexp;
};

static Blocks prefix_pass(const Tape &t)
{
    Blocks b;
    b.nblk = (t.n + FB_BLOCK - 1) / FB_BLOCK;
    b.LU.assign(t.n, 0.0); b.LV.assign(t.n, 0.0);
    b.baseU.assign(b.nblk, 0.0); b.baseV.assign(b.nblk, 0.0); b.gmx.assign(b.nblk, 0.0); b.gmn.assign(b.nblk, 0.0);
    b.sum_abs = 0.0;
    b.qexp = INT_MAX;
    double bu = 0.0, bv = 0.0;
    for (int64_t k = 0; k < b.nblk; ++k) {
        double u = 0.0, v = 0.0, mx = -INFINITY, mn = INFINITY;
        for (int64_t i = k * FB_BLOCK; i < t.n && i < (k + 1) * FB_BLOCK; ++i) {
            double xu, xv = 0.0;
            if (t.run) { xu = t.side[i] > 0 ? t.size[i] : 0.0; xv = t.side[i] < 0 ? -t.size[i] : 0.0; }
            else xu = (double)t.side[i] * t.size[i];
            const int e1 = fb_low_bit_exp(xu), e2 = fb_low_bit_exp(xv);
            b.qexp = e1 < b.qexp ? e1 : b.qexp;
            b.qexp = e2 < b.qexp ? e2 : b.qexp;
            b.sum_abs += fabs(xu) + fabs(xv);
            u += xu;
            v = t.run ? v + xv : u;
            b.LU[i] = u; b.LV[i] = v;
            mx = u > mx ? u : mx;
            mn = v < mn ? v : mn;
        }
        b.baseU[k] = bu; b.baseV[k] = t.run ? bv : bu;
        b.gmx[k] = bu + mx;
        b.gmn[k] = (t.run ? bv : bu) + mn;
        bu += u;
        bv += v;
    }
    return b;
}

struct Tile { double U[FB_BLOCK], V[FB_BLOCK], mx8[FB_BLOCK / 8], mn8[FB_BLOCK / 8], mx64[FB_BLOCK / 64], mn64[FB_BLOCK / 64]; };

static int stage(Tile &tl, const Tape &t, const Blocks &b, int64_t blk)   // fb_stage of the kernel
{
    const int64_t ds = blk * FB_BLOCK;
    const int nv = (int)(t.n - ds < FB_BLOCK ? t.n - ds : FB_BLOCK);
    for (int i = 0; i < FB_BLOCK; ++i) {
        const int src = i < nv ? i : nv - 1;
        tl.U[i] = b.baseU[blk] + b.LU[ds + src];
        tl.V[i] = b.baseV[blk] + b.LV[ds + src];
    }
    fb_pyramid(tl.U, tl.V, tl.mx8, tl.mn8, tl.mx64, tl.mn64);
    return nv;
}

// the search of k_fb_links / k_fb_root for one tick (j = -1: the root) -> close, -1 none, -2 inconsistent
static int64_t link(const Tape &t, const Blocks &b, double T, int64_t j)
{
    Tile tl;
    const int64_t blk = j < 0 ? 0 : j / FB_BLOCK;
    int nv = stage(tl, t, b, blk);
    const int jl = (int)(j - blk * FB_BLOCK);
    const double hi = (j < 0 ? 0.0 : tl.U[jl]) + T, lo = (j < 0 ? 0.0 : tl.V[jl]) - T;
    int r = fb_first_exit(tl.U, tl.V, tl.mx8, tl.mn8, tl.mx64, tl.mn64, j < 0 ? 1 : jl + 1, hi, lo);
    if (r < nv) return blk * FB_BLOCK + r;
    for (int64_t b0 = blk + 1; b0 < b.nblk; b0 += 64) {
        const int nvb = (int)(b.nblk - b0 < 64 ? b.nblk - b0 : 64);
        const int i = fb_first_block(b.gmx.data() + b0, b.gmn.data() + b0, nvb, hi, lo);
        if (i == nvb) continue;
        nv = stage(tl, t, b, b0 + i);
        r = fb_first_exit(tl.U, tl.V, tl.mx8, tl.mn8, tl.mx64, tl.mn64, 0, hi, lo);
        return r < nv ? (b0 + i) * FB_BLOCK + r : -2;
    }
    return -1;
}

static void run_tape(bool run, int64_t n, double thr, int unit_log2, int max_lots, int flavour)
{
    Tape t;
    t.run = run; t.n = n; t.thr = thr;
    t.side.resize(n); t.size.resize(n);
    const double unit = ldexp(1.0, -unit_log2);
    int64_t quiet_to = -1, oneside_to = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (flavour == 1 && rnd(700) == 0) quiet_to = i + rnd(1500);          // stretches of side 0
        if (flavour == 2 && rnd(900) == 0) oneside_to = i + rnd(300);         // one-sided stretches: closes every few ticks
        t.side[i] = i < quiet_to ? 0 : i < oneside_to ? 1 : (int)rnd(3) - 1;
        if (flavour == 3) t.side[i] = rnd(2) ? 1 : -1;
        t.size[i] = unit * (double)(1 + rnd((uint32_t)max_lots));
    }
    const Blocks b = prefix_pass(t);
    double T;
    const bool cert = fb_certificate(b.sum_abs, b.qexp, thr, &T);
    CHECK(cert, "dyadic tape n %lld unit 2^-%d does not certify", (long long)n, unit_log2);
    if (!cert) return;
    CHECK(T >= thr && T - thr < ldexp(1.0, b.qexp == INT_MAX ? 0 : b.qexp), "T %g thr %g", T, thr);
    ++g_tapes;
    for (int64_t j = -1; j < n; ++j) {
        const int64_t want = brute(t, j), got = link(t, b, T, j);
        CHECK(want == got, "%s n %lld thr %g flavour %d: link of tick %lld is %lld, the loop closes at %lld", run ? "run" : "imbalance",
              (long long)n, thr, flavour, (long long)j, (long long)got, (long long)want);
        ++g_links;
    }
}

static void check_low_bit()
{
    for (int it = 0; it < 200000; ++it) {
        uint64_t bits = rnd64();
        if (it % 3 == 0) bits &= ~(((uint64_t)1 << rnd(52)) - 1);             // trailing zeros
        if (it % 7 == 0) bits &= ~((uint64_t)0x7FF << 52);                    // subnormals
        double x;
        memcpy(&x, &bits, 8);
        if (!(x - x == 0.0)) continue;
        const int e = fb_low_bit_exp(x);
        if (x == 0.0) { CHECK(e == INT_MAX, "zero"); continue; }
        // x / 2^e is an odd integer
        const double k = ldexp(x, -e);
        CHECK(k == floor(k) && fmod(fabs(k), 2.0) == 1.0, "x %a e %d", x, e);
    }
}

static void check_certificate()
{
    double T;
    // 2^20 lots of 2^20 and one of 2^-40: the quantum is 2^-40 and the sum needs 80 bits
    CHECK(!fb_certificate(ldexp(1.0, 40) + ldexp(1.0, -40), -40, 8.0, &T), "inexact sums certified");
    CHECK(fb_certificate(ldexp(1.0, 20), -6, 8.0, &T) && T == 8.0, "dyadic lots");
    CHECK(fb_certificate(1000.0, 0, 16.5, &T) && T == 17.0, "tick kind, fractional threshold: T %g", T);
    CHECK(fb_certificate(0.0, INT_MAX, 3.0, &T) && T == 3.0, "no increments");
    CHECK(!fb_certificate(1.0, 0, 0.0, &T) && !fb_certificate(1.0, 0, -1.0, &T) && !fb_certificate(1.0, 0, NAN, &T) &&
          !fb_certificate(1.0, 0, INFINITY, &T), "thresholds outside (0, inf)");
    CHECK(!fb_certificate(INFINITY, 0, 1.0, &T) && !fb_certificate(NAN, 0, 1.0, &T), "sum");
    CHECK(fb_certificate(ldexp(1.0, 52), 0, 1.0, &T) && !fb_certificate(ldexp(1.0, 53), 0, 1.0, &T), "the 2^53 q bound");
    CHECK(fb_certificate(ldexp(1.0, -1060), -1074, 1e-320, &T) && T >= 1e-320, "subnormal quantum");
    CHECK(fb_certificate(8.0, 3, 1e-300, &T) && T == 8.0, "threshold far below the quantum: T %g", T);
    // rounding the threshold up to the quantum keeps every decision on multiples of the quantum
    for (int it = 0; it < 100000; ++it) {
        const int qe = (int)rnd(40) - 20;
        const double thr = ldexp((double)(1 + rnd(1 << 20)) + (double)rnd(1000) / 1000.0, qe - (int)rnd(4));
        if (!fb_certificate(0.0, qe, thr, &T)) continue;
        const double below = T - ldexp(1.0, qe);
        CHECK(T >= thr && below < thr, "qe %d thr %a T %a", qe, thr, T);
    }
}

int main(int argc, char **)
{
    const bool quick = argc > 1;                      // any argument: without the two long tapes per rule (the test suite's run)
    check_low_bit();
    check_certificate();
    for (int run = 0; run < 2; ++run) {
        // lengths at which the 8-segment, the 64-segment and the block end; several blocks; more than 64 blocks (two summary loads)
        for (int64_t n : {1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2500})
            for (int flavour = 0; flavour < 4; ++flavour) {
                run_tape(run != 0, n, 8.0, 6, 64, flavour);
                run_tape(run != 0, n, 3.0, 0, 1, flavour);                    // tick-sized: ties at the threshold
                run_tape(run != 0, n, 100.25, 3, 40, flavour);                // a threshold off the quantum
            }
        if (quick) continue;
        run_tape(run != 0, 66 * FB_BLOCK + 17, run ? 3000.0 : 60.0, 0, 1, 3); // bars of thousands of ticks
        run_tape(run != 0, 65 * FB_BLOCK + 3, 1e9, 0, 1, 0);                  // never closes: every link runs to the end of the summaries
    }
    printf("tapes %lld, links compared %lld, failed checks %lld\n", g_tapes, g_links, g_failed);
    return g_failed ? 1 : 0;
}
