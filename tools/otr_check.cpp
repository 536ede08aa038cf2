// otr_check.cpp -- the plain C++ of the optimal-trading-rule mesh (finmlkit_amd/csrc/fmk_otr_rule.h, with fmk_log.h) on the host.
//   otr_check [quick]
//     the record walk the kernel makes (one walk of a path for the whole mesh: fmk_otr_cross, fmk_otr_kind) against the book's loop
//     per node (snippet 13.2: the first step with P > pt or P < -sl, else the last) -- exit step, value and kind of every node on
//     every path, over parameter sets with and without mean reversion, sigma = 0, odd and single-step horizons, meshes with a
//     repeated level, a zero level and an infinite one; and the early stop never ends a path a node still needs.  Fails when they
//     differ, when a uniform leaves [-1, 1), or when the pairs' moments are off.
//   otr_check mesh n_paths max_hp seed forecast phi sigma n_pt n_sl pt.. sl..
//     one parameter set's mesh by the record walk on one thread, in the definition's summing order (the one-thread yardstick of
//     tools/otrbench.py, and the rule text's side of tests/test_otr_host.py): "node i j mean std sharpe n_profit n_stop n_time hold"
//     with the float64 as hex, then "steps <path steps walked> seconds <wall time>".
//     g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o otr_check tools/otr_check.cpp && ./otr_check
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../finmlkit_amd/csrc/fmk_otr_rule.h"

static long long g_failed, g_paths, g_nodes, g_early;

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            if (g_failed++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                           \
    } while (0)

struct Records {
    std::vector<uint32_t> step;
    std::vector<double> val;
    double last;
    int steps_walked;
};

// one path by the record walk, as a lane of k_otr_walk makes it
static void walk(uint64_t seed, uint64_t p, double forecast, double phi, double sigma, const std::vector<double> &pt,
                 const std::vector<double> &sl, int max_hp, Records &r)
{
    const int n_pt = (int)pt.size(), n_sl = (int)sl.size();
    r.step.assign((size_t)(n_pt + n_sl), FMK_OTR_NONE);
    r.val.assign((size_t)(n_pt + n_sl), 0.0);
    auto rec = [&](int k, uint32_t h, double P) { r.step[(size_t)k] = h; r.val[(size_t)k] = P; };
    const double c0 = fmk_otr_c0(forecast, phi);
    double P = 0.0;
    int ip = 0, is = 0, h = 1;
    for (; h <= max_hp; h += 2) {
        double z0, z1;
        (void)fmk_otr_pair(seed, p, (uint32_t)((h - 1) >> 1), &z0, &z1);
        P = fmk_otr_step(c0, phi, sigma, P, z0);
        fmk_otr_cross(P, (uint32_t)h, pt.data(), n_pt, sl.data(), n_sl, &ip, &is, rec);
        if (fmk_otr_done(ip, n_pt, is, n_sl) || h == max_hp) break;
        P = fmk_otr_step(c0, phi, sigma, P, z1);
        fmk_otr_cross(P, (uint32_t)(h + 1), pt.data(), n_pt, sl.data(), n_sl, &ip, &is, rec);
        if (fmk_otr_done(ip, n_pt, is, n_sl)) { ++h; break; }
    }
    r.last = P;
    r.steps_walked = h < max_hp ? h : max_hp;
}

// the whole path, for the book's loop
static void whole_path(uint64_t seed, uint64_t p, double forecast, double phi, double sigma, int max_hp, std::vector<double> &P)
{
    const double c0 = fmk_otr_c0(forecast, phi);
    P.assign((size_t)max_hp, 0.0);
    double cur = 0.0;
    for (int h = 1; h <= max_hp; ++h) {
        double z0, z1;
        (void)fmk_otr_pair(seed, p, (uint32_t)((h - 1) >> 1), &z0, &z1);
        cur = fmk_otr_step(c0, phi, sigma, cur, ((h - 1) & 1) ? z1 : z0);
        P[(size_t)(h - 1)] = cur;
    }
}

static void check_case(const char *what, uint64_t seed, int n_paths, double forecast, double phi, double sigma,
                       const std::vector<double> &pt, const std::vector<double> &sl, int max_hp)
{
    Records r;
    std::vector<double> P;
    for (int p = 0; p < n_paths; ++p) {
        walk(seed, (uint64_t)p, forecast, phi, sigma, pt, sl, max_hp, r);
        whole_path(seed, (uint64_t)p, forecast, phi, sigma, max_hp, P);
        g_early += r.steps_walked < max_hp;
        ++g_paths;
        for (size_t i = 0; i < pt.size(); ++i)
            for (size_t j = 0; j < sl.size(); ++j) {
                int h = max_hp, kind = FMK_OTR_TIME;                  // snippet 13.2
                for (int t = 1; t <= max_hp; ++t) {
                    const double cp = P[(size_t)(t - 1)];
                    if (cp > pt[i]) { h = t; kind = FMK_OTR_PROFIT; break; }
                    if (cp < -sl[j]) { h = t; kind = FMK_OTR_STOP; break; }
                }
                const double x = P[(size_t)(h - 1)];
                const uint32_t hp = r.step[i], hs = r.step[pt.size() + j];
                const int k2 = fmk_otr_kind(hp, hs);
                const uint32_t h2 = fmk_otr_exit_step(k2, hp, hs, (uint32_t)max_hp);
                const double x2 = k2 == FMK_OTR_PROFIT ? r.val[i] : k2 == FMK_OTR_STOP ? r.val[pt.size() + j] : r.last;
                ++g_nodes;
                CHECK(k2 == kind && (int)h2 == h && memcmp(&x, &x2, 8) == 0, "%s path %d node %zu %zu: loop (%d %d %a) walk (%d %u %a)", what, p,
                      i, j, kind, h, x, k2, h2, x2);
            }
    }
}

static void check_generator(int n_pairs)
{
    double s1 = 0, s2 = 0, s4 = 0;
    long long first = 0;
    for (int p = 0; p < n_pairs; ++p) {
        double z[2];
        const int a = fmk_otr_pair(7, (uint64_t)p, (uint32_t)(p & 2047), &z[0], &z[1]);
        first += a == 1;
        for (double v : z) { s1 += v; s2 += v * v; s4 += v * v * v * v; }
        const double u = fmk_otr_uniform(fmk_sb_word(7, fmk_otr_index((uint64_t)p, 0, 0, 0)));
        CHECK(u >= -1.0 && u < 1.0, "uniform %a", u);
    }
    const double n = 2.0 * n_pairs, mean = s1 / n, var = s2 / n - mean * mean, kurt = s4 / n / (var * var);
    CHECK(fabs(mean) < 6.0 / sqrt(n), "mean %g", mean);
    CHECK(fabs(var - 1.0) < 6.0 * sqrt(2.0 / n), "variance %g", var);
    CHECK(fabs(kurt - 3.0) < 6.0 * sqrt(24.0 / n), "kurtosis %g", kurt);
    CHECK(fabs((double)first / n_pairs - M_PI / 4) < 6.0 * sqrt(M_PI / 4 * (1 - M_PI / 4) / n_pairs), "accepted at once %lld of %d", first, n_pairs);
    CHECK(fmk_otr_uniform(0) == -1.0 && fmk_otr_uniform(~0ull) == 1.0 - 0x1p-52, "the ends of the uniform");
    CHECK(fmk_otr_index(0xFFFFFFFFull, 2047, 63, 1) == ((((0xFFFFFFFFull << 12) | 2047) << 6 | 63) << 1 | 1), "index");
}

static int run_mesh(int argc, char **argv)
{
    if (argc < 10) { fprintf(stderr, "mesh: too few arguments\n"); return 2; }
    const long long n_paths = atoll(argv[2]);
    const int max_hp = atoi(argv[3]);
    const uint64_t seed = strtoull(argv[4], nullptr, 0);
    const double forecast = strtod(argv[5], nullptr), phi = strtod(argv[6], nullptr), sigma = strtod(argv[7], nullptr);
    const int n_pt = atoi(argv[8]), n_sl = atoi(argv[9]);
    if (n_pt < 1 || n_sl < 1 || n_pt > FMK_OTR_MAX_LEVELS || n_sl > FMK_OTR_MAX_LEVELS || argc != 10 + n_pt + n_sl || n_paths < 1 ||
        max_hp < 1 || max_hp > FMK_OTR_MAX_HP) {
        fprintf(stderr, "mesh: bad arguments\n");
        return 2;
    }
    std::vector<double> pt, sl;
    for (int i = 0; i < n_pt; ++i) pt.push_back(strtod(argv[10 + i], nullptr));
    for (int j = 0; j < n_sl; ++j) sl.push_back(strtod(argv[10 + n_pt + j], nullptr));
    const size_t nodes = (size_t)n_pt * n_sl;
    std::vector<double> S1(nodes, 0.0), S2(nodes, 0.0), b1(nodes), b2(nodes);
    std::vector<long long> np(nodes, 0), ns(nodes, 0), hold(nodes, 0);
    long long steps = 0;
    Records r;
    const auto t0 = std::chrono::steady_clock::now();
    for (long long p0 = 0; p0 < n_paths; p0 += FMK_OTR_BLOCK) {
        std::fill(b1.begin(), b1.end(), 0.0);
        std::fill(b2.begin(), b2.end(), 0.0);
        for (long long p = p0; p < p0 + FMK_OTR_BLOCK && p < n_paths; ++p) {
            walk(seed, (uint64_t)p, forecast, phi, sigma, pt, sl, max_hp, r);
            steps += r.steps_walked;
            for (int i = 0; i < n_pt; ++i)
                for (int j = 0; j < n_sl; ++j) {
                    const size_t k = (size_t)i * n_sl + j;
                    const uint32_t hp = r.step[(size_t)i], hs = r.step[(size_t)(n_pt + j)];
                    const int kind = fmk_otr_kind(hp, hs);
                    const double x = kind == FMK_OTR_PROFIT ? r.val[(size_t)i] : kind == FMK_OTR_STOP ? r.val[(size_t)(n_pt + j)] : r.last;
                    fmk_otr_add(x, &b1[k], &b2[k]);
                    np[k] += kind == FMK_OTR_PROFIT;
                    ns[k] += kind == FMK_OTR_STOP;
                    hold[k] += fmk_otr_exit_step(kind, hp, hs, (uint32_t)max_hp);
                }
        }
        for (size_t k = 0; k < nodes; ++k) { S1[k] = S1[k] + b1[k]; S2[k] = S2[k] + b2[k]; }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < n_pt; ++i)
        for (int j = 0; j < n_sl; ++j) {
            const size_t k = (size_t)i * n_sl + j;
            double mean, sd, sharpe;
            fmk_otr_stats(S1[k], S2[k], (double)n_paths, &mean, &sd, &sharpe);
            printf("node %d %d %a %a %a %lld %lld %lld %lld\n", i, j, mean, sd, sharpe, np[k], ns[k], n_paths - np[k] - ns[k], hold[k]);
        }
    printf("steps %lld seconds %.6f\n", steps, sec);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "mesh") == 0) return run_mesh(argc, argv);
    const bool quick = argc > 1;
    const int n = quick ? 600 : 6000;
    const double inf = INFINITY;
    const std::vector<double> five = {0.5, 1.0, 1.5, 2.0, 2.5}, rep = {0.0, 0.75, 0.75, 3.0, inf}, one = {1.0}, off = {inf};
    std::vector<double> wide;
    for (int i = 0; i < 32; ++i) wide.push_back(0.125 * i);
    check_case("mean reverting", 1, n, 0.0, exp2(-1.0 / 5.0), 1.0, five, five, 24);
    check_case("drift", 2, n, 1.5, exp2(-1.0 / 10.0), 0.75, five, rep, 25);
    check_case("random walk", 3, n, 0.0, 1.0, 1.0, rep, five, 24);
    check_case("no memory", 4, n, -0.5, 0.0, 2.0, rep, rep, 7);
    check_case("one step", 5, n, 0.0, 0.5, 1.0, five, five, 1);
    check_case("two steps", 6, n, 0.0, 0.5, 1.0, one, rep, 2);
    check_case("no noise", 7, n / 10, 2.0, 0.5, 0.0, five, five, 12);
    check_case("constant", 8, n / 10, 0.0, 0.5, 0.0, rep, rep, 5);
    check_case("barriers off", 9, n, 0.0, 0.9, 1.0, off, off, 16);
    check_case("one side off", 10, n, 0.0, 0.9, 1.0, off, five, 16);
    check_case("32 x 32", 11, n / 4, 0.25, 0.95, 0.5, wide, wide, 40);
    check_generator(quick ? 40000 : 400000);
    CHECK(g_early > 0, "no path stopped early");
    printf("paths %lld nodes %lld early %lld\n", g_paths, g_nodes, g_early);
    printf("failed checks %lld\n", g_failed);
    return g_failed ? 1 : 0;
}
