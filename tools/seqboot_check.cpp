// seqboot_check.cpp -- the sequential bootstrap on the host, from the plain C++ of
// finmlkit_amd/csrc/fmk_seqboot_rule.h: the per-position brute force (one concurrency count per position of the axis) and the
// compressed form (one per interval between span boundaries, the form the kernel runs).
//   cases on stdin -> the draws and Q of every case on stdout.  A case is whitespace-separated integers:
//       m n K R seed n_words   then m pairs  event touch   then n_words words (0, or R * K of them)
//     answered by two lines, "draws ..." and "q ...", run-major, from the compressed form; where n <= 2^20 the brute force runs too
//     and has to agree.  First argument "time": the compressed form alone, and a line "time_s <seconds>" in front of each answer
//     (the host yardstick of tools/seqbootbench.py, one thread).
//   no input (stdin empty or a terminal) -> self check: brute force == compressed on random cases; fmk_sb_q == S / L on random and
//     extreme operands; and at n = 2^32, with a span over the whole axis drawn again and again beside short ones, every S, Q and T
//     equal to their 128-bit evaluation and inside the bounds the definition promises (S <= L * 2^30 <= 2^62, T <= m * 2^30, Q > 0).
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o seqboot_check tools/seqboot_check.cpp && ./seqboot_check < /dev/null
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <vector>

#include "../finmlkit_amd/csrc/fmk_seqboot_rule.h"

typedef unsigned __int128 u128;
static long long g_failed;

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            if (g_failed++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                           \
    } while (0)

struct Case {
    int64_t m, n, K, R;
    uint64_t seed;
    std::vector<int64_t> ev, touch;
    std::vector<uint64_t> words;
};
struct Result { std::vector<int64_t> draws, q; };

static uint64_t word_of(const Case &c, int64_t r, int64_t k)
{
    const uint64_t idx = (uint64_t)r * (uint64_t)c.K + (uint64_t)k;
    return c.words.empty() ? fmk_sb_word(c.seed, idx) : c.words[idx];
}

// the smallest i with Q_0 + .. + Q_i > target
static int64_t pick(const std::vector<uint64_t> &Q, uint64_t word)
{
    uint64_t T = 0;
    for (uint64_t q : Q) T += q;
    const uint64_t target = fmk_sb_target(word, T);
    uint64_t acc = 0;
    for (size_t i = 0; i < Q.size(); ++i) {
        acc += Q[i];
        if (acc > target) return (int64_t)i;
    }
    return -1;
}

static Result brute(const Case &c)
{
    Result out;
    std::vector<uint32_t> cnt((size_t)c.n);
    std::vector<uint64_t> Q((size_t)c.m);
    for (int64_t r = 0; r < c.R; ++r) {
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (int64_t k = 0; k < c.K; ++k) {
            for (int64_t i = 0; i < c.m; ++i) {
                uint64_t S = 0;
                for (int64_t t = c.ev[i]; t <= c.touch[i]; ++t) S += fmk_sb_w(cnt[(size_t)t]);
                Q[(size_t)i] = S / (uint64_t)(c.touch[i] - c.ev[i] + 1);
            }
            const int64_t i = pick(Q, word_of(c, r, k));
            out.draws.push_back(i);
            out.q.push_back(i < 0 ? -1 : (int64_t)Q[(size_t)i]);
            if (i < 0) return out;
            for (int64_t t = c.ev[i]; t <= c.touch[i]; ++t) cnt[(size_t)t] += 1;
        }
    }
    return out;
}

// verify: every S, Q and T against a 128-bit evaluation and the definition's bounds
static Result compressed(const Case &c, bool verify)
{
    Result out;
    std::vector<uint32_t> len_m1;
    std::vector<FmkSbEvent> events;
    fmk_sb_compress(c.ev.data(), c.touch.data(), c.m, len_m1, events);
    const size_t J = len_m1.size();
    std::vector<uint32_t> cnt(J);
    std::vector<uint64_t> P(J + 1), Q((size_t)c.m);
    for (int64_t r = 0; r < c.R; ++r) {
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (int64_t k = 0; k < c.K; ++k) {
            uint64_t s = 0;
            u128 s128 = 0;
            for (size_t j = 0; j < J; ++j) {
                P[j] = s;
                s += ((uint64_t)len_m1[j] + 1u) * fmk_sb_w(cnt[j]);
                if (verify) s128 += (u128)((uint64_t)len_m1[j] + 1u) * fmk_sb_w(cnt[j]);
            }
            P[J] = s;
            if (verify) CHECK(s128 == (u128)s && s <= (uint64_t)c.n << 30, "the prefix left 64 bits");
            u128 T128 = 0;
            for (int64_t i = 0; i < c.m; ++i) {
                const FmkSbEvent e = events[(size_t)i];
                const uint64_t L = (uint64_t)e.len_m1 + 1u, S = P[e.hi] - P[e.lo];
                Q[(size_t)i] = fmk_sb_q(S, L);
                if (verify) {
                    CHECK(L == (uint64_t)(c.touch[i] - c.ev[i] + 1), "event %lld: L", (long long)i);
                    CHECK(S <= L << 30 && S >= L * 64u, "event %lld: S = %llu outside [64 L, 2^30 L]", (long long)i, (unsigned long long)S);
                    CHECK(Q[(size_t)i] == S / L && Q[(size_t)i] >= 64u && Q[(size_t)i] <= (1u << 30), "event %lld: Q", (long long)i);
                    T128 += Q[(size_t)i];
                }
            }
            if (verify) CHECK(T128 <= (u128)c.m << 30 && T128 > 0, "T outside (0, m 2^30]");
            const int64_t i = pick(Q, word_of(c, r, k));
            out.draws.push_back(i);
            out.q.push_back(i < 0 ? -1 : (int64_t)Q[(size_t)i]);
            if (i < 0) return out;
            for (uint32_t j = events[(size_t)i].lo; j < events[(size_t)i].hi; ++j) cnt[j] += 1;
        }
    }
    return out;
}

static uint64_t g_rng = 0x2545F4914F6CDD1DULL;
static uint64_t rnd64() { return fmk_sb_word(0, g_rng++); }
static int64_t rnd(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd64() % (uint64_t)(hi - lo + 1)); }

static int self_check()
{
    // ---- brute force == compressed
    long long cases = 0, draws = 0;
    for (int it = 0; it < 400; ++it) {
        Case c;
        c.n = rnd(1, 120); c.m = rnd(1, 14); c.K = rnd(1, 40); c.R = rnd(1, 3); c.seed = rnd64();
        for (int64_t i = 0; i < c.m; ++i) {
            const int64_t e = rnd(0, c.n - 1);
            c.ev.push_back(e);
            c.touch.push_back(it % 5 == 0 ? e : rnd(e, c.n - 1));
        }
        if (it % 7 == 0 && c.m > 1) { c.ev[1] = c.ev[0]; c.touch[1] = c.touch[0]; }         // a duplicate
        if (it % 3 == 0)
            for (int64_t w = 0; w < c.R * c.K; ++w) c.words.push_back(w % 4 == 0 ? 0 : w % 4 == 1 ? ~(uint64_t)0 : rnd64());
        const Result a = brute(c), b = compressed(c, true);
        CHECK(a.draws == b.draws && a.q == b.q, "case %d: brute force and compressed form differ", it);
        for (int64_t d : b.draws) CHECK(d >= 0 && d < c.m, "case %d: a draw outside the events", it);
        ++cases;
        draws += (long long)b.draws.size();
    }
    // ---- Q on random and extreme operands
    long long quotients = 0;
    for (int it = 0; it < 2000000; ++it) {
        const uint64_t L = it % 3 == 0 ? ((uint64_t)1 << 32) - (uint64_t)rnd(0, 3) : it % 3 == 1 ? (uint64_t)rnd(1, 100) : (uint64_t)rnd(1, (int64_t)1 << 32);
        uint64_t S = it % 4 == 0 ? L << 30 : it % 4 == 1 ? L * (uint64_t)rnd(0, 1 << 30) : (uint64_t)(((u128)rnd64() * ((L << 30) + 1)) >> 64);
        if (it % 8 == 1 && S) S -= 1;                                                       // just below a multiple of L
        CHECK(fmk_sb_q(S, L) == S / L, "Q(%llu, %llu)", (unsigned long long)S, (unsigned long long)L);
        ++quotients;
    }
    for (uint32_t cc = 0; cc < (1u << 24); cc += (cc < 70000 ? 1 : 997)) CHECK(fmk_sb_w(cc) >= 64u && fmk_sb_w(cc) == (1u << 30) / (cc + 1), "w(%u)", cc);
    CHECK(fmk_sb_target(~(uint64_t)0, 12345) == 12344 && fmk_sb_target(0, 12345) == 0 && fmk_sb_target((uint64_t)1 << 63, 10) == 5, "target");
    // ---- the 64-bit bounds at n = 2^32: the whole axis drawn again and again (steering words), short spans at both ends and inside
    Case c;
    c.n = (int64_t)1 << 32; c.K = 300; c.R = 1; c.seed = 0;
    c.ev = {0, 0, c.n - 1, 5, (int64_t)1 << 31, c.n - 4096};
    c.touch = {c.n - 1, 0, c.n - 1, 70000, ((int64_t)1 << 31) + 1, c.n - 1};
    c.m = (int64_t)c.ev.size();
    for (int64_t k = 0; k < c.K; ++k) c.words.push_back(k % 3 == 2 ? rnd64() : 0);          // word 0 draws event 0: the whole axis
    const Result big = compressed(c, true);
    long long whole = 0;
    for (int64_t d : big.draws) whole += d == 0;
    CHECK(big.q[0] == (1 << 30) && whole >= 200, "the whole-axis span: Q %lld, drawn %lld times", (long long)big.q[0], whole);
    printf("cases %lld draws %lld quotients %lld whole-axis draws %lld failed checks %lld\n", cases, draws, quotients, whole, g_failed);
    return g_failed ? 1 : 0;
}

static bool read_i64(int64_t *v) { long long x; if (scanf("%lld", &x) != 1) return false; *v = x; return true; }
static bool read_u64(uint64_t *v) { unsigned long long x; if (scanf("%llu", &x) != 1) return false; *v = x; return true; }

int main(int argc, char **argv)
{
    const bool timed = argc > 1 && strcmp(argv[1], "time") == 0;
    int64_t n_cases = 0;
    Case c;
    while (!isatty(0) && read_i64(&c.m)) {
        int64_t n_words;
        if (!read_i64(&c.n) || !read_i64(&c.K) || !read_i64(&c.R) || !read_u64(&c.seed) || !read_i64(&n_words)) { printf("bad case header\n"); return 2; }
        if (c.m < 1 || c.m > FMK_SB_MAX_EVENTS || c.K < 1 || c.K > FMK_SB_MAX_DRAWS || c.R < 1 || c.R > FMK_SB_MAX_WORDS / c.K || c.n < 0 ||
            c.n > FMK_SB_MAX_AXIS || (n_words != 0 && n_words != c.R * c.K)) { printf("case outside the bounds\n"); return 2; }
        c.ev.assign((size_t)c.m, 0); c.touch.assign((size_t)c.m, 0); c.words.assign((size_t)n_words, 0);
        for (int64_t i = 0; i < c.m; ++i) {
            if (!read_i64(&c.ev[(size_t)i]) || !read_i64(&c.touch[(size_t)i])) { printf("bad event\n"); return 2; }
            if (c.ev[(size_t)i] < 0 || c.touch[(size_t)i] < c.ev[(size_t)i] || c.touch[(size_t)i] >= c.n) { printf("event outside the axis\n"); return 2; }
        }
        for (int64_t w = 0; w < n_words; ++w) if (!read_u64(&c.words[(size_t)w])) { printf("bad word\n"); return 2; }
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        const Result res = compressed(c, false);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (timed) printf("time_s %.6f\n", (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec));
        else if (c.n <= ((int64_t)1 << 20)) {
            const Result b = brute(c);
            if (b.draws != res.draws || b.q != res.q) { printf("case %lld: brute force and compressed form differ\n", (long long)n_cases); return 1; }
        }
        printf("draws");
        for (int64_t d : res.draws) printf(" %lld", (long long)d);
        printf("\nq");
        for (int64_t q : res.q) printf(" %lld", (long long)q);
        printf("\n");
        ++n_cases;
    }
    if (n_cases) return 0;
    return self_check();
}
