// lz_check.cpp -- the plain C++ of the encoded-series entropies (finmlkit_amd/csrc/fmk_lz_rule.h) on the host, against the
// literal definitions.  Fails when
//   - the run a wave reads from its equality words (fmk_lz_cont from the last word to word 1, then fmk_lz_run at every bit of word 0)
//     is not the count of ones in a row from that bit on, capped -- on random masks of every density, and on the adversarial ones: all
//     ones, one zero at bit 63 / 64 / 65 / 127 / 128, a zero at every single position, runs that pass the cap, caps 1 .. 1024;
//   - the match length k_lz_match's walk gives a position (the words built from a message as the kernel builds them, lag by lag) is
//     not the book's snippet 18.3 restated on arrays, or the invalid rule is not "a 255 in codes[p-n .. p+n), or the span leaves the
//     message" -- on random binary, 16-ary, constant, periodic and spliced messages;
//   - a word id is not the positional value of its codes, is not unique per word, or an invalid code does not give -1;
//   - fmk_lz_bins is not alphabet^word up to 4096 and 0 beyond, or fmk_lz_code is not the count of edges <= x (255 for a NaN).
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o lz_check tools/lz_check.cpp && ./lz_check
// (any argument: a quick run with fewer random cases)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <vector>

#include "../finmlkit_amd/csrc/fmk_lz_rule.h"

static long long g_failed, g_runs, g_positions, g_words;

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

static int mask_words(int n) { return 1 + (n + 62) / 64; }            // (fmk_lz.hip: lz_mask_words)

// the wave's walk over one lag's words -> the capped run of every lane
static void wave_runs(const std::vector<uint64_t> &m, int cap, int (&run)[64])
{
    int cont = 0;
    for (int j = (int)m.size() - 1; j >= 1; --j) cont = fmk_lz_cont(m[j], cont);
    for (int lane = 0; lane < 64; ++lane) run[lane] = fmk_lz_run(m[0], lane, cont, cap);
}

static int literal_run(const std::vector<uint64_t> &m, int bit, int cap)
{
    int run = 0;
    for (size_t k = (size_t)bit; k < 64 * m.size() && run < cap && ((m[k / 64] >> (k % 64)) & 1); ++k) ++run;
    return run;
}

static void check_masks(const std::vector<uint64_t> &m, int cap, const char *what)
{
    int run[64];
    wave_runs(m, cap, run);
    for (int lane = 0; lane < 64; ++lane) {
        const int want = literal_run(m, lane, cap);
        CHECK(run[lane] == want, "%s: %d words, cap %d, lane %d: %d, literal %d", what, (int)m.size(), cap, lane, run[lane], want);
        ++g_runs;
    }
}

static void masks(bool quick)
{
    const int caps[] = {1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 200, 1000, 1023, 1024};
    for (int cap : caps) {
        const int nw = mask_words(cap);
        std::vector<uint64_t> m((size_t)nw, ~0ull);
        check_masks(m, cap, "all ones");
        for (int z = 0; z < 64 * nw; ++z) {                           // one zero, everywhere: 63 / 64 / 65 and every word boundary
            m[(size_t)z / 64] &= ~(1ull << (z % 64));
            check_masks(m, cap, "one zero");
            m[(size_t)z / 64] = ~0ull;
        }
        std::vector<uint64_t> longer((size_t)nw + 3, ~0ull);          // more words than the cap needs: the run passes the cap
        check_masks(longer, cap, "past the cap");
        std::vector<uint64_t> zeros((size_t)nw, 0ull);
        check_masks(zeros, cap, "all zeros");
        const int reps = quick ? 20 : 400;
        for (int r = 0; r < reps; ++r) {
            const double density = r % 8 == 0 ? 0.5 : 1.0 - 1.0 / (double)(1 + rnd64() % 300);      // mostly long runs
            for (auto &w : m) {
                w = 0;
                for (int b = 0; b < 64; ++b) w |= (uint64_t)(rnd01() < density) << b;
            }
            check_masks(m, cap, "random");
        }
    }
}

// snippet 18.3 on arrays: 1 + the longest l <= n with codes[p .. p+l) == codes[j .. j+l) for some j in p-n .. p-1
static int literal_lambda(const std::vector<uint8_t> &c, int64_t p, int n)
{
    const int64_t N = (int64_t)c.size();
    if (p < n || p > N - n) return 0;
    for (int64_t k = p - n; k < p + n; ++k)
        if (c[(size_t)k] == FMK_LZ_INVALID) return 0;
    int best = 0;
    for (int l = 1; l <= n; ++l)
        for (int64_t j = p - n; j < p; ++j) {
            bool same = true;
            for (int q = 0; q < l && same; ++q) same = c[(size_t)(p + q)] == c[(size_t)(j + q)];
            if (same) { best = l; break; }
        }
    return 1 + best;
}

// the kernel's walk for the wave that owns p0 .. p0 + 63: codes outside the message are invalid, as staged
static void check_message(const std::vector<uint8_t> &c, int n, const char *what)
{
    const int64_t N = (int64_t)c.size();
    const int nw = mask_words(n);
    auto at = [&](int64_t g) { return g >= 0 && g < N ? c[(size_t)g] : (uint8_t)FMK_LZ_INVALID; };
    for (int64_t p0 = 0; p0 < N; p0 += 64) {
        int best[64] = {0};
        std::vector<uint64_t> m((size_t)nw);
        for (int d = 1; d <= n; ++d) {
            for (int j = 0; j < nw; ++j) {
                m[(size_t)j] = 0;
                for (int b = 0; b < 64; ++b) m[(size_t)j] |= (uint64_t)(at(p0 + 64 * j + b) == at(p0 + 64 * j + b - d)) << b;
            }
            int run[64];
            wave_runs(m, n, run);
            for (int lane = 0; lane < 64; ++lane) best[lane] = run[lane] > best[lane] ? run[lane] : best[lane];
        }
        for (int lane = 0; lane < 64 && p0 + lane < N; ++lane) {
            const int64_t p = p0 + lane;
            bool invalid = false;
            for (int64_t k = p - n; k < p + n; ++k) invalid |= fmk_lz_invalid(at(k), FMK_LZ_INVALID);
            const int got = fmk_lz_lambda(best[lane], invalid), want = literal_lambda(c, p, n);
            CHECK(got == want, "%s: N %lld, lookback %d, p %lld: %d, literal %d", what, (long long)N, n, (long long)p, got, want);
            CHECK(got <= n + 1, "%s: %d beyond the cap", what, got);
            ++g_positions;
        }
    }
}

static void messages(bool quick)
{
    const int looks[] = {1, 2, 3, 7, 20, 63, 64, 65, 70, 127, 128, 129};      // (the last three: three mask words, the full run only)
    const int64_t N = quick ? 150 : 330;
    for (int n : looks) {
        if (quick && n > 70) continue;
        std::vector<uint8_t> c((size_t)N);
        for (auto &v : c) v = (uint8_t)(rnd64() & 1);
        check_message(c, n, "binary");
        for (auto &v : c) v = (uint8_t)(rnd64() & 15);
        check_message(c, n, "16-ary");
        for (auto &v : c) v = 3;
        check_message(c, n, "constant");
        for (size_t i = 0; i < c.size(); ++i) c[i] = (uint8_t)(i % 2);
        check_message(c, n, "period 2");
        for (size_t i = 0; i < c.size(); ++i) c[i] = (uint8_t)(i % 65);
        check_message(c, n, "period 65");
        for (size_t i = 0; i < c.size(); ++i) c[i] = (uint8_t)(i % 255);
        check_message(c, n, "k mod 255");
        for (auto &v : c) v = (uint8_t)(rnd64() & 1);
        for (size_t i = 40; i < 40 + 100 && i < c.size(); ++i) c[i] = 1;          // a constant stretch across a wave's edge
        check_message(c, n, "spliced");
        c[0] = c[64] = c[(size_t)N - 1] = FMK_LZ_INVALID;
        check_message(c, n, "invalid codes");
        std::vector<uint8_t> tiny((size_t)(2 * n - 1), 1);             // N < 2 n: no position has a span
        check_message(tiny, n, "shorter than two lookbacks");
    }
}

static void words(bool quick)
{
    const int shapes[][2] = {{2, 1}, {2, 2}, {2, 12}, {3, 7}, {4, 6}, {16, 3}, {64, 2}, {255, 1}, {10, 3}};
    for (auto &s : shapes) {
        const int alphabet = s[0], word = s[1];
        const int bins = fmk_lz_bins(alphabet, word);
        long long want = 1;
        for (int j = 0; j < word; ++j) want *= alphabet;
        CHECK(bins == want && bins <= FMK_LZ_MAX_WORDS, "bins(%d, %d) = %d", alphabet, word, bins);
        std::map<int, std::vector<uint8_t>> seen;
        const int reps = quick ? 300 : 5000;
        for (int r = 0; r < reps; ++r) {
            std::vector<uint8_t> w((size_t)word);
            long long value = 0;
            for (auto &v : w) { v = (uint8_t)(rnd64() % (uint64_t)alphabet); value = value * alphabet + v; }
            const int id = fmk_lz_word_id(w.data(), word, alphabet);
            CHECK(id == value && id >= 0 && id < bins, "word id %d, value %lld, bins %d", id, value, bins);
            auto it = seen.find(id);
            if (it != seen.end()) CHECK(it->second == w, "two words share id %d", id);
            else seen[id] = w;
            w[(size_t)(rnd64() % (uint64_t)word)] = (uint8_t)(alphabet + rnd64() % (uint64_t)(256 - alphabet));
            CHECK(fmk_lz_word_id(w.data(), word, alphabet) == -1, "an invalid code in a word of alphabet %d", alphabet);
            ++g_words;
        }
    }
    CHECK(fmk_lz_bins(2, 13) == 0 && fmk_lz_bins(16, 4) == 0 && fmk_lz_bins(255, 2) == 0 && fmk_lz_bins(65, 2) == 0, "bins beyond 4096");
    CHECK(fmk_lz_bins(64, 2) == 4096 && fmk_lz_bins(2, 12) == 4096 && fmk_lz_bins(2, 1000000) == 0, "bins at 4096");
    CHECK(fmk_lz_invalid(255, 255) && !fmk_lz_invalid(254, 255) && fmk_lz_invalid(2, 2) && !fmk_lz_invalid(1, 2), "the invalid rule");
}

static void codes()
{
    const int sizes[] = {1, 2, 3, 7, 254};
    for (int ne : sizes) {
        std::vector<double> e((size_t)ne);
        double v = -3.0;
        for (auto &x : e) { v += 0.001 + rnd01(); x = v; }
        std::vector<double> xs = {-INFINITY, INFINITY, 0.0, -0.0, e[0], e[(size_t)ne - 1], nextafter(e[0], -INFINITY), nextafter(e[0], INFINITY)};
        for (int r = 0; r < 2000; ++r) xs.push_back(r % 3 ? -4.0 + 300.0 * rnd01() : e[(size_t)(rnd64() % (uint64_t)ne)]);
        for (double x : xs) {
            int want = 0;
            for (double edge : e) want += edge <= x;
            CHECK(fmk_lz_code(e.data(), ne, x) == want, "code of %.17g with %d edges", x, ne);
        }
        CHECK(fmk_lz_code(e.data(), ne, NAN) == FMK_LZ_INVALID, "NaN is the invalid code");
    }
}

int main(int argc, char **)
{
    const bool quick = argc > 1;
    masks(quick);
    messages(quick);
    words(quick);
    codes();
    printf("runs %lld positions %lld words %lld failed checks %lld\n", g_runs, g_positions, g_words, g_failed);
    return g_failed ? 1 : 0;
}
