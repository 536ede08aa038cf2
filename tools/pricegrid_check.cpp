// Host check of the price grid of finmlkit_amd/csrc/fmk_common.h (fmk_grid_decode, fmk_grid_tick, fmk_grid_choose_d,
// fmk_grid_choose_form): the decode, and the choice of scale and form that fmk_price_grid_build_dev makes, as plain C++ on the CPU:
//   hipcc -O2 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         tools/pricegrid_check.cpp -o pricegrid_check
//   ./pricegrid_check            (a number scales the sweeps: ./pricegrid_check 10 is the full sweep, about half a minute)
//   1. form B is the correctly rounded quotient: for every d in 0 .. 8, every k below `dense` (5e6 by default, 5e7 in the full sweep),
//      the same range negated, and `rand` random signed 32-bit k (3.5e7 / 3.5e8), fmk_grid_decode<B> has the bits of (double)k / 10^d;
//      INT32_MIN, INT32_MAX and 0 are among them.  Form A differs from the quotient on a good share of k (printed): it alone would
//      not serve real tapes.
//   2. the certificate on whole tapes (the host mirror of the build kernel: fmk_grid_choose_d on the kernel's sample, fmk_grid_tick
//      on every tick, fmk_grid_choose_form on the counts): k * 0.01 -> A at d = 2; quotients k / 10^d -> B at d; and the refusals --
//      -0.0, NaN, +-inf, one off-grid tick (first, last, in between), k beyond int32, full-mantissa doubles -- all give "no grid";
//      n = 0 gives no grid, n = 1 certifies.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../finmlkit_amd/csrc/fmk_common.h"

static uint64_t rng_state = 0x2545F4914F6CDD1DULL;
static uint64_t rng()
{
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ULL);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

static long failed = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failed <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                  \
    } while (0)

// ---- 1. the decode
static void sweep_form_b(int64_t dense, int64_t nrand)
{
    for (int d = 0; d <= FMK_GRID_MAX_D; ++d) {
        const double r = fmk_grid_recip(d), s = fmk_grid_scale(d);
        CHECK(r == 1.0 / s, "d = %d: the literal reciprocal is not RN(1 / s)", d);
        int64_t bad_b = 0, bad_a = 0, total = 0;
        auto one = [&](int32_t k) {
            const uint64_t want = fmk_grid_bits((double)k / s);
            bad_b += fmk_grid_bits(fmk_grid_decode<FMK_GRID_B>(k, r, s)) != want;
            bad_a += fmk_grid_bits(fmk_grid_decode<FMK_GRID_A>(k, r, s)) != want;
            ++total;
        };
        for (int64_t k = 0; k < dense; ++k) { one((int32_t)k); one((int32_t)-k); }
        for (int64_t i = 0; i < nrand; ++i) one((int32_t)(uint32_t)rng());
        one(std::numeric_limits<int32_t>::min());
        one(std::numeric_limits<int32_t>::max());
        CHECK(bad_b == 0, "d = %d: form B differs from the quotient on %lld of %lld k", d, (long long)bad_b, (long long)total);
        printf("d = %d: %lld k, form B mismatches %lld, form A mismatches %lld (%.1f %%)\n", d, (long long)total, (long long)bad_b,
               (long long)bad_a, 100.0 * (double)bad_a / (double)total);
    }
}

// ---- 2. the certificate: what fmk_price_grid_build_dev does, on the host
struct Built { fmk_price_grid g; std::vector<int32_t> k; };
static Built build(const std::vector<double> &price)
{
    Built out{fmk_price_grid{FMK_GRID_NONE, 0, 0.0, 0.0}, {}};
    const int64_t n = (int64_t)price.size();
    if (n == 0) return out;
    const int64_t m = n < FMK_GRID_SAMPLE ? n : FMK_GRID_SAMPLE;
    double sample[FMK_GRID_SAMPLE];
    for (int64_t i = 0; i < m; ++i) sample[i] = price[i == m - 1 ? n - 1 : i * (n / m)];      // k_price_grid_sample
    const int d = fmk_grid_choose_d(sample, m);
    if (d < 0) return out;
    const double r = fmk_grid_recip(d), s = fmk_grid_scale(d);
    uint64_t mis[2] = {0, 0};
    out.k.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {                                                          // k_price_grid_build
        bool a, b;
        out.k[(size_t)i] = fmk_grid_tick(price[(size_t)i], r, s, &a, &b);
        mis[0] += !a;
        mis[1] += !b;
    }
    const int form = fmk_grid_choose_form(mis[0], mis[1]);
    if (form == FMK_GRID_NONE) out.k.clear();
    else out.g = fmk_price_grid{form, d, r, s};
    return out;
}

static void expect(const char *what, const std::vector<double> &price, int form, int d)
{
    const Built b = build(price);
    CHECK(b.g.form == form && (form == FMK_GRID_NONE || b.g.d == d), "%s: form %d at d = %d, expected form %d at d = %d", what, b.g.form,
          b.g.d, form, d);
    if (b.g.form == FMK_GRID_NONE) { CHECK(b.k.empty(), "%s: a column without a grid", what); return; }
    CHECK(b.k.size() == price.size(), "%s: column length", what);
    for (size_t i = 0; i < price.size() && i < b.k.size(); ++i) {
        const double p = b.g.form == FMK_GRID_A ? fmk_grid_decode<FMK_GRID_A>(b.k[i], b.g.r, b.g.s)
                                                : fmk_grid_decode<FMK_GRID_B>(b.k[i], b.g.r, b.g.s);
        CHECK(fmk_grid_bits(p) == fmk_grid_bits(price[i]), "%s: tick %zu does not decode to its price", what, i);
    }
}

static void tapes()
{
    const size_t n = 10007;
    std::vector<double> a(n), neg(n);
    int64_t k = 10000;
    for (size_t i = 0; i < n; ++i) {
        k += (int64_t)(rng() % 7) - 3;
        a[i] = (double)k * 0.01;
        neg[i] = (double)(k - 10020) * 0.01;                    // both signs
    }
    expect("k * 0.01", a, FMK_GRID_A, 2);
    expect("negative k * 0.01", neg, FMK_GRID_A, 2);
    for (int d = 1; d <= FMK_GRID_MAX_D; ++d) {                // real tapes: the nearest double to a decimal string
        std::vector<double> q(n);
        for (size_t i = 0; i < n; ++i) {
            int64_t kk = (int64_t)(rng() % 2000000000u);
            if (kk % 10 == 0) ++kk;                             // (no tick on the coarser grid: d is the scale the tape needs)
            q[i] = (double)kk / fmk_grid_scale(d);
        }
        char what[64];
        snprintf(what, sizeof what, "quotients at d = %d", d);
        expect(what, q, FMK_GRID_B, d);
    }
    expect("whole numbers", std::vector<double>{3.0, -7.0, 0.0, 2147483647.0, -2147483648.0}, FMK_GRID_A, 0);
    expect("n = 0", std::vector<double>{}, FMK_GRID_NONE, 0);
    {
        const Built one = build(std::vector<double>{101.27});
        CHECK(one.g.form != FMK_GRID_NONE && one.g.d == 2 && one.k.size() == 1 && one.k[0] == 10127, "n = 1: form %d, d %d", one.g.form,
              one.g.d);
    }
    // the refusals: each fails the comparison by itself
    auto with = [&](size_t at, double v) { std::vector<double> x = a; x[at] = v; return x; };
    expect("-0.0", with(5, -0.0), FMK_GRID_NONE, 0);
    expect("-0.0 first (sampled)", with(0, -0.0), FMK_GRID_NONE, 0);
    expect("NaN", with(5, std::nan("")), FMK_GRID_NONE, 0);
    expect("+inf", with(5, INFINITY), FMK_GRID_NONE, 0);
    expect("-inf", with(n - 1, -INFINITY), FMK_GRID_NONE, 0);
    expect("off-grid first", with(0, std::nextafter(a[0], 1e9)), FMK_GRID_NONE, 0);
    expect("off-grid last", with(n - 1, std::nextafter(a[n - 1], 1e9)), FMK_GRID_NONE, 0);
    expect("off-grid in between", with(5, std::nextafter(a[5], -1e9)), FMK_GRID_NONE, 0);
    expect("k = 2^31", with(5, 21474836.48), FMK_GRID_NONE, 0);
    expect("k = -2^31 - 1", with(5, -21474836.49), FMK_GRID_NONE, 0);
    {
        std::vector<double> big = a;
        for (double &p : big) p += 30000000.0;                  // k = 3e9 at d = 2: every tick overflows
        expect("every k beyond int32", big, FMK_GRID_NONE, 0);
    }
    {
        std::vector<double> full(n);
        for (double &p : full) p = 10.0 + (double)(rng() >> 11) * (1.0 / 9007199254740992.0) * 990.0;
        expect("full-mantissa doubles", full, FMK_GRID_NONE, 0);
    }
    // the edges of the range do encode
    int32_t kk;
    CHECK(fmk_grid_encode(21474836.47, 100.0, &kk) && kk == 2147483647, "INT32_MAX does not encode");
    CHECK(fmk_grid_encode(-21474836.48, 100.0, &kk) && kk == std::numeric_limits<int32_t>::min(), "INT32_MIN does not encode");
    CHECK(!fmk_grid_encode(1e300, 100.0, &kk) && !fmk_grid_encode(std::nan(""), 100.0, &kk), "a huge price or a NaN encodes");
}

int main(int argc, char **argv)
{
    const int64_t scale = argc > 1 ? atoll(argv[1]) : 1;
    sweep_form_b(5000000 * scale, 35000000 * scale);
    tapes();
    printf("%s (%ld failures)\n", failed ? "FAILED" : "ok", failed);
    return failed ? 1 : 0;
}
