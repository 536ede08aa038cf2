// Host check of the one-lane sorting network of finmlkit_amd/csrc/fmk_bars.h (fmk_lane_sort / fmk_lane_pick) at the three sizes
// the kernels instantiate:  g++ -O2 -std=c++17 tools/lanesort_check.cpp -o lanesort_check && ./lanesort_check
//   N = 16: all 2^16 zero-one inputs -- by the zero-one principle the network then sorts any 16 keys;
//   N = 32, 64: the 256 zero-one inputs that repeat one 8-bit pattern in every aligned block of 8; every threshold pattern
//     (x[i] = perm[i] >= t, t = 0 .. N) of 1 000 seeded random permutations -- a network sorts a permutation exactly when it sorts
//     these; 10 000 seeded random key arrays with duplicates, 0, 0xFFFFFFFF (MedKey<false>::MAXK, the padding of idle slots).
// Every output is compared with std::sort of its input, and fmk_lane_pick(r, i) with r[i] for every i.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../finmlkit_amd/csrc/fmk_bars.h"

static uint64_t rng_state = 0x2545F4914F6CDD1DULL;
static uint64_t rng()
{
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ULL);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

static long checked = 0, failed = 0;

template <int N>
static void check(const uint32_t (&in)[N])
{
    uint32_t r[N], want[N];
    std::copy(in, in + N, r);
    std::copy(in, in + N, want);
    std::sort(want, want + N);
    fmk_lane_sort<N>(r);
    bool ok = std::equal(r, r + N, want);
    for (int i = 0; i < N; ++i) ok = ok && fmk_lane_pick<N>(r, i) == r[i];
    ++checked;
    if (!ok) ++failed;
}

template <int N>
static void sampled()
{
    uint32_t x[N];
    for (unsigned pat = 0; pat < 256; ++pat) {
        for (int i = 0; i < N; ++i) x[i] = (pat >> (i & 7)) & 1u;
        check<N>(x);
    }
    for (int seed = 0; seed < 1000; ++seed) {
        int perm[N];
        for (int i = 0; i < N; ++i) perm[i] = i;
        for (int i = N - 1; i > 0; --i) std::swap(perm[i], perm[rng() % (uint64_t)(i + 1)]);
        for (int t = 0; t <= N; ++t) {
            for (int i = 0; i < N; ++i) x[i] = perm[i] >= t ? 1u : 0u;
            check<N>(x);
        }
    }
    static const uint32_t special[4] = {0u, 0xFFFFFFFFu, 0x007FFFFFu, 0xFF800000u};
    for (int k = 0; k < 10000; ++k) {
        const int distinct = 1 + (int)(rng() % N);                   // few distinct values: many duplicates
        uint32_t pool[N];
        for (int i = 0; i < distinct; ++i) pool[i] = (rng() & 3) == 0 ? special[rng() & 3] : (uint32_t)rng();
        const int L = (int)(rng() % (N + 1));                        // a bar of L keys, padded like the kernels do
        for (int i = 0; i < N; ++i) x[i] = i < L ? pool[rng() % (uint64_t)distinct] : 0xFFFFFFFFu;
        check<N>(x);
    }
}

int main()
{
    uint32_t x[16];
    for (unsigned pat = 0; pat < 65536; ++pat) {
        for (int i = 0; i < 16; ++i) x[i] = (pat >> i) & 1u;
        check<16>(x);
    }
    sampled<32>();
    sampled<64>();
    printf("lane sorts checked: %ld, failed checks: %ld\n", checked, failed);
    return failed != 0;
}
