// fmk_seqboot_rule.h -- everything of the sequential bootstrap (fmk_seqboot.hip) that decides a bit: the weight of a
// concurrency count, the random word of a draw, the target inside the total, the average uniqueness Q of a candidate, and the
// compression of the axis to the intervals between span boundaries.  Plain C++17 and integers only, so that the kernel, the entry
// points' host code and a host program (tools/seqboot_check.cpp) run the same text; every sum in between is an exact unsigned
// 64-bit sum, so its order is free.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#ifdef __HIPCC__
#define FMK_SB_FN __host__ __device__ __forceinline__
#else
#define FMK_SB_FN static inline
#endif

#define FMK_SB_ONE_LOG2 30                           // Q and w are in units of 2^-30
#define FMK_SB_MAX_EVENTS (((int64_t)1 << 31) - 1)   // T <= m * 2^30 <= 2^61
#define FMK_SB_MAX_DRAWS ((int64_t)1 << 24)          // w(c) >= 64: Q > 0 and T > 0 always
#define FMK_SB_MAX_WORDS ((int64_t)1 << 40)          // n_runs * n_draws
#define FMK_SB_MAX_AXIS ((int64_t)1 << 32)           // S <= L * 2^30 <= 2^62

// w(c) = floor(2^30 / (c + 1)): the uniqueness of one position that c earlier draws cover, the candidate itself counted
FMK_SB_FN uint32_t fmk_sb_w(uint32_t c) { return ((uint32_t)1 << FMK_SB_ONE_LOG2) / (c + 1u); }

// the random word of draw `index` = run * n_draws + draw: splitmix64 at the counter index + 1
FMK_SB_FN uint64_t fmk_sb_word(uint64_t seed, uint64_t index)
{
    uint64_t z = seed + (index + 1u) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// target = the high 64 bits of word * total: uniform on [0, total) up to 2^-64 * total
FMK_SB_FN uint64_t fmk_sb_target(uint64_t word, uint64_t total)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(word, total);
#else
    return (uint64_t)(((unsigned __int128)word * total) >> 64);
#endif
}

// Q = floor(S / L) for 1 <= L <= 2^32 and S <= L * 2^30.  A float64 quotient is within one of it (S and the quotient carry a
// relative error of 2^-52 together, on a value of at most 2^30); the two loops then make it exact whatever the estimate was.
FMK_SB_FN uint64_t fmk_sb_q(uint64_t S, uint64_t L)
{
    uint64_t q = (uint64_t)((double)S / (double)L);
    int64_t r = (int64_t)(S - q * L);
    while (r < 0) { --q; r += (int64_t)L; }
    while (r >= (int64_t)L) { ++q; r -= (int64_t)L; }
    return q;
}

// One event on the compressed axis: it covers the intervals [lo, hi) and L = len_m1 + 1 positions (L may be 2^32).
struct FmkSbEvent { uint32_t lo, hi, len_m1; };

// ---- host only

// b = sorted unique of {e_i} and {t_i + 1}; interval j = [b_j, b_{j+1}), len_m1[j] = its length - 1 (J = b.size() - 1 <= 2m - 1
// intervals); event i covers [lo_i, hi_i).  The caller has checked 0 <= e_i <= t_i < n <= 2^32 and 1 <= m <= 2^31 - 1.
static inline void fmk_sb_compress(const int64_t *ev, const int64_t *touch, int64_t m, std::vector<uint32_t> &len_m1,
                                   std::vector<FmkSbEvent> &events)
{
    std::vector<int64_t> b((size_t)m * 2);
    for (int64_t i = 0; i < m; ++i) { b[(size_t)i * 2] = ev[i]; b[(size_t)i * 2 + 1] = touch[i] + 1; }
    std::sort(b.begin(), b.end());
    b.erase(std::unique(b.begin(), b.end()), b.end());
    const size_t J = b.size() - 1;
    len_m1.resize(J);
    for (size_t j = 0; j < J; ++j) len_m1[j] = (uint32_t)(b[j + 1] - b[j] - 1);
    events.resize((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        FmkSbEvent e;
        e.lo = (uint32_t)(std::lower_bound(b.begin(), b.end(), ev[i]) - b.begin());
        e.hi = (uint32_t)(std::lower_bound(b.begin(), b.end(), touch[i] + 1) - b.begin());
        e.len_m1 = (uint32_t)(touch[i] - ev[i]);
        events[(size_t)i] = e;
    }
}
