// fmk_lz_rule.h -- what decides a value of the encoded-series entropies (fmk_lz.hip): which code is invalid, the id
// of a word, and the length of a run of matches read from equality masks.  Plain C++17, so that the kernels and a host program
// (tools/lz_check.cpp) run the same text.
//
// The masks of one wave and one lag d: the wave owns the 64 positions p0 .. p0 + 63, and bit b of word j says
// codes[k] == codes[k - d] at k = p0 + 64 j + b.  So the run of lane l starts at bit l of word 0, and what lies behind word 0 is
// the same for every lane: cont[j], the ones in a row from bit 0 of word j on, through the words behind it.  The wave takes the
// words last to first, carrying cont, and ends with one run per lane -- the same steps whatever the data.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define FMK_LZ_FN __host__ __device__ __forceinline__
#else
#define FMK_LZ_FN static inline
#endif

#define FMK_LZ_INVALID 255                 // never a code: what encode gives a NaN
#define FMK_LZ_MAX_EDGES 254
#define FMK_LZ_MAX_ALPHABET 255
#define FMK_LZ_MAX_WORDS 4096              // alphabet^word, the bins of the plug-in histogram
#define FMK_LZ_MAX_WINDOW 4096
#define FMK_LZ_MAX_LOOKBACK 1024

// a code the estimators do not count: a window that reads one gives NaN
FMK_LZ_FN bool fmk_lz_invalid(uint8_t code, int alphabet) { return (int)code >= alphabet; }

// the code of a value: the edges at or below it (np.searchsorted(edges, x, side="right"): -inf gives 0, +inf n_edges), NaN invalid
FMK_LZ_FN uint8_t fmk_lz_code(const double *edges, int n_edges, double x)
{
    if (x != x) return FMK_LZ_INVALID;
    int lo = 0, hi = n_edges;                                        // edges[0 .. lo) <= x < edges[hi ..)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return (uint8_t)lo;
}

// alphabet^word when that is at most FMK_LZ_MAX_WORDS, 0 when it is more (alphabet >= 2, word >= 1)
FMK_LZ_FN int fmk_lz_bins(int64_t alphabet, int64_t word)
{
    int64_t bins = 1;
    for (int64_t j = 0; j < word; ++j) {
        bins *= alphabet;
        if (bins > FMK_LZ_MAX_WORDS) return 0;
    }
    return (int)bins;
}

// the id of the word codes[0 .. word), the first code the most significant digit: in 0 .. alphabet^word - 1; -1 when the word holds
// an invalid code
FMK_LZ_FN int fmk_lz_word_id(const uint8_t *codes, int word, int alphabet)
{
    int id = 0;
    bool bad = false;
    for (int j = 0; j < word; ++j) {
        bad |= fmk_lz_invalid(codes[j], alphabet);
        id = id * alphabet + (int)codes[j];
    }
    return bad ? -1 : id;
}

// trailing ones of a word, 64 for a full one
FMK_LZ_FN int fmk_lz_ones(uint64_t m) { return ~m ? __builtin_ctzll(~m) : 64; }

// cont[j] from word j and cont[j + 1] (0 behind the last word)
FMK_LZ_FN int fmk_lz_cont(uint64_t m, int cont_next)
{
    const int c = fmk_lz_ones(m);
    return c == 64 ? 64 + cont_next : c;
}

// the run that starts at bit `bit` of word 0, cont1 = cont[1], capped at `cap`
FMK_LZ_FN int fmk_lz_run(uint64_t m0, int bit, int cont1, int cap)
{
    const int c = fmk_lz_ones(m0 >> bit);                            // (the shift brings zeros in: c <= 64 - bit for bit > 0)
    const int run = c >= 64 - bit ? 64 - bit + cont1 : c;
    return run < cap ? run : cap;
}

// the match length of a position from the longest capped run over the lags; 0 where the position has none (invalid)
FMK_LZ_FN uint16_t fmk_lz_lambda(int best_run, bool invalid) { return invalid ? (uint16_t)0 : (uint16_t)(1 + best_run); }
