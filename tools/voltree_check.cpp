// voltree_check.cpp -- the table tree of the volume bar indexer (finmlkit_amd/csrc/fmk_voltree.h) on the host, from the header's
// own plan, composition and hand-down (plain C++; the kernels are wrappers over them).  Random close chains -- nxt strictly
// increasing, every hop at most W, chains that end in "no further close" before the tape does -- for W in {3, 4, 7}, blocks of W,
// W + 2 and 3 W ticks, radix 2, 3 and 16, 1 .. 40 blocks (0 .. 6 levels), a level-0 table filled directly, plain and packed.  Fails when
//   - the arrays a bound plan hands out overlap, leave the plan's byte count or put an int64 off 8-byte alignment;
//   - the top level's count for the first close is not the length of the sequential chain;
//   - walking the level-0 blocks from the handed-down (entry, slot) pairs does not write exactly the sequential chain into
//     slots 1, 2, ..., every slot once;
//   - a composition reports an overflow although no hop exceeds W, or none although the chain holds a hop beyond W.
//     g++ -O2 -std=c++17 -o voltree_check tools/voltree_check.cpp && ./voltree_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../finmlkit_amd/csrc/fmk_voltree.h"

static long long g_trees, g_failed, g_levels[VOL_MAX_LEVELS];

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            if (g_failed++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                           \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(uint32_t below)                   // splitmix64
{
    uint64_t x = (g_rng += 0x9E3779B97F4A7C15ULL);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return (uint32_t)(((x ^ (x >> 31)) >> 33) % below);
}

struct Case {
    int W, span0, radix, nblk0;
    bool packed;
    int64_t n;
    std::vector<uint32_t> nxt;
    std::vector<unsigned char> mem;
    VolTree t;
};

static void describe(const Case &c, char *buf, size_t len)
{
    snprintf(buf, len, "W %d span0 %d radix %d blocks %d n %lld %s", c.W, c.span0, c.radix, c.nblk0, (long long)c.n, c.packed ? "packed" : "plain");
}

// what a level-0 kernel leaves: row i of block b for the chain that enters at tick b * span0 + i
static void fill_level0(Case &c)
{
    for (int64_t b = 0; b < c.nblk0; ++b)
        for (int i = 0; i < c.W; ++i) {
            const int64_t j = b * c.span0 + i, bend = (b + 1) * c.span0;
            uint32_t e = VOL_END, cnt = 0;
            if (j < c.n) {
                cnt = 1;
                e = c.nxt[j];
                while (e != VOL_END && (int64_t)e < bend) { ++cnt; e = c.nxt[e]; }
            }
            if (c.packed) c.t.E[0][b * c.W + i] = (cnt << 16) | (e == VOL_END ? 0xFFFFu : e - (uint32_t)bend);
            else { c.t.E[0][b * c.W + i] = e; c.t.C[0][b * c.W + i] = cnt; }
        }
}

// -> did any composition report an overflow
static bool compose_levels(Case &c)
{
    bool any = false;
    VolTree &t = c.t;
    for (int k = 1; k <= t.K; ++k)
        for (int64_t b = 0; b < t.nblk[k]; ++b)
            for (int64_t i = 0; i < t.W; ++i) {
                bool ovf = false;
                const VolRow r = k == 1 && t.packed0
                    ? vol_tree_compose<true>(t.E[0], nullptr, t.nblk[0], t.span[0], t.W, t.radix, b, i, &ovf)
                    : vol_tree_compose<false>(t.E[k - 1], t.C[k - 1], t.nblk[k - 1], t.span[k - 1], t.W, t.radix, b, i, &ovf);
                t.E[k][b * t.W + i] = r.e;
                t.C[k][b * t.W + i] = r.c;
                any |= ovf;
            }
    return any;
}

static void check_regions(const Case &c, const unsigned char *base, size_t bytes)
{
    char what[160];
    describe(c, what, sizeof what);
    const VolTree &t = c.t;
    std::vector<std::pair<uintptr_t, uintptr_t>> r;
    for (int k = 0; k <= t.K; ++k) {
        const size_t rows = (size_t)t.nblk[k] * (size_t)t.W;
        r.push_back({(uintptr_t)t.E[k], (uintptr_t)(t.E[k] + rows)});
        r.push_back({(uintptr_t)t.C[k], (uintptr_t)(t.C[k] + rows)});
        r.push_back({(uintptr_t)t.ent[k], (uintptr_t)(t.ent[k] + t.nblk[k])});
        r.push_back({(uintptr_t)t.off[k], (uintptr_t)(t.off[k] + t.nblk[k])});
        CHECK((uintptr_t)t.off[k] % 8 == 0, "%s level %d", what, k);
    }
    CHECK(t.nblk[t.K] == 1, "%s", what);
    std::sort(r.begin(), r.end());
    CHECK(r.front().first >= (uintptr_t)base && r.back().second <= (uintptr_t)base + bytes, "%s", what);
    size_t sum = 0;
    for (size_t q = 0; q < r.size(); ++q) {
        sum += r[q].second - r[q].first;
        if (q) CHECK(r[q - 1].second <= r[q].first, "%s regions %zu and %zu", what, q - 1, q);
    }
    CHECK(sum == bytes, "%s: the regions hold %zu of %zu bytes", what, sum, bytes);
}

static void run_case(int W, int span0, int radix, int nblk0, bool packed, int variant)
{
    Case c;
    c.W = W; c.span0 = span0; c.radix = radix; c.nblk0 = nblk0; c.packed = packed;
    c.n = (int64_t)(nblk0 - 1) * span0 + 1 + rnd(span0);              // the last block holds 1 .. span0 ticks
    char what[160];
    describe(c, what, sizeof what);
    // variant 1: every chain ends ("no further close") at a tick well before the end of the tape
    const int64_t stop = variant == 1 ? (int64_t)rnd((uint32_t)c.n) : c.n;
    c.nxt.resize(c.n);
    for (int64_t j = 0; j < c.n; ++j) {
        const int64_t to = j + 1 + rnd(W);
        c.nxt[j] = to < c.n && j < stop ? (uint32_t)to : VOL_END;
    }
    c.t = vol_tree_plan(nblk0, span0, W, radix, packed);
    const size_t bytes = vol_tree_bytes(c.t), guard = 64;
    c.mem.assign(bytes + 2 * guard + 8, 0xA5);
    unsigned char *base = c.mem.data() + guard;
    base += (8 - (uintptr_t)base % 8) % 8;
    vol_tree_bind(c.t, base);
    check_regions(c, base, bytes);
    ++g_trees;
    ++g_levels[c.t.K];
    VolTree &t = c.t;

    fill_level0(c);
    CHECK(!compose_levels(c), "%s: an overflow without a hop beyond W", what);
    // the first close: a tick among the first W (variant 2: none at all)
    const uint32_t root = variant == 2 ? VOL_END : rnd((uint32_t)(c.n < W ? c.n : W));
    std::vector<uint32_t> chain;
    for (uint32_t j = root; j != VOL_END; j = c.nxt[j]) chain.push_back(j);
    if (root != VOL_END) {
        const uint32_t top = t.K == 0 && packed ? vol_unpack0(t.E[0][root], 0, span0).c : t.C[t.K][root];
        CHECK(top == chain.size(), "%s: the top level counts %u closes, the chain has %zu", what, top, chain.size());
    }
    t.ent[t.K][0] = root;
    t.off[t.K][0] = 1;
    for (int k = t.K; k >= 1; --k)
        for (int64_t b = 0; b < t.nblk[k]; ++b) {
            if (k == 1 && packed)
                vol_tree_hand_down<true>(t.ent[1][b], t.off[1][b], t.E[0], nullptr, t.nblk[0], t.span[0], t.W, radix, b, t.ent[0], t.off[0]);
            else
                vol_tree_hand_down<false>(t.ent[k][b], t.off[k][b], t.E[k - 1], t.C[k - 1], t.nblk[k - 1], t.span[k - 1], t.W, radix, b,
                                          t.ent[k - 1], t.off[k - 1]);
        }
    // the emit pass: every level-0 block writes its nodes
    std::vector<int64_t> out(chain.size() + 2, -1);
    std::vector<int> writes(chain.size() + 2, 0);
    for (int64_t b = 0; b < nblk0; ++b) {
        uint32_t j = t.ent[0][b];
        int64_t o = t.off[0][b];
        while (j != VOL_END && (int64_t)j < (b + 1) * span0) {
            CHECK(o >= 1 && o <= (int64_t)chain.size(), "%s: block %lld writes slot %lld of 1 .. %zu", what, (long long)b, (long long)o, chain.size());
            if (o >= 1 && o <= (int64_t)chain.size()) { out[o] = j; ++writes[o]; }
            ++o;
            j = c.nxt[j];
        }
    }
    for (size_t q = 1; q <= chain.size(); ++q)
        CHECK(writes[q] == 1 && out[q] == (int64_t)chain[q - 1], "%s: slot %zu written %d times, holds %lld, the chain's close is %u", what, q,
              writes[q], (long long)out[q], chain[q - 1]);
    // the guard bytes around the plan's region are untouched
    for (size_t q = 0; q < guard; ++q) CHECK(base[-1 - (ptrdiff_t)q] == 0xA5 && base[bytes + q] == 0xA5, "%s: a write outside the region", what);

    // a hop beyond W on the chain: the last chain node of some block jumps to row W of the next block
    if (t.K >= 1 && chain.size() > 1) {
        const int64_t b0 = rnd((uint32_t)(nblk0 - 1)), to = (b0 + 1) * span0 + W;
        int64_t from = -1;
        for (uint32_t j : chain)
            if ((int64_t)j / span0 == b0) from = j;
        if (from >= 0 && to < c.n) {
            c.nxt[from] = (uint32_t)to;
            fill_level0(c);
            CHECK(compose_levels(c), "%s: a hop of %lld ticks from %lld raised no overflow", what, (long long)(to - from), (long long)from);
            ++g_trees;
        }
    }
}

int main()
{
    for (int W : {3, 4, 7})
        for (int span0 : {W, W + 2, 3 * W})
            for (int radix : {2, 3, 16})
                for (int nblk0 = 1; nblk0 <= 40; ++nblk0)
                    for (int packed = 0; packed < 2; ++packed)
                        for (int variant = 0; variant < 3; ++variant) run_case(W, span0, radix, nblk0, packed != 0, variant);
    for (int k = 0; k <= 3; ++k) CHECK(g_levels[k] > 0, "no tree of %d levels above level 0", k);
    printf("trees checked: %lld, failed checks: %lld\n", g_trees, g_failed);
    return g_failed ? 1 : 0;
}
