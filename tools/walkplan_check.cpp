// walkplan_check.cpp -- replays the lockstep window walk of finmlkit_amd/csrc/fmk_window.h on the host, from the header's own step
// plan (fmk_walk_plan, plain C++), for BLOCK 256, OPL 1 and 4 and every wave of the workgroup, over every window 1 .. 3 * slab + 2
// of the slabs 64, 100, 256 and 1300 (the smallest of these that leaves an unchecked body at OPL 4, whose reach is 831 words) and
// tiles of 1, 63, 64, 65, tile - 1 and tile outputs.  Per output and slab the steps an output takes are intervals of q, so they
// are followed as intervals: exhaustive, and quick.  It fails when
//   - an output below the tile's count does not take every position of its window exactly once, ascending;
//   - a step of the unchecked range indexes outside [0, len) for some lane (with or without an output);
//   - a wave with no element in a slab takes a step, or one with an element takes none.
//     g++ -O2 -o walkplan_check tools/walkplan_check.cpp && ./walkplan_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../finmlkit_amd/csrc/fmk_window.h"

static long long g_plans, g_failed;

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            if (g_failed++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                           \
    } while (0)

static void walk(int block, int opl, int slab, int64_t window, int64_t outputs)
{
    const int tile = block * opl, reach = (opl - 1) * block + 63;
    const int64_t span = window - 1 + outputs;
    std::vector<int64_t> next(tile, 0);                  // per output: the position its next element must have
    for (int64_t s0 = 0; s0 < span; s0 += slab) {
        const int len = (int)(span - s0 < slab ? span - s0 : slab);
        for (int wave0 = 0; wave0 < block; wave0 += 64) {
            const int64_t w0 = wave0 - s0;
            const fmk_walk_steps s = fmk_walk_plan(w0, window, len, reach);
            ++g_plans;
            // the words the wave's windows cover: w0 .. w0 + window - 1 + reach
            const bool some = w0 <= len - 1 && w0 + window - 1 + reach >= 0;
            CHECK(s.any == some, "any %d, block %d opl %d slab %d window %lld outputs %lld s0 %lld wave %d", (int)s.any, block, opl, slab,
                  (long long)window, (long long)outputs, (long long)s0, wave0);
            if (!s.any) continue;
            if (s.fa <= s.fb)
                CHECK(s.fa >= 0 && s.fb + reach <= len - 1, "unchecked words %d .. %d of %d, opl %d slab %d window %lld s0 %lld wave %d",
                      s.fa, s.fb + reach, len, opl, slab, (long long)window, (long long)s0, wave0);
            // the walk's three loops, in its order; {from, to, checked}
            const int range[3][3] = {{s.qlo, s.hb, 1}, {s.fa, s.fb, 0}, {s.fb + 1, s.qhi, 1}};
            for (int r = 0; r < opl; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int off = r * block + lane, o = r * block + wave0 + lane;
                    for (int k = 0; k < 3; ++k) {
                        int64_t a = range[k][0], b = range[k][1];
                        if (range[k][2]) {               // (unsigned)(q + off) < (unsigned)len
                            if (a < -off) a = -off;
                            if (b > len - 1 - off) b = len - 1 - off;
                        }
                        if (a > b) continue;
                        // word q + off is span element s0 + q + off = o + p: position p = q - w0 of output o
                        CHECK(a - w0 >= 0 && b - w0 < window, "positions %lld .. %lld of window %lld", (long long)(a - w0),
                              (long long)(b - w0), (long long)window);
                        if (o >= outputs) continue;      // a lane without an output: what it takes is dropped
                        CHECK(a - w0 == next[o], "output %d takes position %lld, not %lld: opl %d slab %d window %lld outputs %lld s0 %lld", o,
                              (long long)(a - w0), (long long)next[o], opl, slab, (long long)window, (long long)outputs, (long long)s0);
                        next[o] = b - w0 + 1;
                    }
                }
        }
    }
    for (int o = 0; o < tile && o < outputs; ++o)
        CHECK(next[o] == window, "output %d took %lld of %lld positions: opl %d slab %d outputs %lld", o, (long long)next[o],
              (long long)window, opl, slab, (long long)outputs);
}

int main()
{
    const int slabs[4] = {64, 100, 256, 1300}, opls[2] = {1, 4};
    for (int opl : opls)
        for (int slab : slabs) {
            const int tile = 256 * opl;
            const int counts[6] = {1, 63, 64, 65, tile - 1, tile};
            for (int64_t window = 1; window <= 3 * slab + 2; ++window)
                for (int outputs : counts) walk(256, opl, slab, window, outputs);
        }
    // the slab the kernels take (fmk_slab): what a full tile reads, at most FMK_SLAB_MAX
    CHECK(fmk_slab(1, 256) == 256 && fmk_slab(3841, 256) == 4096 && fmk_slab(3842, 256) == 4096 && fmk_slab(3073, 1024) == 4096 &&
              fmk_slab(3072, 1024) == 4095 && fmk_slab(((int64_t)1 << 31) - 1, 1024) == FMK_SLAB_MAX,
          "fmk_slab");
    printf("walk plans checked: %lld, failed checks: %lld\n", g_plans, g_failed);
    return g_failed ? 1 : 0;
}
