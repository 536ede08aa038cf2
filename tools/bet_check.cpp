// bet_check.cpp -- bet sizing on the host, from the plain C++ of finmlkit_amd/csrc/fmk_bet_rule.h: the text the
// kernels of fmk_bet.hip compile, walked over a difference array by one thread.  Replays cases from standard input and prints what
// the library would return, bit for bit (tests/test_betsize_host.py compares with tests/_bet_ref.py):
//   path <n_events> <n> <step>        then n_events lines  <event_idx> <touch_idx> <signal>
//       -> "ok" and n lines  <value as 16 hex digits> <count>,  or  "refused spans|signals|concurrency <count>"
//   budget <n_events> <n>             then n_events lines  <event_idx> <touch_idx> <side>
//       -> "ok <Ml> <Ms>" and n lines  <m as 16 hex digits>,   or  "refused spans|concurrency <count>"
//   disc <count> <step>               then count lines  <value>
//       -> count lines  <discretised value as 16 hex digits>
// Floating-point numbers are read with strtod (C hex floats such as Python's float.hex() are exact).
//     g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o bet_check tools/bet_check.cpp
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../finmlkit_amd/csrc/fmk_bet_rule.h"

static uint64_t bits(double x)
{
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}

static bool read_double(double *x)
{
    char tok[128];
    if (scanf("%127s", tok) != 1) return false;
    char *end;
    *x = strtod(tok, &end);
    return end != tok && *end == 0;
}

static int run_path()
{
    long long ne, n;
    double step;
    if (scanf("%lld %lld", &ne, &n) != 2 || !read_double(&step)) return 2;
    if (ne < 1 || n < 1 || n > (1ll << 26) || !fmk_bet_step_ok(step)) return 2;
    std::vector<int64_t> ds((size_t)n, 0);
    std::vector<int32_t> dc((size_t)n, 0);
    long long bad = 0, bad_signal = 0;
    for (long long i = 0; i < ne; ++i) {
        long long s, t;
        double m;
        if (scanf("%lld %lld", &s, &t) != 2 || !read_double(&m)) return 2;
        if (s < 0 || t < s || t >= n) { ++bad; continue; }
        int64_t q;
        if (!fmk_bet_quantise(m, &q)) { ++bad_signal; continue; }
        if (t == s) continue;
        ds[(size_t)s] += q;
        ds[(size_t)t] -= q;
        dc[(size_t)s] += 1;
        dc[(size_t)t] -= 1;
    }
    if (bad) { printf("refused spans %lld\n", bad); return 0; }
    if (bad_signal) { printf("refused signals %lld\n", bad_signal); return 0; }
    std::vector<double> v((size_t)n);
    std::vector<int32_t> c((size_t)n);
    FmkBetAcc run = {0, 0, 0};
    int32_t top = 0;
    for (long long j = 0; j < n; ++j) {
        run = fmk_bet_combine(run, FmkBetAcc{ds[(size_t)j], dc[(size_t)j], 0});
        c[(size_t)j] = run.c;
        top = run.c > top ? run.c : top;
        v[(size_t)j] = fmk_bet_discretise(fmk_bet_value(run.s, run.c), step);
    }
    if (top > FMK_BET_MAX_CONC) { printf("refused concurrency %d\n", top); return 0; }
    printf("ok\n");
    for (long long j = 0; j < n; ++j) printf("%016" PRIx64 " %d\n", bits(v[(size_t)j]), c[(size_t)j]);
    return 0;
}

static int run_budget()
{
    long long ne, n;
    if (scanf("%lld %lld", &ne, &n) != 2 || ne < 1 || n < 1 || n > (1ll << 26)) return 2;
    std::vector<int32_t> dl((size_t)n, 0), dsh((size_t)n, 0);
    long long bad = 0;
    for (long long i = 0; i < ne; ++i) {
        long long s, t;
        int side;
        if (scanf("%lld %lld %d", &s, &t, &side) != 3) return 2;
        if (s < 0 || t < s || t >= n) { ++bad; continue; }
        if (t == s || side == 0) continue;
        std::vector<int32_t> &d = side > 0 ? dl : dsh;
        d[(size_t)s] += 1;
        d[(size_t)t] -= 1;
    }
    if (bad) { printf("refused spans %lld\n", bad); return 0; }
    std::vector<FmkBetSides> at((size_t)n);
    FmkBetSides run = {0, 0};
    int32_t ml = 0, ms = 0;
    for (long long j = 0; j < n; ++j) {
        run = fmk_bet_sides_combine(run, FmkBetSides{dl[(size_t)j], dsh[(size_t)j]});
        at[(size_t)j] = run;
        ml = run.l > ml ? run.l : ml;
        ms = run.s > ms ? run.s : ms;
    }
    if (ml > FMK_BET_MAX_CONC || ms > FMK_BET_MAX_CONC) { printf("refused concurrency %d\n", ml > ms ? ml : ms); return 0; }
    printf("ok %d %d\n", ml, ms);
    for (long long j = 0; j < n; ++j) printf("%016" PRIx64 "\n", bits(fmk_bet_budget_value(at[(size_t)j].l, at[(size_t)j].s, ml, ms)));
    return 0;
}

static int run_disc()
{
    long long count;
    double step;
    if (scanf("%lld", &count) != 1 || !read_double(&step) || count < 0 || !fmk_bet_step_ok(step)) return 2;
    for (long long i = 0; i < count; ++i) {
        double v;
        if (!read_double(&v)) return 2;
        printf("%016" PRIx64 "\n", bits(fmk_bet_discretise(v, step)));
    }
    return 0;
}

int main()
{
    char what[32];
    long long cases = 0;
    while (scanf("%31s", what) == 1) {
        int rc;
        if (!strcmp(what, "path")) rc = run_path();
        else if (!strcmp(what, "budget")) rc = run_budget();
        else if (!strcmp(what, "disc")) rc = run_disc();
        else rc = 2;
        if (rc) { fprintf(stderr, "bet_check: malformed case %lld (%s)\n", cases, what); return rc; }
        ++cases;
    }
    fprintf(stderr, "bet_check: %lld cases\n", cases);
    return 0;
}
