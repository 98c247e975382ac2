// Stand-alone check of rr::mark_inpass_headwaters' coefficient rule (tests/test_inpass_eligibility.py compiles this file with
// river_route_amd/csrc/rr_plan.cpp and runs it): a headwater's c1row cannot be set through the C ABI, so the rule is exercised on the
// planner's own function.  Prints one line per case: "<name> <eligible flags of the positions that own reaches 0..n-1> <count>".
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../river_route_amd/csrc/rr_plan.hpp"

int main()
{
    // reaches 0..7: isolated (headwater and outlet at once); 8 -> 9: a headwater and the reach it flows into
    const std::vector<int32_t> down = {-1, -1, -1, -1, -1, -1, -1, -1, 9, -1};
    const std::vector<int32_t> lag_of = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    const int n = (int)down.size();
    rr::TilePlan T;
    rr::build_tile_plan(down, lag_of, 512, T);
    if (!T.ok || T.np != n) { std::printf("plan failed\n"); return 1; }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    auto run = [&](const char *name, const std::vector<double> *by_reach) {      // by_reach: {c1row, c2, c3} per REACH, or null
        std::vector<double> coef;
        if (by_reach) {
            coef.assign(3 * (size_t)T.np, 0.0);
            for (int i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) coef[3 * (size_t)T.inv[i] + k] = (*by_reach)[3 * i + k];
        }
        std::vector<uint8_t> elig;
        int64_t counts[4];
        const int64_t c = rr::mark_inpass_headwaters(T, T.lag, 0, elig, counts, by_reach ? coef.data() : nullptr);
        std::printf("%s ", name);
        for (int i = 0; i < n; ++i) std::printf("%d", (int)elig[T.inv[i]]);
        std::printf(" %lld %lld %lld\n", (long long)c, (long long)counts[0], (long long)counts[1]);
    };
    run("structure", nullptr);
    std::vector<double> plain(3 * (size_t)n);
    for (int i = 0; i < n; ++i) { plain[3 * i] = 0.0; plain[3 * i + 1] = 0.25; plain[3 * i + 2] = 0.5; }
    plain[3 * 9] = 0.3;      // the reach with an upstream reach has a weight
    run("plain", &plain);
    std::vector<double> odd(plain);
    odd[3 * 0 + 1] = inf;                                             // c2 +inf
    odd[3 * 1 + 1] = -inf;                                            // c2 -inf
    odd[3 * 2 + 1] = nan;                                             // c2 NaN
    odd[3 * 3 + 0] = -0.0;                                            // c1row -0.0
    odd[3 * 4 + 0] = 1.0;                                             // c1row not a zero
    odd[3 * 5 + 1] = -0.75;                                           // c2 negative, finite: eligible
    odd[3 * 6 + 1] = std::numeric_limits<double>::denorm_min();       // c2 subnormal: eligible
    odd[3 * 7 + 1] = -0.0;                                            // c2 -0.0: eligible
    odd[3 * 8 + 2] = inf;                                             // c3 is not part of the rule: eligible
    run("odd", &odd);
    return 0;
}
