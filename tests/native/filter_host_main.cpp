// Stand-alone check of the host-side decisions of the filtered invariance sweep (adelie_amd/csrc/filter_host.hpp), built with
// -fsanitize=address,undefined by tests/test_filter_host.py.  Replays a path-like sequence of screen sizes through the
// threshold rule and checks it against a direct restatement; exits non-zero on the first disagreement.
#include "../../adelie_amd/csrc/filter_host.hpp"
#include <cstdio>
#include <limits>
#include <random>

using namespace ahip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    // the thresholds
    FilterRule f;
    f.alpha = 0.5; f.lm = 2.0; f.lm_next = 1.8; f.G = 10000; f.screen_size = 100; f.n_new_active = 5;
    CHECK(filter_tstar(f) == 0);                                   // no valid screen_thr under the pivot rule
    f.thr_valid = true; f.screen_thr = 0.3; f.thr_count = 600;
    CHECK(filter_tstar(f) == 0.3);                                 // need = 110 + 7 + 100 + 2 = 219 <= 0.97 * 600
    CHECK(pivot_need(100, 5, 10000, 0.1, 1, 1.25) == 219);
    f.screen_thr = 5.0;
    CHECK(filter_tstar(f) == 0.5 * 1.8);                           // alpha * lm_next is the smallest
    f.thr_count = 220;
    CHECK(filter_tstar(f) == 0);                                   // 219 > 0.97 * 220: screen() would sort all G scores
    f.n_new_active = 0;
    CHECK(filter_tstar(f) == 0.9);                                 // ... unless it skips the pivot search altogether
    f.n_new_active = 5; f.thr_count = 100000; f.G = 800;
    CHECK(filter_tstar(f) == 0);                                   // need * 4 >= G
    f.G = 10000; f.lm_next = 0;
    CHECK(filter_tstar(f) == 0);                                   // last lambda: the state handed back is exact
    f.lm_next = 1.8; f.alpha = 0;
    CHECK(filter_tstar(f) == 0);
    f.alpha = 0.5; f.screen_rule = kFilterRuleStrong; f.thr_valid = false;
    CHECK(filter_tstar(f) == (2 * 1.8 - 2.0) * 0.5);
    f.lm_next = 0.9;
    CHECK(filter_tstar(f) == 0);                                   // 2 lm_next - lm <= 0: everything is compared with <= 0
    f.screen_rule = 7;
    CHECK(filter_tstar(f) == 0);
    f.screen_rule = kFilterRulePivot; f.thr_valid = true; f.lm_next = 1.8; f.screen_thr = std::numeric_limits<double>::infinity();
    CHECK(filter_tstar(f) == 0.9);
    f.screen_thr = std::numeric_limits<double>::quiet_NaN();
    CHECK(!(filter_tstar(f) > 0.9));                               // (min with NaN keeps a finite value or gives 0, never more)

    // random sweeps: tstar never exceeds any threshold a later decision uses, and is 0 exactly when the rule says so
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> u(0, 1);
    for (int it = 0; it < 20000; ++it) {
        FilterRule g;
        g.screen_rule = it & 1;
        g.alpha = u(rng); g.lm = 3 * u(rng); g.lm_next = g.lm * (0.4 + 0.6 * u(rng));
        g.thr_valid = u(rng) < 0.8; g.screen_thr = u(rng); g.G = 1 + int64_t(20000 * u(rng));
        g.screen_size = int64_t(double(g.G) * u(rng) * 0.5); g.n_new_active = int64_t(50 * u(rng));
        g.thr_count = int64_t(double(g.G) * u(rng)); g.subset_min = 1 + int64_t(5 * u(rng));
        const double t = filter_tstar(g);
        CHECK(t >= 0);
        if (t > 0) {
            CHECK(t <= g.alpha * g.lm && t <= g.alpha * g.lm_next);
            if (g.screen_rule == kFilterRuleStrong) CHECK(t <= (2 * g.lm_next - g.lm) * g.alpha);
            else {
                CHECK(g.thr_valid && t <= g.screen_thr);
                if (g.n_new_active > 0) {
                    const int64_t need = pivot_need(g.screen_size, g.n_new_active, g.G, g.subset_ratio, g.subset_min, g.slack_ratio);
                    CHECK(need * 4 < g.G && double(need) <= 0.97 * double(g.thr_count));
                }
            }
        }
    }

    // the list of unpenalized columns and the follow-up of the flags
    std::vector<int64_t> groups{0, 4, 8, 9}, sizes{4, 4, 1, 3};
    std::vector<double> pen{1.0, 0.0, -1.0, 2.0};
    const std::vector<int32_t> c = filter_unpenalized_cols(groups, sizes, pen);
    CHECK(c.size() == 5 && c[0] == 4 && c[3] == 7 && c[4] == 8);
    CHECK(filter_unpenalized_cols(std::vector<int64_t>{}, std::vector<int64_t>{}, std::vector<double>{}).empty());
    CHECK(!filter_follow_up(0).refill && !filter_follow_up(0).retire);
    CHECK(filter_follow_up(kFilterOverflow).refill && !filter_follow_up(kFilterOverflow).retire);
    CHECK(filter_follow_up(kFilterStale).refill && filter_follow_up(kFilterStale).retire);
    CHECK(filter_follow_up(3).refill && filter_follow_up(3).retire);
    CHECK(filter_list_cap(37) == 1024 && filter_list_cap(10000) == 2500 && filter_list_cap(4100) == 1025);
    std::printf(fails ? "filter_host: %d check(s) FAILED\n" : "filter_host: ok\n", fails);
    return fails ? 1 : 0;
}
