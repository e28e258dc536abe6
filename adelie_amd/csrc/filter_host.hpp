// filter_host.hpp — the host-side decisions of the filtered invariance sweep (solver_screen.hpp, kernels_filter.hip), free of
// any device call so that they also build into a stand-alone program (tests/native/filter_host_main.cpp, run under the address
// and undefined-behaviour sanitizers by tests/test_filter_host.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ahip {

constexpr int kFilterRuleStrong = 0, kFilterRulePivot = 1; // ADELIE_HIP_SCREEN_STRONG / _PIVOT

// `need` of the pivot rule's next screen() call (solver_screen.hpp, screen()): the positions of the sorted scores it may read
inline int64_t pivot_need(int64_t old_size, int64_t n_new_active, int64_t G, double subset_ratio, int64_t subset_min,
                          double slack_ratio) {
    const int64_t subset_size =
        std::min<int64_t>(std::max<int64_t>(int64_t(double(old_size) * (1 + subset_ratio)), subset_min), G);
    return subset_size + int64_t(std::ceil(slack_ratio * double(n_new_active))) + old_size + 2;
}

struct FilterRule {
    int screen_rule = kFilterRulePivot;
    double alpha = 1, lm = 0, lm_next = 0; // the lambda of the sweep and the one that follows if KKT passes (0: none)
    bool thr_valid = false;                // pivot rule: screen_thr and how many scores lay at or above it when it was set
    double screen_thr = 0;
    int64_t thr_count = 0;
    int64_t G = 0, screen_size = 0, n_new_active = 0;
    double subset_ratio = 0.1, slack_ratio = 1.25;
    int64_t subset_min = 1;
};

// The smallest threshold a decision after the sweep at `lm` can compare a group outside the screen set with, or 0 when the
// sweep has to be the full one: kkt() compares with alpha*lm, the two fallback loops of screen() with alpha*lm_next, the strong
// rule with (2 lm_next - lm) alpha, the pivot rule's threshold pass with screen_thr.  Under the pivot rule a screen() that
// will sort all G scores (need*4 >= G, or more positions wanted than lay above screen_thr: 3 % margin) needs every value.
inline double filter_tstar(const FilterRule& f) {
    if (!(f.lm_next > 0) || !(f.lm > 0) || !(f.alpha > 0)) return 0;
    double tstar = std::min(f.alpha * f.lm, f.alpha * f.lm_next);
    if (f.screen_rule == kFilterRuleStrong) {
        tstar = std::min(tstar, (2 * f.lm_next - f.lm) * f.alpha);
    } else if (f.screen_rule == kFilterRulePivot) {
        if (!f.thr_valid) return 0;
        if (f.n_new_active > 0) {
            const int64_t need = pivot_need(f.screen_size, f.n_new_active, f.G, f.subset_ratio, f.subset_min, f.slack_ratio);
            if (!(need * 4 < f.G) || double(need) > 0.97 * double(f.thr_count)) return 0;
        }
        tstar = std::min(tstar, f.screen_thr);
    } else {
        return 0;
    }
    return (tstar > 0 && std::isfinite(tstar)) ? tstar : 0;
}

// columns of the groups without a penalty: swept exactly by every filtered sweep
template <class I, class T>
inline std::vector<int32_t> filter_unpenalized_cols(const std::vector<I>& groups, const std::vector<I>& group_sizes,
                                                    const std::vector<T>& penalty) {
    std::vector<int32_t> c;
    for (size_t g = 0; g < groups.size(); ++g)
        if (!(penalty[g] > 0))
            for (I t = 0; t < group_sizes[g]; ++t) c.push_back(int32_t(groups[g] + t));
    return c;
}

constexpr int32_t kFilterOverflow = 1, kFilterStale = 2; // flags of a filtered sweep (filter_classify_kernel, shadow_guard)
struct FilterFollowUp {
    bool refill;     // run the full sweep on the same residual
    bool retire;     // no later sweep of this design takes the shadow
};
inline FilterFollowUp filter_follow_up(int32_t flags) {
    return FilterFollowUp{(flags & (kFilterOverflow | kFilterStale)) != 0, (flags & kFilterStale) != 0};
}
inline int64_t filter_list_cap(int64_t p) { return std::max<int64_t>(1024, p / 4); }

} // namespace ahip
