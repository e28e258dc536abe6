// screen_reads_host.hpp — what the pivot rule of screen() reads of the sorted scores, and the depth rule built on it: the
// threshold of the next filtered invariance sweep is put at the depth the rule is predicted to read, not at the worst case
// `need` (filter_host.hpp: pivot_need).  Free of any device call, like filter_host.hpp, so that it builds into a stand-alone
// program (tests/native/screen_reads_main.cpp, run under the address and undefined-behaviour sanitizers by
// tests/test_screen_reads_host.py).
#pragma once
#include "filter_host.hpp"
#include <limits>
#include <utility>

namespace ahip {

// optimization/search_pivot.hpp:7-62
template <class T>
inline int search_pivot(const std::vector<T>& x, const std::vector<T>& y, std::vector<T>& mses) {
    const int64_t m = int64_t(x.size());
    if (m <= 0) return -1;
    mses[0] = std::numeric_limits<T>::infinity();
    if (m == 1) return 0;
    T y_mean = 0;
    for (int64_t i = 0; i < m; ++i) y_mean += y[i];
    y_mean /= T(m);
    T x_sum = x[0], xsq_sum = x[0] * x[0], y_sum = y[0], yx_sum = y[0] * x[0], min_mse = mses[0];
    int argmin = 0;
    for (int64_t i = 1; i < m; ++i) {
        x_sum += x[i];
        xsq_sum += x[i] * x[i];
        y_sum += y[i];
        yx_sum += y[i] * x[i];
        const T t_bar = ((i + 1) * x[i] - x_sum) / m;
        const T var_t = ((i + 1) * x[i] * x[i] - 2 * x[i] * x_sum + xsq_sum - m * t_bar * t_bar);
        const T cov_ty = (x[i] * (y_sum - (i + 1) * y_mean) - (yx_sum - y_mean * x_sum));
        const T b1 = cov_ty / var_t;
        mses[i] = -b1 * b1 * var_t;
        if (mses[i] < min_mse) { argmin = int(i); min_mse = mses[i]; }
    }
    return argmin;
}

// The pivot rule's reading of the sorted scores (solver_base.hpp:320-360).  `top`: the M largest of the G (score, group) pairs
// in ascending order, so that position ii of the full order is top[ii - (G - M)].  The rule reads the `subset_size` largest
// scores for the pivot search, every group at or above the pivot, and below it as many more positions as it takes to find
// slack * n_new_active groups outside the screen set.  `append`: the groups it adds, in its order.  `reads`: the positions it
// read, counted from the top.  `sufficient` is false when a read would go below position G - M; `append` is then not to be
// used.  Same groups in the same order for every M that is sufficient.
struct PivotRead {
    int64_t reads = 0;
    bool sufficient = true;
};
template <class T, class I, class InScreen>
inline PivotRead pivot_read(const std::pair<T, I>* top, int64_t M, int64_t G, int64_t subset_size, T slack_ratio,
                            int64_t n_new_active, InScreen&& in_screen, std::vector<I>& append) {
    PivotRead r;
    append.clear();
    const int64_t base = G - M;
    if (subset_size > M) {
        r.sufficient = false;
        return r;
    }
    const size_t ns = size_t(subset_size);
    std::vector<T> sub(ns), mses(ns), ind(ns);
    for (int64_t i = 0; i < subset_size; ++i) {
        sub[size_t(i)] = top[G - subset_size + i - base].first;
        ind[size_t(i)] = T(i);
    }
    const int64_t pivot_idx = search_pivot(ind, sub, mses);
    const int64_t full_pivot_idx = G - subset_size + pivot_idx;
    if (full_pivot_idx < base) { // (no subset at all and nothing collected: the rule reads the top position)
        r.sufficient = false;
        return r;
    }
    r.reads = std::max<int64_t>(subset_size, G - full_pivot_idx);
    for (int64_t ii = G - 1; ii >= full_pivot_idx; --ii) {
        const I i = top[ii - base].second;
        if (in_screen(i)) continue;
        append.push_back(i);
    }
    int64_t count = 0;
    for (int64_t ii = full_pivot_idx - 1; ii >= 0; --ii) {
        if (count >= slack_ratio * n_new_active) break;
        if (ii < base) {
            r.sufficient = false;
            return r;
        }
        r.reads = std::max<int64_t>(r.reads, G - ii);
        const I i = top[ii - base].second;
        if (in_screen(i)) continue;
        append.push_back(i);
        ++count;
    }
    return r;
}

// ---- the depth rule (ADELIE_HIP_FILTER_DEPTH) -------------------------------------------------------------------------------
// After every screen() call the host holds a score for every group (exact, or derived from the shadow and then below the
// sweep's threshold), so the threshold of the next sweep can be put at any depth D of them with nth_element.  D follows the
// positions the next call is predicted to read; a call whose threshold pass is not `sufficient` sorts all G scores after the
// full sweep, as the parent's rule does, so D is a matter of speed only.

// The next call's reads: its subset (known: it follows from the screen set as it stands) plus the walk below the subset that
// the last call took, or, before any call has read, twice the groups a call is asked to find.
constexpr double kDepthMargin = 0.25; // m and c of D: profiles/filter_depth.txt (zero short passes on the headline path)
constexpr int64_t kDepthExtra = 16;
inline int64_t pivot_subset_size(int64_t screen_size, int64_t G, double subset_ratio, int64_t subset_min) {
    return std::min<int64_t>(std::max<int64_t>(int64_t(double(screen_size) * (1 + subset_ratio)), subset_min), G);
}
inline int64_t predict_reads(int64_t subset_next, int64_t last_reads, int64_t last_subset, int64_t n_new_active,
                             double slack_ratio) {
    const int64_t walk = last_reads > 0 ? std::max<int64_t>(last_reads - last_subset, 0)
                                        : 2 * int64_t(std::ceil(slack_ratio * double(std::max<int64_t>(n_new_active, 1))));
    return subset_next + walk;
}
// D = min(G, ceil((1 + m) reads_pred) + c); m <= 0 (the test hook) drops c as well: D is the prediction itself
inline int64_t filter_depth(int64_t G, int64_t reads_pred, double m) {
    if (G <= 0) return 0;
    const double d = std::ceil((1 + std::max(m, 0.0)) * double(std::max<int64_t>(reads_pred, 0)));
    const int64_t D = (d < double(G) ? int64_t(d) : G) + (m > 0 ? kDepthExtra : 0);
    return std::max<int64_t>(1, std::min<int64_t>(G, D));
}
// the D-th largest of `scores` (reordered in place); D in [1, scores.size()]
template <class T>
inline T depth_score(std::vector<T>& scores, int64_t D) {
    const int64_t G = int64_t(scores.size());
    if (G == 0) return std::numeric_limits<T>::infinity();
    D = std::max<int64_t>(1, std::min<int64_t>(D, G));
    std::nth_element(scores.begin(), scores.begin() + (D - 1), scores.end(), std::greater<T>());
    return scores[size_t(D - 1)];
}

// The same value with `scores` left as they are: when at least D of them lie at or above `lo_hint` (a guess, such as a little
// under the last threshold), the D-th largest is among those and nth_element runs on them alone, a fraction of the G scores.
template <class T>
inline T depth_score_hinted(const std::vector<T>& scores, int64_t D, T lo_hint, std::vector<T>& scratch) {
    const int64_t G = int64_t(scores.size());
    D = std::max<int64_t>(1, std::min<int64_t>(D, G));
    scratch.clear();
    if (lo_hint > 0)
        for (const T s : scores)
            if (s >= lo_hint) scratch.push_back(s);
    if (int64_t(scratch.size()) < D) scratch = scores;
    return depth_score(scratch, D);
}

// Whether a sweep is filtered, in bytes: the columns read in f64 (screen, unpenalised, predicted open) and the shadow's
// elements of the columns it does not skip, against the fraction rho of the 8 n p bytes of the full sweep.
// rho, measured on the headline (profiles/filter_depth.txt): a filtered sweep through the 16-bit copy takes 462 us + 0.128 us per
// exact column (they go one per workgroup) and meets sweep_kernel's 1153 us at 5400 of 10000 columns, 0.79 of the bytes; with
// every sweep below that filtered the path is no faster than with rho = 0.6, which keeps a fifth of the full sweep's time as
// the gain of the last sweep it admits.  With the pipelined 16-bit sweep the span is about 50 us shorter and that fifth is met
// at 0.67 of the bytes, but rho = 0.6, 0.65, 0.7 and 1 gave the same wall clock (profiles/shadow_q15_rate.txt): 0.6 stays.  A design under 2^28 bytes is not held to the rule: its sweeps are launch-bound (under
// 50 us either way) and the model has nothing to say about them.
#ifndef AHIP_FILTER_BYTES_RHO // (a compile-time variant for measuring the crossing: build.sh, AHIP_VARIANT / AHIP_EXTRA_FLAGS)
#define AHIP_FILTER_BYTES_RHO 0.6
#endif
constexpr double kFilterBytesRho = AHIP_FILTER_BYTES_RHO;
constexpr double kFilterBytesRuleMin = double(int64_t(1) << 28);
inline bool filter_bytes_eligible(int64_t exact_cols, int64_t n, int64_t p, int64_t skip_cols, double shadow_elem_bytes,
                                  double rho = kFilterBytesRho) {
    if (p <= 0 || n <= 0) return false;
    const double full = 8.0 * double(n) * double(p);
    if (full < kFilterBytesRuleMin) return true;
    const double bytes = double(n) * (8.0 * double(std::max<int64_t>(exact_cols, 0)) +
                                      shadow_elem_bytes * double(std::max<int64_t>(p - std::max<int64_t>(skip_cols, 0), 0)));
    return bytes < rho * full;
}
// the open list's capacity under the depth rule: late lambdas list more than filter_list_cap allows
inline int64_t filter_depth_list_cap(int64_t p) { return std::max<int64_t>(1024, p / 2); }

} // namespace ahip
