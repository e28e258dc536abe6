// cd_screen_host.hpp — the two host-only decisions of the screen-set coordinate descents (cd_screen_driver.hpp): which
// coordinates a KKT round admits, and whether a caller's warm start is one the solver could have left.  No HIP here: the
// functions run as a stand-alone program under the sanitizers (tests/native/cd_screen_main.cpp, tests/test_cd_screen_host.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace ahip {

// kkt_screen's admission: the coordinates by descending violation (std::stable_sort from 0..p-1, so ties go to the lower index;
// the reference's std::sort leaves them open), non-members with viol > 0 appended to `added` until there are `kappa` of them.
// Returns kkt_passed: false as soon as one such coordinate is seen, admitted or not.
template <class T>
bool cd_screen_admit(const T* viols, int64_t p, const uint8_t* is_screen, int64_t kappa, std::vector<int64_t>& added) {
    std::vector<int64_t> order(static_cast<size_t>(p));
    std::iota(order.begin(), order.end(), int64_t(0));
    std::stable_sort(order.begin(), order.end(), [&](int64_t i, int64_t j) { return viols[size_t(i)] > viols[size_t(j)]; });
    added.clear();
    bool kkt_passed = true;
    for (int64_t t = 0; t < p; ++t) {
        const int64_t k = order[size_t(t)];
        if (is_screen[size_t(k)] || viols[size_t(k)] <= T(0)) continue;
        kkt_passed = false;
        if (int64_t(added.size()) >= kappa) break;
        added.push_back(k);
    }
    return kkt_passed;
}

// distinct members in range; the active set inside the screen set (what the solver itself maintains).  Null, or the message
// of the first rule broken.
inline const char* cd_screen_warm_start_error(const int64_t* screen_set, int64_t screen_set_size, const int64_t* active_set,
                                              int64_t active_set_size, int64_t p, const char* screen_msg, const char* active_msg) {
    std::vector<uint8_t> seen(size_t(p), 0);
    for (int64_t i = 0; i < screen_set_size; ++i) {
        const int64_t j = screen_set[i];
        if (j < 0 || j >= p || seen[size_t(j)]) return screen_msg;
        seen[size_t(j)] = 1;
    }
    for (int64_t i = 0; i < active_set_size; ++i) {
        const int64_t j = active_set[i];
        if (j < 0 || j >= p || seen[size_t(j)] != 1) return active_msg;
        seen[size_t(j)] = 2;
    }
    return nullptr;
}

} // namespace ahip
