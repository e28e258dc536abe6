// pin_rows_main.cpp — the CSR assembly of a pin path's rows (adelie_amd/csrc/pin_rows_host.hpp) against rows written out by
// hand, as a stand-alone program (tests/test_pin_rows_host.py builds it with the address and undefined-behaviour sanitizers).
#include "../../adelie_amd/csrc/pin_rows_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace ahip;

static void fail(const char* what) {
    std::printf("pin_rows: FAIL %s\n", what);
    std::exit(1);
}

template <class T>
static void expect_row(const std::vector<std::vector<int64_t>>& ri, const std::vector<std::vector<T>>& rv, size_t l,
                       std::vector<int64_t> idx, std::vector<T> val, const char* what) {
    if (l >= ri.size() || ri[l] != idx || rv[l] != val) fail(what);
}

template <class T>
static void run() {
    // 6 groups on 10 columns: sizes 1, 3, 1, 3, 1, 1 -> first columns 0, 1, 4, 5, 8, 9
    const std::vector<int64_t> groups{0, 1, 4, 5, 8, 9}, sizes{1, 3, 1, 3, 1, 1};
    // screen set given out of column order: groups 3, 0, 5, 1  -> screen values [0..3) [3] [4] [5..8)
    const std::vector<int64_t> screen_set{3, 0, 5, 1}, screen_begins{0, 3, 4, 5};
    PinLayout lay{screen_set.data(), screen_begins.data(), groups.data(), sizes.data(), 4, 8, 6};
    // the active set grew in the order: screen position 2 (group 5, column 9), 0 (group 3, columns 5-7), 3 (group 1, columns 1-3)
    const std::vector<int64_t> active_set{2, 0, 3};
    // 4 rows of an L = 6 path were solved (n_solved < L): active sizes 0, 1, 3, 3
    const std::vector<int32_t> row_active{0, 1, 3, 3};
    const std::vector<T> snap{
        0, 0, 0,  0,  0,  0, 0, 0,    // row 0: nothing active
        0, 0, 0,  0,  7,  0, 0, 0,    // row 1: group 5 only
        0, 0, 0,  0,  8,  1, 2, 3,    // row 2: group 3 active but all zero at this row (stored zeros), group 1 = 1 2 3
        4, 5, 6,  0,  9,  1, 0, 3,    // row 3
    };
    std::vector<std::vector<int64_t>> ri;
    std::vector<std::vector<T>> rv;
    pin_assemble_rows<T>(lay, snap.data(), row_active.data(), 4, active_set.data(), 3, ri, rv);
    if (ri.size() != 4 || rv.size() != 4) fail("row count");
    expect_row<T>(ri, rv, 0, {}, {}, "row with no active group");
    expect_row<T>(ri, rv, 1, {9}, {7}, "one group of one");
    expect_row<T>(ri, rv, 2, {1, 2, 3, 5, 6, 7, 9}, {1, 2, 3, 0, 0, 0, 8}, "active group whose coefficients are all zero");
    expect_row<T>(ri, rv, 3, {1, 2, 3, 5, 6, 7, 9}, {1, 0, 3, 4, 5, 6, 9}, "sizes 1 and 3 mixed, out of column order");
    // screen position 1 (group 0) never became active: its value (column 0) is in no row
    for (auto& r : ri)
        for (int64_t c : r)
            if (c == 0) fail("inactive screen group stored");
    // appending: a second call adds to the rows that are there
    pin_assemble_rows<T>(lay, snap.data(), row_active.data(), 1, active_set.data(), 3, ri, rv);
    if (ri.size() != 5 || !ri[4].empty()) fail("append");
    // order and begins of the final active set
    if (pin_active_order(lay, active_set.data(), 3) != std::vector<int64_t>{2, 1, 0}) fail("active_order");
    if (pin_active_begins(lay, active_set.data(), 3) != std::vector<int64_t>{0, 1, 4}) fail("active_begins");
    if (!pin_active_order(lay, active_set.data(), 0).empty()) fail("empty active_order");
    // refusals: an active size that shrinks, one beyond the active set, an active entry outside the screen set
    auto throws = [&](const std::vector<int32_t>& ra, const std::vector<int64_t>& as) {
        std::vector<std::vector<int64_t>> a;
        std::vector<std::vector<T>> b;
        try {
            pin_assemble_rows<T>(lay, snap.data(), ra.data(), int64_t(ra.size()), as.data(), int64_t(as.size()), a, b);
        } catch (const std::runtime_error&) {
            return true;
        }
        return false;
    };
    if (!throws({1, 0}, active_set)) fail("shrinking active size accepted");
    if (!throws({4}, active_set)) fail("active size beyond the active set accepted");
    if (!throws({1}, {4})) fail("active entry outside the screen set accepted");
    if (throws({0, 3}, active_set)) fail("valid rows refused");
}

int main() {
    run<double>();
    run<float>();
    std::printf("pin_rows: ok\n");
    return 0;
}
