// pin_rows_host.hpp — host side of the one-launch pin path: the CSR rows of `betas` from the snapshot block.
//
// The path kernel (kernels_cd_pin.hip) leaves, per solved lambda l, the nv screen coefficients and the active size.  The
// active set of a pin solve only grows, and only by appending, so the active groups of row l are the first active_size[l]
// entries of the FINAL active_set.  A row lists the coefficients of its active groups, zeros included, with the groups sorted by
// their first column: what sparsify_active_beta writes through active_order (solver_gaussian_pin_naive.hpp:359-394).
// Plain C++ (no HIP): tests/native/pin_rows_main.cpp builds it on its own under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <stdexcept>
#include <vector>

namespace ahip {

struct PinLayout {
    const int64_t* screen_set;    // [ns] group of each screen position
    const int64_t* screen_begins; // [ns] first screen value of each screen position
    const int64_t* groups;        // [G] first column of each group
    const int64_t* group_sizes;   // [G]
    int64_t ns, nv, G;
};

// positions 0..count-1 of active_set, ordered by the first column of their groups (active_order of the reference)
inline std::vector<int64_t> pin_active_order(const PinLayout& lay, const int64_t* active_set, int64_t count) {
    std::vector<int64_t> order(static_cast<size_t>(count));
    std::iota(order.begin(), order.end(), int64_t(0));
    std::sort(order.begin(), order.end(), [&](int64_t i, int64_t j) {
        return lay.groups[lay.screen_set[active_set[i]]] < lay.groups[lay.screen_set[active_set[j]]];
    });
    return order;
}

// active_begins of the reference: offsets of the active groups' coefficients, in activation order
inline std::vector<int64_t> pin_active_begins(const PinLayout& lay, const int64_t* active_set, int64_t count) {
    std::vector<int64_t> b(static_cast<size_t>(count));
    int64_t off = 0;
    for (int64_t i = 0; i < count; ++i) {
        b[size_t(i)] = off;
        off += lay.group_sizes[lay.screen_set[active_set[i]]];
    }
    return b;
}

// rows [0, n_rows) of the path: snap is (n_rows, nv) row-major, row_active[l] the active size after lambda l (non-decreasing,
// at most n_active).  Appends one (indices, values) pair per row.
template <class T>
void pin_assemble_rows(const PinLayout& lay, const T* snap, const int32_t* row_active, int64_t n_rows, const int64_t* active_set,
                       int64_t n_active, std::vector<std::vector<int64_t>>& rows_idx, std::vector<std::vector<T>>& rows_val) {
    for (int64_t i = 0; i < n_active; ++i)
        if (active_set[i] < 0 || active_set[i] >= lay.ns) throw std::runtime_error("pin rows: active_set entry outside the screen set.");
    int64_t prev = 0;
    std::vector<int64_t> order;
    for (int64_t l = 0; l < n_rows; ++l) {
        const int64_t a = row_active[l];
        if (a < prev || a > n_active) throw std::runtime_error("pin rows: active sizes must be non-decreasing and within the active set.");
        if (a != prev || l == 0) order = pin_active_order(lay, active_set, a);
        prev = a;
        std::vector<int64_t> ri;
        std::vector<T> rv;
        const T* row = snap + l * lay.nv;
        for (int64_t k : order) {
            const int64_t ss = active_set[k], g = lay.screen_set[ss], b = lay.screen_begins[ss];
            for (int64_t t = 0; t < lay.group_sizes[g]; ++t) {
                ri.push_back(lay.groups[g] + t);
                rv.push_back(row[b + t]);
            }
        }
        rows_idx.emplace_back(std::move(ri));
        rows_val.emplace_back(std::move(rv));
    }
}

} // namespace ahip
