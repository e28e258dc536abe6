// cov_csc_host.hpp — host side of the covariance matrix kept sparse (adelie_hip_design_create_cov_csc): plain C++, no HIP, so
// that tests/native/cov_csc_main.cpp can run it as a stand-alone program under the address and undefined-behaviour sanitizers.
// cov_csc_validate holds the checks the entry point makes of its caller's column-compressed form (the one-form half of
// csc_build_host.hpp's csc_validate_pair: a symmetric matrix needs no row form, so there is no pair to compare), and
// cov_csc_lanes / cov_csc_shape the launch shape of the kernels in kernels_cov_sparse.hip.  The messages are returned as
// nullptr or a string (the caller raises it as a core_error).
#pragma once
#include <cstddef>
#include <cstdint>

namespace ahip {

// The compressed-column form of a (p, p) matrix, p > 0 and indptr not null.  Values are not looked at (symmetry is the caller's
// word, as on the dense handle).
inline const char* cov_csc_validate(const int64_t* indptr, const int32_t* indices, const void* values, int64_t p) {
    if (p >= (int64_t(1) << 31)) return "number of columns must fit in int32.";
    if (indptr[0] != 0) return "sparse(): indptr must start at 0.";
    for (int64_t j = 0; j < p; ++j)
        if (indptr[j + 1] < indptr[j]) return "sparse(): indptr must be non-decreasing.";
    const int64_t nnz = indptr[p]; // the entry count
    if (nnz > 0 && (!indices || !values)) return "null argument.";
    for (int64_t j = 0; j < p; ++j) // rows ascending and distinct inside a column (scipy: sort_indices + sum_duplicates)
        for (int64_t k = indptr[j]; k < indptr[j + 1]; ++k) {
            if (indices[k] < 0 || indices[k] >= p) return "sparse(): row index out of range.";
            if (k > indptr[j] && indices[k] <= indices[k - 1]) return "sparse(): row indices must be sorted and distinct inside a column.";
        }
    return nullptr;
}

// Lanes of the group that walks one column: the stored entries are strided over the lanes and summed by a shuffle tree of
// log2(lanes) steps, so a lane should own a few entries before the tree is worth its steps.  Mean column count <= 8: 4 lanes
// (two entries each at the most on average), <= 64: 16 lanes, above: a whole wavefront.
inline int cov_csc_lanes(int64_t nnz, int64_t p) {
    const int64_t mean = p > 0 ? (nnz + p - 1) / p : 0;
    return mean <= 8 ? 4 : (mean <= 64 ? 16 : 64);
}

constexpr int kCovCscBlock = 256; // threads of a block of the column kernels

// One group of `lanes` lanes per column, 256 / lanes columns per block, the columns spread over grid.x (no 65535 cap: the x
// dimension takes 2^31 - 1 blocks and ncols < 2^31).  Column of (block, group) = block * cols_per_block + group, live when
// below ncols.
struct CovCscShape {
    int lanes, cols_per_block;
    int64_t blocks;
};
inline CovCscShape cov_csc_shape(int64_t ncols, int lanes) {
    CovCscShape sh;
    sh.lanes = lanes;
    sh.cols_per_block = kCovCscBlock / lanes;
    sh.blocks = (ncols + sh.cols_per_block - 1) / sh.cols_per_block;
    return sh;
}

} // namespace ahip
