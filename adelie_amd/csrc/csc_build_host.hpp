// csc_build_host.hpp — host side of the designs kept sparse: plain C++, no HIP, so that tests/native/csc_build_main.cpp can
// run it as a stand-alone program under the address and undefined-behaviour sanitizers.  csc_validate_pair holds the checks
// adelie_hip_design_create_csc makes of its caller's two compressed forms, csc_offsets_from_counts the prefix sums of a device
// build (kernels_phased.hip, kernels_relu_sparse.hip).  Both return nullptr or a message (the caller raises it as a core_error).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace ahip {

// The compressed-column form (indptr, indices, values) and the compressed-row form (row_*) of one (n, p) matrix whose values
// take `value_bytes` (4 or 8) each; n, p > 0 and the two pointer arrays are not null.
inline const char* csc_validate_pair(const int64_t* indptr, const int32_t* indices, const void* values, const int64_t* row_indptr,
                                     const int32_t* row_indices, const void* row_values, int64_t n, int64_t p, size_t value_bytes) {
    if (indptr[0] != 0 || row_indptr[0] != 0) return "sparse(): indptr must start at 0.";
    for (int64_t j = 0; j < p; ++j)
        if (indptr[j + 1] < indptr[j]) return "sparse(): indptr must be non-decreasing.";
    for (int64_t i = 0; i < n; ++i)
        if (row_indptr[i + 1] < row_indptr[i]) return "sparse(): indptr must be non-decreasing.";
    const int64_t nnz = indptr[p];
    if (row_indptr[n] != nnz) return "sparse(): the two compressed forms must hold the same entries.";
    if (nnz > 0 && (!indices || !values || !row_indices || !row_values)) return "null argument.";
    for (int64_t j = 0; j < p; ++j) // rows ascending and distinct inside a column (scipy: sort_indices + sum_duplicates)
        for (int64_t k = indptr[j]; k < indptr[j + 1]; ++k) {
            if (indices[k] < 0 || indices[k] >= n) return "sparse(): row index out of range.";
            if (k > indptr[j] && indices[k] <= indices[k - 1]) return "sparse(): row indices must be sorted and distinct inside a column.";
        }
    if (p >= (int64_t(1) << 31)) return "number of columns must fit in int32.";
    // The two forms must hold the SAME entries: gradients read the column form, residual updates the row form, and an
    // inconsistent pair would make them disagree silently.  Columns ascending and distinct inside a row, the same number of
    // entries per column in both forms, and an order-independent checksum over (row, column, value bits).
    auto mix = [](uint64_t r, uint64_t c, uint64_t v) {
        uint64_t h = (r * 0x9E3779B97F4A7C15ull) ^ (c * 0xC2B2AE3D27D4EB4Full) ^ (v * 0x165667B19E3779F9ull);
        h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
        return h;
    };
    auto bits = [&](const void* vals, int64_t k) {
        uint64_t b = 0;
        std::memcpy(&b, static_cast<const char*>(vals) + size_t(k) * value_bytes, value_bytes);
        return b;
    };
    std::vector<int64_t> per_col(static_cast<size_t>(p), 0);
    uint64_t sum_r = 0, sum_c = 0;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = row_indptr[i]; k < row_indptr[i + 1]; ++k) {
            const int32_t c = row_indices[k];
            if (c < 0 || c >= p) return "sparse(): column index out of range.";
            if (k > row_indptr[i] && c <= row_indices[k - 1]) return "sparse(): column indices must be sorted and distinct inside a row.";
            ++per_col[size_t(c)];
            sum_r += mix(uint64_t(i), uint64_t(c), bits(row_values, k));
        }
    for (int64_t j = 0; j < p; ++j) {
        if (per_col[size_t(j)] != indptr[j + 1] - indptr[j]) return "sparse(): the two compressed forms must hold the same entries.";
        for (int64_t k = indptr[j]; k < indptr[j + 1]; ++k) sum_c += mix(uint64_t(indices[k]), uint64_t(j), bits(values, k));
    }
    if (sum_r != sum_c) return "sparse(): the two compressed forms must hold the same entries.";
    return nullptr;
}

// col_cnt: the entries per (column, tile), column-major over n_cols_counted columns of nt tiles (a column's segments are
// consecutive).  The build has n_cols_out columns, n_cols_counted or twice that: the second half repeats the counts of the first.
// Writes cptr (n_cols_out + 1), the segment starts col_pos (n_cols_out * nt), rptr (n + 1) from the per-row counts row_cnt
// (may be rptr + 1: the sum then runs in place) and the entry count *total.  The caller puts its name in front of the message.
inline const char* csc_offsets_from_counts(const int32_t* col_cnt, int64_t n_cols_counted, int64_t n_cols_out, int64_t nt,
                                           const int64_t* row_cnt, int64_t n, int64_t* cptr, int64_t* col_pos, int64_t* rptr,
                                           int64_t* total) {
    const size_t segs = size_t(n_cols_counted) * size_t(nt), psegs = size_t(n_cols_out) * size_t(nt);
    int64_t run = 0;
    for (size_t k = 0; k < psegs; ++k) {
        if (k % size_t(nt) == 0) cptr[k / size_t(nt)] = run;
        col_pos[k] = run;
        run += col_cnt[k % segs];
    }
    cptr[size_t(n_cols_out)] = run;
    rptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) rptr[size_t(i) + 1] = rptr[size_t(i)] + row_cnt[size_t(i)];
    *total = run;
    return rptr[size_t(n)] != run ? "the row and column counts of the build disagree." : nullptr;
}

} // namespace ahip
