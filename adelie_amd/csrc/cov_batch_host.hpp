// cov_batch_host.hpp — host side of the lambda-batched covariance product (adelie_hip_design_cov_mul_batch: out[l, :] = v - A beta_l
// for the L sparse rows beta_l of a CSR matrix B): plain C++, no HIP, so that tests/native/cov_batch_main.cpp can run it as a
// stand-alone program under the address and undefined-behaviour sanitizers.  cov_batch_validate holds the checks the entry point
// makes of its caller's CSR form before anything is uploaded, cov_batch_chunk_rows the number of rows of B that the launcher
// (design.hip, op_cov_mul_batch) keeps on the device at a time, and cov_batch_plan_unions what the dense-storage kernel
// (kernels_cov.hip, cov_mul_batch_kernel) reads for one chunk.  The messages are returned as nullptr or a string (the caller
// raises it as a core_error).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ahip {

constexpr int kCovBatchLb = 8;                             // rows of B per batch: the accumulators of a thread / a lane
constexpr int kCovBatchMaxBatches = 16;                    // batches per chunk at the most
constexpr int64_t kCovBatchOutBytes = int64_t(256) << 20;  // the chunk's (rows, p) output block stays below this, one batch excepted

// The CSR form of an (L, p) matrix, L >= 0 and p > 0: indptr (L + 1) starts at 0 and does not decrease, the column indices of
// a row are inside [0, p) and strictly ascending (scipy: sort_indices + sum_duplicates).  Values are not looked at.
inline const char* cov_batch_validate(int64_t L, const int64_t* indptr, const int64_t* indices, const void* values, int64_t p) {
    if (L < 0) return "mul_batch: L must be >= 0.";
    if (L == 0) return nullptr;
    if (!indptr) return "null argument.";
    if (indptr[0] != 0) return "mul_batch: indptr must start at 0.";
    for (int64_t l = 0; l < L; ++l)
        if (indptr[l + 1] < indptr[l]) return "mul_batch: indptr must be non-decreasing.";
    if (indptr[L] > 0 && (!indices || !values)) return "null argument.";
    for (int64_t l = 0; l < L; ++l)
        for (int64_t k = indptr[l]; k < indptr[l + 1]; ++k) {
            if (indices[k] < 0 || indices[k] >= p) return "mul_batch: column index out of range.";
            if (k > indptr[l] && indices[k] <= indices[k - 1]) return "mul_batch: column indices must be ascending and distinct inside a row.";
        }
    return nullptr;
}

// Rows of B per chunk: whole batches, as many as keep the (rows, p) output block within kCovBatchOutBytes, between one batch and
// kCovBatchMaxBatches.  The device scratch of a call is that of one chunk whatever L is.
inline int64_t cov_batch_chunk_rows(int64_t p, size_t elem) {
    const int64_t row_bytes = std::max<int64_t>(p, 1) * int64_t(elem);
    const int64_t batches = kCovBatchOutBytes / row_bytes / kCovBatchLb;
    return kCovBatchLb * std::min<int64_t>(std::max<int64_t>(batches, 1), kCovBatchMaxBatches);
}

// What the dense-storage kernel reads for the rows [l0, l0 + lc) of a validated B, batch b = rows [l0 + b Lb, l0 + (b + 1) Lb):
// ucols[uptr[b] .. uptr[b + 1]) is the ascending union of the batch's column indices and coef[k * Lb + r] the value row
// l0 + b Lb + r has at ucols[k], zero where the row lacks the index or lies beyond the chunk.
template <class T>
struct CovBatchPlan {
    std::vector<int64_t> uptr;
    std::vector<int32_t> ucols;
    std::vector<T> coef;
    int64_t batches() const { return int64_t(uptr.size()) - 1; }
};

template <class T>
void cov_batch_plan_unions(int64_t l0, int64_t lc, const int64_t* indptr, const int64_t* indices, const T* values, CovBatchPlan<T>& plan) {
    constexpr int Lb = kCovBatchLb;
    plan.uptr.assign(1, 0);
    plan.ucols.clear();
    plan.coef.clear();
    for (int64_t b0 = 0; b0 < lc; b0 += Lb) {
        const int rows = int(std::min<int64_t>(Lb, lc - b0));
        int64_t cur[Lb], end[Lb];
        for (int r = 0; r < rows; ++r) cur[r] = indptr[l0 + b0 + r], end[r] = indptr[l0 + b0 + r + 1];
        for (;;) { // a merge of the rows' ascending runs: the smallest index that some row still has
            int64_t next = -1;
            for (int r = 0; r < rows; ++r)
                if (cur[r] < end[r] && (next < 0 || indices[cur[r]] < next)) next = indices[cur[r]];
            if (next < 0) break;
            plan.ucols.push_back(int32_t(next));
            const size_t at = plan.coef.size();
            plan.coef.resize(at + Lb, T(0));
            for (int r = 0; r < rows; ++r)
                if (cur[r] < end[r] && indices[cur[r]] == next) plan.coef[at + size_t(r)] = values[cur[r]++];
        }
        plan.uptr.push_back(int64_t(plan.ucols.size()));
    }
}

} // namespace ahip
