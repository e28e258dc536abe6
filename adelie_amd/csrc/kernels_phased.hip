// kernels_phased.hip — the kept-sparse design of matrix.snp_phased_ancestry built on the device (gfx950 / CDNA4, wave64).
//
// Input: the CODE TABLE of phased_decode_host.hpp, a column-major uint8 (n, 2 s) array; column 2 j + k is haplotype k of SNP j,
// an entry is the ancestry of a mutation or kPhasedNone.  The design (reference matrix_naive_snp_phased_ancestry.ipp,
// io_snp_phased_ancestry.ipp:44-71) has s A columns, X[i, j A + a] = the number of the two haplotypes of (i, j) that are
// mutated with ancestry a: at most two stored entries per (sample, SNP), one of value 2 when both haplotypes carry the same
// ancestry, two of value 1 in column order when they differ.  Output: the six arrays of a CscView in canonical form (rows
// ascending inside a column, columns ascending inside a row, no explicit zeros), so that every kernel of kernels_sparse.hip
// runs on the result.  No n x s A array is formed and nothing is sorted.
//
//   phased_col_count   one workgroup per (SNP, tile of kPhasedTileRows rows): an A-bin histogram of the tile's entries in LDS
//                      (integer adds: the counts do not depend on their order) -> col_cnt[(j A + a) nt + t]
//   phased_row_count   one thread per row over all SNPs (the table is column-major: coalesced) -> row_cnt[i]
//   (the caller turns the counts into cptr, the start of every (column, tile) segment and rptr by prefix sums)
//   phased_col_fill    one wavefront per (SNP, tile) walks its rows 64 at a time in order; for every ancestry present in the
//                      64 rows the ballot of the lanes that hold it places them: segment start + entries of earlier steps +
//                      the lower lanes of the ballot.  Only ancestries present in the wave are visited.
//   phased_row_fill    one thread per row writes its entries from rptr[i] on, SNPs ascending, the two ancestries of a SNP in
//                      column order.
//
// Every position comes from a count and a prefix sum, none from an atomic's return value: two builds give identical arrays.
// A code that is neither < A nor kPhasedNone cannot come out of the host side; the kernels read it as kPhasedNone all the
// same, count and fill alike, so that the positions stay inside the arrays whatever the table holds.
#include "kernels.hpp"
#include "phased_decode_host.hpp"

#include <algorithm>

namespace ahip {

namespace {

constexpr int kCountThreads = 256;
constexpr int kRowThreads = 256;
constexpr int kNone = int(kPhasedNone);

__device__ __forceinline__ int phased_code(const uint8_t* __restrict__ col, int64_t i, int A) {
    const int c = col[i];
    return c < A ? c : kNone;
}

__global__ __launch_bounds__(kCountThreads) void phased_col_count_kernel(const uint8_t* __restrict__ code, int64_t n, int A, int nt,
                                                                         int32_t* __restrict__ col_cnt) {
    __shared__ int32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t j = int64_t(blockIdx.x) / nt;
    const int t = int(int64_t(blockIdx.x) % nt);
    const uint8_t* h0 = code + 2 * j * n;
    const uint8_t* h1 = h0 + n;
    const int64_t r0 = int64_t(t) * kPhasedTileRows, r1 = min(n, r0 + kPhasedTileRows);
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kCountThreads) {
        const int c0 = phased_code(h0, i, A), c1 = phased_code(h1, i, A);
        if (c0 != kNone) atomicAdd(&hist[c0], 1);
        if (c1 != kNone && c1 != c0) atomicAdd(&hist[c1], 1);
    }
    __syncthreads();
    for (int a = threadIdx.x; a < A; a += kCountThreads) col_cnt[(j * A + a) * nt + t] = hist[a];
}

__global__ __launch_bounds__(kRowThreads) void phased_row_count_kernel(const uint8_t* __restrict__ code, int64_t n, int64_t s, int A,
                                                                       int64_t* __restrict__ row_cnt) {
    const int64_t i = int64_t(blockIdx.x) * kRowThreads + threadIdx.x;
    if (i >= n) return;
    int64_t cnt = 0;
    for (int64_t j = 0; j < s; ++j) {
        const int c0 = phased_code(code + 2 * j * n, i, A), c1 = phased_code(code + (2 * j + 1) * n, i, A);
        cnt += int(c0 != kNone) + int(c1 != kNone && c1 != c0);
    }
    row_cnt[i] = cnt;
}

template <class T>
__global__ __launch_bounds__(64) void phased_col_fill_kernel(const uint8_t* __restrict__ code, int64_t n, int A, int nt,
                                                             const int64_t* __restrict__ col_pos, int32_t* __restrict__ cidx,
                                                             T* __restrict__ cval) {
    __shared__ int32_t run[256]; // entries of ancestry a written by the earlier steps of this tile
    const int lane = threadIdx.x;
    for (int a = lane; a < 256; a += 64) run[a] = 0;
    __syncthreads();
    const int64_t j = int64_t(blockIdx.x) / nt;
    const int t = int(int64_t(blockIdx.x) % nt);
    const uint8_t* h0 = code + 2 * j * n;
    const uint8_t* h1 = h0 + n;
    const int64_t r0 = int64_t(t) * kPhasedTileRows, r1 = min(n, r0 + kPhasedTileRows);
    const int64_t* pos = col_pos + j * A * nt + t; // the segment of ancestry a starts at pos[a * nt]
    const unsigned long long lower = (1ull << lane) - 1;
    for (int64_t b = r0; b < r1; b += 64) { // (b, r1 and every loop condition below are the same in all lanes)
        const int64_t i = b + lane;
        int c0 = kNone, c1 = kNone;
        if (i < r1) {
            c0 = phased_code(h0, i, A);
            c1 = phased_code(h1, i, A);
        }
        // what the lane still has to place: its first haplotype's column, and the second's when that is another column
        int p0 = c0 != kNone ? c0 : -1;
        int p1 = (c1 != kNone && c1 != c0) ? c1 : -1;
        for (;;) {
            const int cand = p0 >= 0 ? p0 : p1;
            const unsigned long long pend = __ballot(cand >= 0);
            if (!pend) break;
            const int a = __shfl(cand, __ffsll(pend) - 1); // an ancestry present in these 64 rows; each is visited once
            const bool hit = p0 == a || p1 == a;
            const unsigned long long m = __ballot(hit);
            const int32_t before = run[a];
            __syncthreads();
            if (hit) {
                const int64_t at = pos[int64_t(a) * nt] + before + __popcll(m & lower);
                cidx[at] = int32_t(i);
                cval[at] = T((c0 == a && c1 == a) ? 2 : 1);
                if (p0 == a) p0 = -1;
                else p1 = -1;
            }
            if (lane == 0) run[a] = before + int32_t(__popcll(m));
            __syncthreads();
        }
    }
}

template <class T>
__global__ __launch_bounds__(kRowThreads) void phased_row_fill_kernel(const uint8_t* __restrict__ code, int64_t n, int64_t s, int A,
                                                                      const int64_t* __restrict__ rptr, int32_t* __restrict__ rcol,
                                                                      T* __restrict__ rval) {
    const int64_t i = int64_t(blockIdx.x) * kRowThreads + threadIdx.x;
    if (i >= n) return;
    int64_t k = rptr[i];
    for (int64_t j = 0; j < s; ++j) {
        const int c0 = phased_code(code + 2 * j * n, i, A), c1 = phased_code(code + (2 * j + 1) * n, i, A);
        const int lo = min(c0, c1), hi = max(c0, c1); // kNone is the largest code: lo is a column unless both are kNone
        if (lo == kNone) continue;
        const int32_t base = int32_t(j * A);
        rcol[k] = base + lo;
        rval[k] = T(lo == hi ? 2 : 1);
        ++k;
        if (hi != kNone && hi != lo) {
            rcol[k] = base + hi;
            rval[k] = T(1);
            ++k;
        }
    }
}

} // namespace

int phased_tiles(int64_t n) { return int((n + kPhasedTileRows - 1) / kPhasedTileRows); }

void launch_phased_count(const uint8_t* code, int64_t n, int64_t s, int A, int32_t* col_cnt, int64_t* row_cnt, hipStream_t st) {
    const int nt = phased_tiles(n);
    hipLaunchKernelGGL(phased_col_count_kernel, dim3(unsigned(s * nt)), dim3(kCountThreads), 0, st, code, n, A, nt, col_cnt);
    hipLaunchKernelGGL(phased_row_count_kernel, dim3(unsigned((n + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, st, code, n, s,
                       A, row_cnt);
}

template <class T>
void launch_phased_fill(const uint8_t* code, int64_t n, int64_t s, int A, const int64_t* col_pos, const int64_t* rptr, int32_t* cidx,
                        T* cval, int32_t* rcol, T* rval, hipStream_t st) {
    const int nt = phased_tiles(n);
    hipLaunchKernelGGL((phased_col_fill_kernel<T>), dim3(unsigned(s * nt)), dim3(64), 0, st, code, n, A, nt, col_pos, cidx, cval);
    hipLaunchKernelGGL((phased_row_fill_kernel<T>), dim3(unsigned((n + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, st, code, n,
                       s, A, rptr, rcol, rval);
}
template void launch_phased_fill<double>(const uint8_t*, int64_t, int64_t, int, const int64_t*, const int64_t*, int32_t*, double*,
                                         int32_t*, double*, hipStream_t);
template void launch_phased_fill<float>(const uint8_t*, int64_t, int64_t, int, const int64_t*, const int64_t*, int32_t*, float*, int32_t*,
                                        float*, hipStream_t);

} // namespace ahip
