// kernels_pinball_sparse.hip — the two products pinball's extend() needs when the constraint matrix A (m, d) is kept sparse
// (adelie_hip_design_create_constraint_csc; reference matrix_constraint_sparse.ipp).  The handle is the kCsc design of A': a row
// of A is one compressed column (cptr / cidx / cval, stored indices ascending), as a row of the dense constraint handle is one
// contiguous column.  Both kernels replace launch_ptq (kernels_pinball.hip) where it reads the dense A':
//
//   rows x dense          AS[r + c ld]  = sum_e val_e S[idx_e, r]            e over the stored entries of row cols[c] of A
//   rows . dense columns  C[r + c ldc]  = sum_e val_e Q[idx_e + c ldq]       e over the stored entries of row pcols[r] of A
//
// Every output element is one thread's sum over e in ascending stored index, in one accumulator that starts at 0, each term
// written as ptq_kernel writes it (acc += a * b under the same contraction setting).  ptq_kernel runs over all d indices in
// ascending order; the terms these kernels skip multiply a structural zero and are exact no-ops for finite inputs, so AS and H
// of the sparse route are, as numbers, those of the dense route on A.toarray().  That holds in float64, where both files compile
// every term to one fused multiply-add (tests/test_gpu_pinball_sparse.py compares the two routes with array_equal).  In float32
// the compiler packs part of ptq_kernel's unrolled tile loop into separate multiplies and adds, which no loop over stored entries
// can mirror term by term: there the two routes agree to rounding.  No atomics: two runs give the same bits.
//
// Lanes and memory:
//   * rows x dense.  One wavefront per output column c, its lanes over r.  The row's (idx, val) pairs are the same address for
//     the whole wavefront (broadcast loads, read once per 64 outputs); the gather is by idx_e into S.  S[idx_e, r] over lanes r
//     would stride by d in the column-major S, so the kernel reads the transposed copy ST[r + idx_e d] (one copy of d^2 values
//     per solve, the size of the upload itself): each gathered row of ST is contiguous across the lanes, and so is the store.
//   * rows . dense columns.  One thread per row r and kColsPerThread = 8 consecutive columns c, lanes over r: the thread loads
//     each of its (idx, val) pairs once per 8 outputs and keeps the 8 sums in registers, the four wavefronts of a workgroup take
//     the same 64 rows (their entries stay in the CU's cache) and neighbouring column groups, and the stores are contiguous
//     across the lanes.  The gather is Q[idx_e + c ldq]: rows are short and differ from lane to lane, so the 64 lanes of a load
//     hit 64 places of ONE column of Q (d values, 4 KB at d = 512), which sits in L2 (Q is the compact AS, ns d values).  Lanes
//     over c instead would make the entries a broadcast but turn both the gather and the store into strides of ldq / ldc.
//     Rows of unequal length leave lanes idle until the longest of the 64 is done; one accumulator per element in ascending
//     order rules out splitting a row over lanes.
#include "kernels.hpp"

#include <algorithm>

namespace ahip {

namespace {

constexpr int kColsPerThread = 8;
constexpr int kTrTile = 32;

inline unsigned sp_blocks_for(int64_t n, int64_t per, int64_t cap) {
    return unsigned(std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap)));
}

// out[c + r d] = in[r + c d]  (d x d, LDS tiles: both sides contiguous across the lanes)
template <class T>
__global__ __launch_bounds__(kTrTile * 8) void transpose_square_kernel(const T* __restrict__ in, int64_t d, T* __restrict__ out) {
    __shared__ T tile[kTrTile][kTrTile + 1];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t r0 = int64_t(blockIdx.x) * kTrTile, c0 = int64_t(blockIdx.y) * kTrTile;
    for (int k = ty; k < kTrTile; k += 8) {
        const int64_t r = r0 + tx, c = c0 + k;
        tile[k][tx] = (r < d && c < d) ? in[r + c * d] : T(0);
    }
    __syncthreads();
    for (int k = ty; k < kTrTile; k += 8) {
        const int64_t c = c0 + tx, r = r0 + k;
        if (r < d && c < d) out[c + r * d] = tile[tx][k];
    }
}

// AS[r + c ld] = sum_e cval[e] ST[r + cidx[e] d] over the entries of compressed column col(c) = cols ? cols[c] : c
template <class T>
__global__ __launch_bounds__(256) void csc_rows_dense_kernel(const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                              const T* __restrict__ cval, const int32_t* __restrict__ cols,
                                                              int64_t N, const T* __restrict__ ST, int64_t d, T* __restrict__ AS,
                                                              int64_t ld) {
    const int64_t c = int64_t(blockIdx.x) * 4 + threadIdx.y;
    if (c >= N) return;
    const int64_t col = cols ? int64_t(cols[c]) : c;
    const int64_t b = cptr[col], e = cptr[col + 1];
    for (int64_t r = int64_t(blockIdx.y) * 64 + threadIdx.x; r < d; r += int64_t(gridDim.y) * 64) {
        T acc = T(0);
        for (int64_t t = b; t < e; ++t) acc += cval[t] * ST[r + int64_t(cidx[t]) * d];
        AS[r + c * ld] = acc;
    }
}

// C[r + c ldc] = sum_e cval[e] Q[cidx[e] + c ldq] over the entries of compressed column pcol(r) = pcols ? pcols[r] : r
template <class T>
__global__ __launch_bounds__(256) void csc_rows_cols_kernel(const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                             const T* __restrict__ cval, const int32_t* __restrict__ pcols,
                                                             int64_t M, const T* __restrict__ Q, int64_t ldq, int64_t N,
                                                             T* __restrict__ C, int64_t ldc) {
    const int64_t r = int64_t(blockIdx.x) * 64 + threadIdx.x;
    if (r >= M) return;
    const int64_t col = pcols ? int64_t(pcols[r]) : r;
    const int64_t b = cptr[col], e = cptr[col + 1];
    const int64_t step = int64_t(gridDim.y) * 4 * kColsPerThread;
    for (int64_t c0 = (int64_t(blockIdx.y) * 4 + threadIdx.y) * kColsPerThread; c0 < N; c0 += step) {
        const T* __restrict__ q = Q + c0 * ldq;
        T acc[kColsPerThread];
#pragma unroll
        for (int k = 0; k < kColsPerThread; ++k) acc[k] = T(0);
        if (c0 + kColsPerThread <= N) {
            for (int64_t t = b; t < e; ++t) {
                const T a = cval[t];
                const T* __restrict__ qi = q + cidx[t];
#pragma unroll
                for (int k = 0; k < kColsPerThread; ++k) acc[k] += a * qi[int64_t(k) * ldq];
            }
        } else {
            const int nk = int(N - c0);
            for (int64_t t = b; t < e; ++t) {
                const T a = cval[t];
                const T* __restrict__ qi = q + cidx[t];
#pragma unroll
                for (int k = 0; k < kColsPerThread; ++k)
                    if (k < nk) acc[k] += a * qi[int64_t(k) * ldq];
            }
        }
#pragma unroll
        for (int k = 0; k < kColsPerThread; ++k)
            if (c0 + k < N) C[r + (c0 + k) * ldc] = acc[k];
    }
}

} // namespace

template <class T>
void launch_transpose_square(const T* in, int64_t d, T* out, hipStream_t s) {
    if (d <= 0) return;
    const unsigned g = unsigned((d + kTrTile - 1) / kTrTile);
    hipLaunchKernelGGL((transpose_square_kernel<T>), dim3(g, g), dim3(kTrTile, 8), 0, s, in, d, out);
}

template <class T>
void launch_csc_rows_dense(const CscView<T>& A, const int32_t* cols, int64_t N, const T* ST, T* AS, int64_t ld, hipStream_t s) {
    if (N <= 0 || A.n <= 0) return;
    hipLaunchKernelGGL((csc_rows_dense_kernel<T>), dim3(unsigned((N + 3) / 4), sp_blocks_for(A.n, 64, 65535)), dim3(64, 4), 0, s,
                       A.cptr, A.cidx, A.cval, cols, N, ST, A.n, AS, ld);
}

template <class T>
void launch_csc_rows_cols(const CscView<T>& A, const int32_t* pcols, int64_t M, const T* Q, int64_t ldq, int64_t N, T* C,
                          int64_t ldc, hipStream_t s) {
    if (M <= 0 || N <= 0) return;
    hipLaunchKernelGGL((csc_rows_cols_kernel<T>), dim3(unsigned((M + 63) / 64), sp_blocks_for(N, 4 * kColsPerThread, 65535)),
                       dim3(64, 4), 0, s, A.cptr, A.cidx, A.cval, pcols, M, Q, ldq, N, C, ldc);
}

#define AHIP_INSTANTIATE(T)                                                                                                   \
    template void launch_transpose_square<T>(const T*, int64_t, T*, hipStream_t);                                            \
    template void launch_csc_rows_dense<T>(const CscView<T>&, const int32_t*, int64_t, const T*, T*, int64_t, hipStream_t);  \
    template void launch_csc_rows_cols<T>(const CscView<T>&, const int32_t*, int64_t, const T*, int64_t, int64_t, T*, int64_t, \
                                          hipStream_t);
AHIP_INSTANTIATE(float)
AHIP_INSTANTIATE(double)
#undef AHIP_INSTANTIATE

} // namespace ahip
