// kernels_cov_sparse.hip — the covariance method's matrix A kept sparse in HBM (adelie_hip_design_create_cov_csc; reference
// MatrixCovSparse, matrix_cov_sparse.ipp, and MatrixCovBlockDiag): the column-compressed form of a symmetric (p, p) matrix and
// nothing else, 12 bytes per stored entry in f64.  The path solver touches A in two places (kernels_cov.hip has the dense
// forms): the gather of A[S, S] into the screen Gram matrix and grad = v - A beta once per lambda.  Both walk stored entries
// only; neither uses an atomic and every sum runs in a fixed order, so two runs give the same bits.
//
// Column dot (grad, mul, bmul): out[j] = base[j] - sum_e cval[e] * w[cidx[e]] over the entries of column j, w a dense (p,)
// vector that holds the coefficients at their rows and zero elsewhere.  A symmetric, so column j is row j.  One group of L
// lanes per column (L in {4, 16, 64}, cov_csc_host.hpp picks it from the mean column count), entries strided over the lanes,
// a shuffle tree inside the group, lane 0 writes; a column longer than L entries loops.  12 nnz + O(p) bytes whatever the
// active set is.
// Gather: a (p,) map from a row of A to its position among the screen values, then one lane group per new column copies the
// stored entries whose row is a screen value; the cells of the two strips that A does not store are zeroed first.  Every cell
// has one writer and is a copy, so C has the bits the dense gather gives.
#include "common.hpp"
#include "cov_csc_host.hpp"
#include "cov_batch_host.hpp"

namespace ahip {

namespace {

constexpr int kCovCscBatchPasses = 4; // passes of a lane group in flight in the batched column dot (its header comment)

// w[cols[k]] = coef[k] for k < *cnt (the count lives on the device, as cov_grad_kernel reads it); w was zeroed before
template <class T>
__global__ __launch_bounds__(256) void cov_csc_fill_w_kernel(const int32_t* __restrict__ cols, const T* __restrict__ coef,
                                                             const int32_t* __restrict__ cnt, T* __restrict__ w) {
    const int32_t m = *cnt;
    for (int32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x) w[cols[k]] = coef[k];
}

template <class T, int L>
__global__ __launch_bounds__(kCovCscBlock) void cov_csc_coldot_kernel(const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                                      const T* __restrict__ cval, const int64_t* __restrict__ subset,
                                                                      int64_t ncols, const T* __restrict__ w, const T* __restrict__ base,
                                                                      T* __restrict__ out) {
    const int l = threadIdx.x % L;
    const int64_t jj = int64_t(blockIdx.x) * (kCovCscBlock / L) + threadIdx.x / L;
    if (jj >= ncols) return; // (a whole group leaves together: the shuffles below stay inside a group)
    const int64_t j = subset ? subset[jj] : jj;
    const int64_t e1 = cptr[j + 1];
    T acc = 0;
    // eight passes' loads in flight at once (a column of 512 entries is one trip of a 64-lane group); a pass beyond the column's
    // end loads nothing and adds nothing, and the additions keep the order of the plain loop
    constexpr int U = 8;
    for (int64_t e = cptr[j] + l; e < e1; e += U * L) {
        int32_t r[U];
        T a[U], x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = e + u * L < e1 ? cidx[e + u * L] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = e + u * L < e1 ? cval[e + u * L] : T(0);
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = w[r[u]];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (e + u * L < e1) acc += a[u] * x[u];
    }
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, L);
    if (l == 0) out[jj] = base ? base[j] - acc : acc;
}

// Lambda-batched column dot (adelie_hip_design_cov_mul_batch): LB rows of a CSR matrix B at a time.
// Fill: w is a dense (p, LB) block, the row of B fastest, zeroed before; row b of the batch writes its values at its columns
// (blockIdx.y = b; indptr holds the chunk's row pointers, `ebase` the position of the chunk's first entry).  The value goes
// through 0 + x as on the single-vector route (cov_csc_upload_w sums into a zeroed vector), so a stored -0 reads the same.
template <class T, int LB>
__global__ __launch_bounds__(256) void cov_csc_fill_w_batch_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                                                                   const T* __restrict__ values, int64_t ebase, T* __restrict__ w) {
    const int b = blockIdx.y;
    const int64_t e1 = indptr[b + 1] - ebase;
    for (int64_t e = indptr[b] - ebase + blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += int64_t(gridDim.x) * blockDim.x)
        w[indices[e] * LB + b] = T(0) + values[e];
}

// out[b, j] = base[j] - sum_e cval[e] * w[cidx[e], b] for b < rows: cov_csc_coldot_kernel with LB accumulators per lane.  The
// lane group, the entries a lane owns, their order and the shuffle tree are the single-vector kernel's, so row b has the bits
// of a single column dot over w[:, b]; an index and a value are loaded once for the LB rows, and the LB values of w behind an
// index are one contiguous run (64 bytes in f64).
// LB = 8 with U = 4 passes unrolled, from the compile output for gfx950 (-Rpass-analysis=kernel-resource-usage; the figures
// do not depend on the lane count; no scratch memory anywhere), f64 VGPRs / waves per SIMD:
//     LB 4, U 8: 60 / 8     LB 8, U 2: 52 / 8     LB 8, U 4: 60 / 8     LB 8, U 8: 76 / 6     LB 16, U 2: 84 / 5     LB 16, U 4: 92 / 5
// (f32 at LB 8, U 4: 44 / 8).  LB = 8 is the widest batch that keeps the full 8 waves per SIMD, and U = 4 the deepest unroll
// that does at that width; every doubling of LB halves the reads of the stored entries per row of B.
template <class T, int L, int LB, int U>
__global__ __launch_bounds__(kCovCscBlock) void cov_csc_coldot_batch_kernel(const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                                            const T* __restrict__ cval, int64_t ncols,
                                                                            const T* __restrict__ w, const T* __restrict__ base, int rows,
                                                                            T* __restrict__ out) {
    const int l = threadIdx.x % L;
    const int64_t j = int64_t(blockIdx.x) * (kCovCscBlock / L) + threadIdx.x / L;
    if (j >= ncols) return; // (a whole group leaves together: the shuffles below stay inside a group)
    const int64_t e1 = cptr[j + 1];
    T acc[LB];
#pragma unroll
    for (int b = 0; b < LB; ++b) acc[b] = T(0);
    for (int64_t e = cptr[j] + l; e < e1; e += U * L) {
        int32_t r[U];
        T a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = e + u * L < e1 ? cidx[e + u * L] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = e + u * L < e1 ? cval[e + u * L] : T(0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            T x[LB]; // (a pass beyond the column's end reads row 0 of w and adds nothing)
#pragma unroll
            for (int b = 0; b < LB; ++b) x[b] = w[int64_t(r[u]) * LB + b];
            if (e + u * L < e1) {
#pragma unroll
                for (int b = 0; b < LB; ++b) acc[b] = fma(a[u], x[b], acc[b]); // (spelled out: the single kernel's sum is contracted to this)
            }
        }
    }
#pragma unroll
    for (int b = 0; b < LB; ++b) {
#pragma unroll
        for (int off = L / 2; off > 0; off >>= 1) acc[b] += __shfl_down(acc[b], off, L);
    }
    if (l == 0) {
#pragma unroll
        for (int b = 0; b < LB; ++b)
            if (b < rows) out[int64_t(b) * ncols + j] = base ? base[j] - acc[b] : acc[b];
    }
}

__global__ __launch_bounds__(256) void cov_csc_pos_kernel(const int32_t* __restrict__ vcol, int32_t nv, int32_t* __restrict__ pos) {
    const int32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < nv) pos[vcol[a]] = a;
}

// zeroes C[0:nv, pos0:nv] and C[pos0:nv, 0:pos0]
template <class T>
__global__ __launch_bounds__(256) void cov_csc_zero_strips_kernel(int32_t nv, int32_t pos0, int32_t N, T* __restrict__ C, int64_t ldc) {
    const int64_t tall = int64_t(nv) * N, total = tall + int64_t(N) * pos0;
    for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < total; k += int64_t(gridDim.x) * blockDim.x) {
        if (k < tall) C[k % nv + (pos0 + k / nv) * ldc] = T(0);
        else C[pos0 + (k - tall) % N + ((k - tall) / N) * ldc] = T(0);
    }
}

// C[a, pos0 + b] = A(vcol[a], vcol[pos0 + b]) for the stored rows of column vcol[pos0 + b] that are screen values, mirrored into
// C[pos0 + b, a] for the old values a < pos0 (cov_gather_kernel's cells; the new x new square is covered from both sides)
template <class T, int L>
__global__ __launch_bounds__(kCovCscBlock) void cov_csc_gather_kernel(const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                                      const T* __restrict__ cval, const int32_t* __restrict__ vcol,
                                                                      const int32_t* __restrict__ pos, int32_t pos0, int32_t N,
                                                                      T* __restrict__ C, int64_t ldc) {
    const int l = threadIdx.x % L;
    const int64_t b = int64_t(blockIdx.x) * (kCovCscBlock / L) + threadIdx.x / L;
    if (b >= N) return;
    const int64_t cb = pos0 + b, j = vcol[cb];
    const int64_t e1 = cptr[j + 1];
    for (int64_t e = cptr[j] + l; e < e1; e += L) {
        const int32_t a = pos[cidx[e]];
        if (a < 0) continue;
        const T val = cval[e];
        C[a + cb * ldc] = val;
        if (a < pos0) C[cb + int64_t(a) * ldc] = val;
    }
}

// out (q, q) column-major, zeroed before: the stored entries of columns i .. i + q whose row lies in [i, i + q)
template <class T, int L>
__global__ __launch_bounds__(kCovCscBlock) void cov_csc_to_dense_kernel(const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                                        const T* __restrict__ cval, int64_t i, int64_t q, T* __restrict__ out) {
    const int l = threadIdx.x % L;
    const int64_t b = int64_t(blockIdx.x) * (kCovCscBlock / L) + threadIdx.x / L;
    if (b >= q) return;
    const int64_t e1 = cptr[i + b + 1];
    for (int64_t e = cptr[i + b] + l; e < e1; e += L) {
        const int64_t r = int64_t(cidx[e]) - i;
        if (r >= 0 && r < q) out[r + b * q] = cval[e];
    }
}

// runs f(std::integral_constant<int, L>) for the handle's lane count
template <class F>
void with_lanes(int lanes, F&& f) {
    if (lanes == 4) f(std::integral_constant<int, 4>{});
    else if (lanes == 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 64>{});
}

} // namespace

template <class T>
void launch_cov_csc_fill_w(const int32_t* cols, const T* coef, const int32_t* cnt, int64_t max_cnt, T* w, int64_t p, hipStream_t s) {
    AHIP_CHECK(hipMemsetAsync(w, 0, size_t(p) * sizeof(T), s));
    if (max_cnt <= 0) return;
    const int64_t blocks = std::min<int64_t>((max_cnt + 255) / 256, 4096);
    hipLaunchKernelGGL((cov_csc_fill_w_kernel<T>), dim3(unsigned(blocks)), dim3(256), 0, s, cols, coef, cnt, w);
}

template <class T>
void launch_cov_csc_coldot(const CovCscView<T>& A, const int64_t* subset, int64_t ncols, const T* w, const T* base, T* out,
                           hipStream_t s) {
    if (ncols <= 0) return;
    const CovCscShape sh = cov_csc_shape(ncols, A.lanes);
    with_lanes(sh.lanes, [&](auto L) {
        hipLaunchKernelGGL((cov_csc_coldot_kernel<T, decltype(L)::value>), dim3(unsigned(sh.blocks)), dim3(kCovCscBlock), 0, s, A.cptr,
                           A.cidx, A.cval, subset, ncols, w, base, out);
    });
}

template <class T>
void launch_cov_csc_fill_w_batch(const int64_t* indptr, const int64_t* indices, const T* values, int64_t ebase, int rows,
                                 int64_t max_row, T* w, int64_t p, hipStream_t s) {
    AHIP_CHECK(hipMemsetAsync(w, 0, size_t(p) * kCovBatchLb * sizeof(T), s));
    if (rows <= 0 || max_row <= 0) return;
    const int64_t blocks = std::min<int64_t>((max_row + 255) / 256, 4096);
    hipLaunchKernelGGL((cov_csc_fill_w_batch_kernel<T, kCovBatchLb>), dim3(unsigned(blocks), unsigned(rows)), dim3(256), 0, s, indptr,
                       indices, values, ebase, w);
}

// One batch of `rows` <= kCovBatchLb rows: w (p, kCovBatchLb) from launch_cov_csc_fill_w_batch, out (rows, p) with rows
// contiguous.  The lane count is the one launch_cov_csc_coldot takes for a full-width product.
template <class T>
void launch_cov_csc_coldot_batch(const CovCscView<T>& A, const T* w, const T* base, int rows, T* out, hipStream_t s) {
    if (rows <= 0 || A.p <= 0) return;
    const CovCscShape sh = cov_csc_shape(A.p, A.lanes);
    with_lanes(sh.lanes, [&](auto L) {
        hipLaunchKernelGGL((cov_csc_coldot_batch_kernel<T, decltype(L)::value, kCovBatchLb, kCovCscBatchPasses>), dim3(unsigned(sh.blocks)),
                           dim3(kCovCscBlock), 0, s, A.cptr, A.cidx, A.cval, A.p, w, base, rows, out);
    });
}

template <class T>
void launch_cov_csc_gather(const CovCscView<T>& A, const int32_t* vcol, int32_t nv, int32_t pos0, int32_t N, T* C, int64_t ldc,
                           int32_t* pos, hipStream_t s) {
    if (nv <= 0 || N <= 0) return;
    AHIP_CHECK(hipMemsetAsync(pos, 0xFF, size_t(A.p) * sizeof(int32_t), s)); // -1: not a screen value
    hipLaunchKernelGGL(cov_csc_pos_kernel, dim3(unsigned((nv + 255) / 256)), dim3(256), 0, s, vcol, nv, pos);
    const int64_t cells = int64_t(nv) * N + int64_t(N) * pos0;
    hipLaunchKernelGGL((cov_csc_zero_strips_kernel<T>), dim3(unsigned(std::min<int64_t>((cells + 255) / 256, int64_t(1) << 20))), dim3(256),
                       0, s, nv, pos0, N, C, ldc);
    const CovCscShape sh = cov_csc_shape(N, A.lanes);
    with_lanes(sh.lanes, [&](auto L) {
        hipLaunchKernelGGL((cov_csc_gather_kernel<T, decltype(L)::value>), dim3(unsigned(sh.blocks)), dim3(kCovCscBlock), 0, s, A.cptr,
                           A.cidx, A.cval, vcol, pos, pos0, N, C, ldc);
    });
}

template <class T>
void launch_cov_csc_to_dense(const CovCscView<T>& A, int64_t i, int64_t q, T* out, hipStream_t s) {
    if (q <= 0) return;
    AHIP_CHECK(hipMemsetAsync(out, 0, size_t(q) * size_t(q) * sizeof(T), s));
    const CovCscShape sh = cov_csc_shape(q, A.lanes);
    with_lanes(sh.lanes, [&](auto L) {
        hipLaunchKernelGGL((cov_csc_to_dense_kernel<T, decltype(L)::value>), dim3(unsigned(sh.blocks)), dim3(kCovCscBlock), 0, s, A.cptr,
                           A.cidx, A.cval, i, q, out);
    });
}

#define INST(T)                                                                                                                  \
    template void launch_cov_csc_fill_w<T>(const int32_t*, const T*, const int32_t*, int64_t, T*, int64_t, hipStream_t);         \
    template void launch_cov_csc_coldot<T>(const CovCscView<T>&, const int64_t*, int64_t, const T*, const T*, T*, hipStream_t);  \
    template void launch_cov_csc_gather<T>(const CovCscView<T>&, const int32_t*, int32_t, int32_t, int32_t, T*, int64_t, int32_t*, \
                                           hipStream_t);                                                                         \
    template void launch_cov_csc_to_dense<T>(const CovCscView<T>&, int64_t, int64_t, T*, hipStream_t);                           \
    template void launch_cov_csc_fill_w_batch<T>(const int64_t*, const int64_t*, const T*, int64_t, int, int64_t, T*, int64_t,   \
                                                 hipStream_t);                                                                   \
    template void launch_cov_csc_coldot_batch<T>(const CovCscView<T>&, const T*, const T*, int, T*, hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
