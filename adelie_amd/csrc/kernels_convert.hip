// kernels_convert.hip — building a resident design from what the caller holds, and one design from another (gfx950 / CDNA4):
// transpose, pack_snp, bed_transcode, snp_impute, derive_dense (standardize / subset of a dense or 2-bit design), snp_subset,
// gather_cols, csc_scatter, copy2d.  None of them is on a solve's hot path; the streaming sweeps are kernels_sweep.hip.
// Also the solver's small elementwise helpers that belong to no engine: abs_grad / abs_grad_cons (update_abs_grad) and the
// clamped diagonals of Gram blocks (diag_vars, block_diag_vars).
#include "sweep_common.hpp"
#include <algorithm>

namespace ahip {

namespace {

template <class T>
__global__ void abs_grad_kernel(const T* __restrict__ grad, const int64_t* __restrict__ groups,
                                const int64_t* __restrict__ group_sizes, int64_t G, const int32_t* __restrict__ slot,
                                const T* __restrict__ screen_beta, const T* __restrict__ penalty, T oma_lmda,
                                T* __restrict__ abs_grad) {
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int64_t k = groups[g], sz = group_sizes[g];
    const int32_t sl = slot[g];
    T acc = T(0);
    if (sl >= 0) {
        const T regul = oma_lmda * penalty[g];
        for (int64_t t = 0; t < sz; ++t) {
            const T e = grad[k + t] - regul * screen_beta[sl + t];
            acc += e * e;
        }
    } else {
        for (int64_t t = 0; t < sz; ++t) acc += grad[k + t] * grad[k + t];
    }
    abs_grad[g] = sqrt(acc);
}

// update_abs_grad (solver_base.hpp:20-110) when some groups of one coefficient carry a box constraint
// lo <= beta <= hi (lo <= 0 <= hi, +-inf: none): a screened coordinate subtracts its multiplier (the constraint's gradient,
// :69-75), any other constrained one takes the multiplier that best explains its gradient at beta = 0 (solve_zero,
// constraint_box.ipp:268-284: free in the directions whose bound is exactly zero, zero elsewhere).  mu_out: every group's
// multiplier (what sparsify_dual reads off the constraint objects, :158-222).
template <class T>
__global__ void abs_grad_cons_kernel(const T* __restrict__ grad, const int64_t* __restrict__ groups,
                                     const int64_t* __restrict__ group_sizes, int64_t G,
                                     const int32_t* __restrict__ slot, const T* __restrict__ screen_beta,
                                     const T* __restrict__ penalty, T oma_lmda, const T* __restrict__ clo,
                                     const T* __restrict__ chi, const T* __restrict__ cmu, T* __restrict__ abs_grad,
                                     T* __restrict__ mu_out) {
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const T INF = T(1) / T(0), M = T(1e100); // Configs::max_solver_value (inf in single precision, as in the reference)
    const int64_t sz = group_sizes[g];
    if (sz != 1) { // groups of several coefficients carry no constraint: abs_grad_kernel's norm
        const int64_t k = groups[g];
        const int32_t sl0 = slot[g];
        T acc = T(0);
        for (int64_t t = 0; t < sz; ++t) {
            const T e0 = sl0 >= 0 ? grad[k + t] - oma_lmda * penalty[g] * screen_beta[sl0 + t] : grad[k + t];
            acc += e0 * e0;
        }
        abs_grad[g] = sqrt(acc);
        mu_out[g] = T(0);
        return;
    }
    const T v = grad[groups[g]], lo = clo[g], hi = chi[g];
    const bool constrained = lo != -INF || hi != INF;
    const int32_t sl = slot[g];
    T mu = T(0), e;
    if (sl >= 0) {
        if (constrained) mu = cmu[sl];
        e = v - oma_lmda * penalty[g] * screen_beta[sl] - mu;
    } else {
        if (constrained) mu = fmin(fmax(v, lo >= T(0) ? -M : T(0)), hi <= T(0) ? M : T(0));
        e = v - mu;
    }
    abs_grad[g] = fabs(e);
    mu_out[g] = mu;
}

template <class T>
__global__ void copy2d_kernel(const T* __restrict__ src, int64_t lds_, T* __restrict__ dst, int64_t ldd, int64_t rows,
                              int64_t cols) {
    const int64_t j = blockIdx.y;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < rows; i += int64_t(gridDim.x) * blockDim.x)
        dst[i + j * ldd] = src[i + j * lds_];
    (void)cols;
}

template <class T>
__global__ void diag_vars_kernel(const T* __restrict__ C, int64_t ldc, int32_t pos0, int32_t cnt, T* __restrict__ vars) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= cnt) return;
    const T d = C[int64_t(pos0 + a) * (ldc + 1)];
    vars[pos0 + a] = d > T(0) ? d : T(0);
}

// row-major (n,p) -> column-major with leading dimension ld, through a 32x33 LDS tile
template <class T>
__global__ void transpose_kernel(const T* __restrict__ src, int64_t n, int64_t p, T* __restrict__ dst, int64_t ld) {
    __shared__ T tile[32][33];
    const int64_t i0 = int64_t(blockIdx.y) * 32, j0 = int64_t(blockIdx.x) * 32;
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int64_t i = i0 + r, j = j0 + threadIdx.x;
        if (i < n && j < p) tile[r][threadIdx.x] = src[i * p + j];
    }
    __syncthreads();
    for (int c = threadIdx.y; c < 32; c += blockDim.y) {
        const int64_t j = j0 + c, i = i0 + threadIdx.x;
        if (i < n && j < p) dst[i + j * ld] = tile[threadIdx.x][c];
    }
}

__global__ void pack_snp_kernel(const int8_t* __restrict__ calldata, int64_t n, int64_t p, uint8_t* __restrict__ bits,
                                int64_t ldb) {
    const int64_t j = blockIdx.y;
    const int64_t nb = (n + 3) / 4;
    for (int64_t b = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; b < ldb; b += int64_t(gridDim.x) * blockDim.x) {
        unsigned byte = 0;
        if (b < nb) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = b * 4 + k;
                unsigned code = 0;
                if (i < n) {
                    const int8_t c = calldata[i + j * n];
                    code = c < 0 ? 3u : unsigned(c);
                }
                byte |= code << (2 * k);
            }
        }
        bits[j * ldb + b] = uint8_t(byte);
    }
    (void)p;
}

// PLINK 1 .bed record (SNP-major) -> device 2-bit codes.  .bed: 2 bits per sample, low bits first,
// 00 = two copies of A1, 10 = one, 11 = none, 01 = missing; device code = count of A1 (0/1/2), 3 = missing.
// Each byte is four samples in both layouts, so a byte maps to a byte; the tail samples of the last byte are zeroed.
__global__ void bed_transcode_kernel(const uint8_t* __restrict__ bed, int64_t n, int64_t stride_in,
                                     uint8_t* __restrict__ bits, int64_t ldb) {
    const int64_t j = blockIdx.y;
    const int64_t nb = (n + 3) / 4;
    for (int64_t b = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; b < ldb; b += int64_t(gridDim.x) * blockDim.x) {
        unsigned out = 0;
        if (b < nb) {
            const unsigned in = bed[j * stride_in + b];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned f = (in >> (2 * k)) & 3u;
                // 00 -> 2, 01 -> 3 (missing), 10 -> 1, 11 -> 0
                const unsigned code = (b * 4 + k < n) ? ((0x1Eu >> (2 * f)) & 3u) : 0u;
                out |= code << (2 * k);
            }
        }
        bits[j * ldb + b] = uint8_t(out);
    }
}

// impute[j] = mean of the non-missing calls of column j (reference io/utils.hpp:10-31); one workgroup per column
template <class T>
__global__ __launch_bounds__(256) void snp_impute_kernel(const uint8_t* __restrict__ bits, int64_t n, int64_t ldb,
                                                         T* __restrict__ impute) {
    __shared__ unsigned long long red[3][4];
    const int64_t j = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t nb = (n + 3) / 4;
    unsigned long long c1 = 0, c2 = 0, c3 = 0;
    for (int64_t b = tid; b < nb; b += 256) {
        const unsigned byte = bits[j * ldb + b];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned c = (byte >> (2 * k)) & 3u;
            c1 += c == 1u; c2 += c == 2u; c3 += c == 3u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c1 += __shfl_xor(c1, off, 64); c2 += __shfl_xor(c2, off, 64); c3 += __shfl_xor(c3, off, 64);
    }
    if (lane == 0) { red[0][wv] = c1; red[1][wv] = c2; red[2][wv] = c3; }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long s1 = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        const unsigned long long s2 = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        const unsigned long long s3 = red[2][0] + red[2][1] + red[2][2] + red[2][3];
        const unsigned long long valid = (unsigned long long)n - s3;
        impute[j] = T(double(s1 + 2 * s2) / double(valid > 0 ? valid : 1));
    }
}

} // namespace

template <class T>
void launch_abs_grad(const T* grad, const int64_t* groups, const int64_t* group_sizes, int64_t G, const int32_t* slot,
                     const T* screen_beta, const T* penalty, T oma_lmda, T* abs_grad, hipStream_t s) {
    if (G <= 0) return;
    hipLaunchKernelGGL((abs_grad_kernel<T>), dim3(unsigned((G + 255) / 256)), dim3(256), 0, s, grad, groups,
                       group_sizes, G, slot, screen_beta, penalty, oma_lmda, abs_grad);
}

template <class T>
void launch_abs_grad_cons(const T* grad, const int64_t* groups, const int64_t* group_sizes, int64_t G, const int32_t* slot,
                          const T* screen_beta, const T* penalty, T oma_lmda, const T* clo, const T* chi, const T* cmu,
                          T* abs_grad, T* mu_out, hipStream_t s) {
    if (G <= 0) return;
    hipLaunchKernelGGL((abs_grad_cons_kernel<T>), dim3(unsigned((G + 255) / 256)), dim3(256), 0, s, grad, groups, group_sizes,
                       G, slot, screen_beta, penalty, oma_lmda, clo, chi, cmu, abs_grad, mu_out);
}

template <class T>
void launch_copy2d(const T* src, int64_t lds_, T* dst, int64_t ldd, int64_t rows, int64_t cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    for (int64_t j0 = 0; j0 < cols; j0 += 65535) {
        const unsigned cy = unsigned(cols - j0 < 65535 ? cols - j0 : 65535);
        hipLaunchKernelGGL((copy2d_kernel<T>), dim3(grid1d(rows, 256, 64), cy), dim3(256), 0, s, src + j0 * lds_, lds_,
                           dst + j0 * ldd, ldd, rows, cols);
    }
}
// vars[pos] = max(D_y[i, i], 0) for the blocks of a build batch (block y at D0 + sb.dst[y], leading dimension ldb): pos = the
// screen position of the block's i-th visit = list ? list[base + sb.off[y] + i] : base + sb.off[y] + i
namespace {
template <class T>
__global__ __launch_bounds__(128) void block_diag_vars_kernel(const T* __restrict__ D0, SyrkBatch sb, int ldb, int32_t base,
                                                              const int32_t* __restrict__ list, T* __restrict__ vars) {
    const int y = blockIdx.x, i = threadIdx.x;
    if (i >= sb.nb[y]) return;
    const int32_t k = base + sb.off[y] + i;
    const T v = D0[sb.dst[y] + i + int64_t(i) * ldb];
    vars[list ? list[k] : k] = v > T(0) ? v : T(0);
}
} // namespace
template <class T>
void launch_block_diag_vars(const T* D0, const SyrkBatch& sb, int ldb, int32_t base, const int32_t* list, T* vars, hipStream_t s) {
    if (sb.count <= 0) return;
    hipLaunchKernelGGL((block_diag_vars_kernel<T>), dim3(unsigned(sb.count)), dim3(128), 0, s, D0, sb, ldb, base, list, vars);
}
template <class T>
void launch_diag_vars(const T* C, int64_t ldc, int32_t pos0, int32_t cnt, T* vars, hipStream_t s) {
    if (cnt <= 0) return;
    hipLaunchKernelGGL((diag_vars_kernel<T>), dim3((cnt + 255) / 256), dim3(256), 0, s, C, ldc, pos0, cnt, vars);
}
// dst[i + c*ldd] = (X[rows ? rows[i] : i, cols ? cols[c] : c] - (centers ? centers[col] : 0)) / (scales ? scales[col] : 1):
// a new dense design from a resident one (standardize / subset, reference matrix_naive_standardize.ipp,
// matrix_naive_subset.ipp -- views there; materialised here, HBM is not the scarce resource)
template <class T, class Acc>
__global__ void derive_dense_kernel(Acc X, int64_t nout, int64_t pout, const int64_t* __restrict__ rows,
                                    const int64_t* __restrict__ cols, const T* __restrict__ centers,
                                    const T* __restrict__ scales, T* __restrict__ dst, int64_t ldd) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t c = blockIdx.y;
    if (i >= nout || c >= pout) return;
    const int64_t j = cols ? cols[c] : c, r = rows ? rows[i] : i;
    const T x = X.template load<1>(X.colptr(j), r, j).v[0];
    const T ce = centers ? centers[c] : T(0), sc = scales ? scales[c] : T(1);
    dst[i + c * ldd] = (x - ce) / sc;
}
// from(c): the accessor whose column 0 is column c of the source design (a chunk without a column list starts there)
template <class T, class From>
static void derive_dense_any(From from, int64_t nout, int64_t pout, const int64_t* rows, const int64_t* cols, const T* centers,
                             const T* scales, T* dst, int64_t ldd, hipStream_t s) {
    for (int64_t c0 = 0; c0 < pout; c0 += 65535) {
        const int64_t pc = std::min<int64_t>(65535, pout - c0);
        auto acc = from(cols ? 0 : c0);
        hipLaunchKernelGGL((derive_dense_kernel<T, decltype(acc)>), dim3((unsigned)((nout + 255) / 256), (unsigned)pc), dim3(256), 0,
                           s, acc, nout, pc, rows, cols ? cols + c0 : nullptr, centers ? centers + c0 : nullptr,
                           scales ? scales + c0 : nullptr, dst + c0 * ldd, ldd);
    }
}
template <class T>
void launch_derive_dense(const DenseView<T>& X, int64_t nout, int64_t pout, const int64_t* rows, const int64_t* cols,
                         const T* centers, const T* scales, T* dst, int64_t ldd, hipStream_t s) {
    derive_dense_any([&](int64_t c) { return DenseAcc<T>{X.X + c * X.ld, X.ld}; }, nout, pout, rows, cols, centers, scales, dst,
                     ldd, s);
}
template <class T>
void launch_derive_dense_snp(const SnpView& X, const T* impute, int64_t nout, int64_t pout, const int64_t* rows,
                             const int64_t* cols, const T* centers, const T* scales, T* dst, int64_t ldd, hipStream_t s) {
    derive_dense_any([&](int64_t c) { return SnpAcc<T>{X.bits + c * X.ldb, X.ldb, impute + c}; }, nout, pout, rows, cols, centers,
                     scales, dst, ldd, s);
}

// Rows / columns of a 2-bit design as another 2-bit design (matrix.subset on an SNP design: reference matrix_naive_subset.ipp
// wraps lazily; here the selected calls are re-packed, 2 bits per call, instead of being decoded into a dense copy).
// One thread per output byte: four calls gathered from the source column.
__global__ __launch_bounds__(256) void snp_subset_kernel(const uint8_t* __restrict__ src, int64_t ldb_src, int64_t nout, int64_t pout,
                                                          const int64_t* __restrict__ rows, const int64_t* __restrict__ cols,
                                                          uint8_t* __restrict__ dst, int64_t ldb_dst) {
    const int64_t bo = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const int64_t c = blockIdx.y;
    if (c >= pout || bo >= ldb_dst) return;
    const uint8_t* col = src + (cols ? cols[c] : c) * ldb_src;
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = bo * 4 + k;
        if (i < nout) {
            const int64_t r = rows ? rows[i] : i;
            out |= ((unsigned(col[r >> 2]) >> (2 * (r & 3))) & 3u) << (2 * k);
        }
    }
    dst[c * ldb_dst + bo] = uint8_t(out); // (padding bytes and padding calls are zeros)
}
void launch_snp_subset(const SnpView& X, int64_t nout, int64_t pout, const int64_t* rows, const int64_t* cols, uint8_t* dst,
                       int64_t ldb_dst, hipStream_t s) {
    for (int64_t c0 = 0; c0 < pout; c0 += 65535) {
        const int64_t pc = std::min<int64_t>(65535, pout - c0);
        hipLaunchKernelGGL(snp_subset_kernel, dim3((unsigned)((ldb_dst + 255) / 256), (unsigned)pc), dim3(256), 0, s,
                           X.bits + (cols ? 0 : c0 * X.ldb), X.ldb, nout, pc, rows, cols ? cols + c0 : nullptr, dst + c0 * ldb_dst,
                           ldb_dst);
    }
}
// out[c] = src[cols ? cols[c] : c]
template <class T>
__global__ void gather_cols_kernel(const T* __restrict__ src, const int64_t* __restrict__ cols, int64_t pout, T* __restrict__ out) {
    const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c < pout) out[c] = src[cols ? cols[c] : c];
}
template <class T>
void launch_gather_cols(const T* src, const int64_t* cols, int64_t pout, T* out, hipStream_t s) {
    hipLaunchKernelGGL((gather_cols_kernel<T>), dim3((unsigned)((pout + 255) / 256)), dim3(256), 0, s, src, cols, pout, out);
}

// CSC -> resident dense columns (matrix.sparse; reference matrix_naive_sparse.ipp keeps the CSC arrays and walks them per
// operation -- with 288 GB of HBM the design is expanded once and every operation is the dense streaming kernel).
// One workgroup per column; duplicate (row, col) entries add up, as they do in the reference's sparse dot products.
template <class T>
__global__ void csc_scatter_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                   const T* __restrict__ values, int64_t n, T* __restrict__ dst, int64_t ld) {
    const int64_t c = blockIdx.x;
    const int64_t b = indptr[c], e = indptr[c + 1];
    T* col = dst + c * ld;
    for (int64_t k = b + threadIdx.x; k < e; k += blockDim.x) {
        const int64_t i = indices[k];
        if (i >= 0 && i < n) atomicAdd(col + i, values[k]);
    }
}
template <class T>
void launch_csc_scatter(const int64_t* indptr, const int32_t* indices, const T* values, int64_t n, int64_t p, T* dst,
                        int64_t ld, hipStream_t s) {
    for (int64_t c0 = 0; c0 < p; c0 += 1 << 30) {
        const int64_t pc = std::min<int64_t>(int64_t(1) << 30, p - c0);
        hipLaunchKernelGGL((csc_scatter_kernel<T>), dim3((unsigned)pc), dim3(256), 0, s, indptr + c0, indices, values, n,
                           dst + c0 * ld, ld);
    }
}

template <class T>
void launch_transpose(const T* src, int64_t n, int64_t p, T* dst, int64_t ld, hipStream_t s) {
    if (n <= 0 || p <= 0) return;
    const int64_t gy_total = (n + 31) / 32;
    for (int64_t y0 = 0; y0 < gy_total; y0 += 65535) {
        const unsigned gy = unsigned(gy_total - y0 < 65535 ? gy_total - y0 : 65535);
        hipLaunchKernelGGL((transpose_kernel<T>), dim3(unsigned((p + 31) / 32), gy), dim3(32, 8), 0, s,
                           src + y0 * 32 * p, n - y0 * 32, p, dst + y0 * 32, ld);
    }
}
void launch_pack_snp(const int8_t* calldata, int64_t n, int64_t p, uint8_t* bits, int64_t ldb, hipStream_t s) {
    if (n <= 0 || p <= 0) return;
    for (int64_t j0 = 0; j0 < p; j0 += 65535) {
        const unsigned cy = unsigned(p - j0 < 65535 ? p - j0 : 65535);
        hipLaunchKernelGGL(pack_snp_kernel, dim3(grid1d(ldb, 256, 256), cy), dim3(256), 0, s, calldata + j0 * n, n, p,
                           bits + j0 * ldb, ldb);
    }
}

void launch_bed_transcode(const uint8_t* bed, int64_t n, int64_t p, int64_t stride_in, uint8_t* bits, int64_t ldb,
                          hipStream_t s) {
    if (n <= 0 || p <= 0) return;
    for (int64_t j0 = 0; j0 < p; j0 += 65535) {
        const unsigned cy = unsigned(p - j0 < 65535 ? p - j0 : 65535);
        hipLaunchKernelGGL(bed_transcode_kernel, dim3(grid1d(ldb, 256, 256), cy), dim3(256), 0, s, bed + j0 * stride_in, n,
                           stride_in, bits + j0 * ldb, ldb);
    }
}
template <class T>
void launch_snp_impute(const uint8_t* bits, int64_t n, int64_t p, int64_t ldb, T* impute, hipStream_t s) {
    if (p <= 0) return;
    hipLaunchKernelGGL((snp_impute_kernel<T>), dim3((unsigned)p), dim3(256), 0, s, bits, n, ldb, impute);
}
template void launch_snp_impute<double>(const uint8_t*, int64_t, int64_t, int64_t, double*, hipStream_t);
template void launch_snp_impute<float>(const uint8_t*, int64_t, int64_t, int64_t, float*, hipStream_t);

#define INST(T)                                                                                                        \
    template void launch_abs_grad<T>(const T*, const int64_t*, const int64_t*, int64_t, const int32_t*, const T*,      \
                                     const T*, T, T*, hipStream_t);                                                    \
    template void launch_abs_grad_cons<T>(const T*, const int64_t*, const int64_t*, int64_t, const int32_t*, const T*, \
                                          const T*, T, const T*, const T*, const T*, T*, T*, hipStream_t);             \
    template void launch_copy2d<T>(const T*, int64_t, T*, int64_t, int64_t, int64_t, hipStream_t);                     \
    template void launch_diag_vars<T>(const T*, int64_t, int32_t, int32_t, T*, hipStream_t);                           \
    template void launch_block_diag_vars<T>(const T*, const SyrkBatch&, int, int32_t, const int32_t*, T*, hipStream_t); \
    template void launch_csc_scatter<T>(const int64_t*, const int32_t*, const T*, int64_t, int64_t, T*, int64_t, hipStream_t);\
    template void launch_transpose<T>(const T*, int64_t, int64_t, T*, int64_t, hipStream_t);                            \
    template void launch_derive_dense<T>(const DenseView<T>&, int64_t, int64_t, const int64_t*, const int64_t*, const T*, \
                                         const T*, T*, int64_t, hipStream_t);                                          \
    template void launch_derive_dense_snp<T>(const SnpView&, const T*, int64_t, int64_t, const int64_t*, const int64_t*, \
                                             const T*, const T*, T*, int64_t, hipStream_t);                              \
    template void launch_gather_cols<T>(const T*, const int64_t*, int64_t, T*, hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
