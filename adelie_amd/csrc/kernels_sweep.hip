// kernels_sweep.hip — HBM-bound streaming kernels over the resident design (gfx950 / CDNA4).
//
//   sweep      out[c] = X[:,col(c)] . v            replaces MatrixNaiveDense::mul / bmul / cmul / sq_mul
//                                                  (reference matrix_naive_dense.ipp:23-34,61-80,125-146,199-217,
//                                                   kernels matrix/utils.hpp:131-161,194-269) and the invariance
//                                                  sweep of solver_gaussian_naive.hpp:377-393 (incl. the
//                                                  `grad -= resid_sum * X_means` epilogue, fused).
//   axpy_cols  out += sign * sum_k coef_k X[:,col_k]  replaces ctmul / btmul (matrix_naive_dense.ipp:49-59,106-123)
//                                                  and applies the residual update of a whole CD fit at once.
//   sp_tmul    out[l,:] = sum_e V[l,e] X[:,idx_e]  replaces MatrixNaiveDense::sp_tmul (:219-256).
//
// Design notes (MI355X): one column is n*sizeof(T) contiguous bytes (800 KB at n=100k f64).  A sweep block owns a
// panel of CB columns and walks the rows with 16-byte loads per lane (1 KiB per wave-instruction); the vector
// v = w*r (<= 4 MB) is read through L2 once per panel instead of once per column, the CB column streams are
// independent loads in flight (no LDS staging needed: there is no reuse of X), lanes reduce with wave shuffles
// (64-wide), waves through a few LDS words.  Grid = panels x row-splits >> 256 CUs; partial sums of the row
// splits are combined by a second tiny kernel so results are deterministic (no float atomics).
// The filtered invariance sweep built on these is kernels_filter.hip; building and converting designs is kernels_convert.hip.
#include "sweep_common.hpp"
#include <algorithm>

namespace ahip {

namespace {

// ---- sweep ----------------------------------------------------------------------------------------
template <class T, class Acc, int CB, int VEC, bool SQ>
__global__ __launch_bounds__(kThreads) void sweep_kernel(Acc X, const T* __restrict__ v, T* __restrict__ out,
                                                         int64_t n, int64_t c0, int64_t ncols,
                                                         const int32_t* __restrict__ cols, int64_t rows_per_split,
                                                         int nsplit, const T* __restrict__ sub_scale,
                                                         const T* __restrict__ sub_vec) {
    const int tid = threadIdx.x;
    const int64_t cb = blockIdx.x;
    const int split = blockIdx.y;
    const int64_t r0 = int64_t(split) * rows_per_split;
    const int64_t r1 = min(n, r0 + rows_per_split);

    int64_t cj[CB];
    decltype(X.colptr(0)) cp[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k) {
        int64_t c = cb * CB + k;
        if (c >= ncols) c = ncols - 1; // duplicate work on the tail panel, discarded below
        cj[k] = cols ? int64_t(cols[c]) : c0 + c;
        cp[k] = X.colptr(cj[k]);
    }
    T acc[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k) acc[k] = T(0);

    const int64_t body_end = r0 + ((r1 - r0) / VEC) * VEC;
#pragma unroll 2
    for (int64_t i = r0 + int64_t(tid) * VEC; i < body_end; i += int64_t(kThreads) * VEC) {
        const Pack<T, VEC> vv = load_vec<T, VEC>(v + i);
        Pack<T, VEC> xx[CB];
#pragma unroll
        for (int k = 0; k < CB; ++k) xx[k] = X.template load<VEC>(cp[k], i, cj[k]);
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T x = SQ ? xx[k].v[e] * xx[k].v[e] : xx[k].v[e];
                acc[k] = fma(x, vv.v[e], acc[k]);
            }
    }
    // row tail (< VEC rows)
    for (int64_t i = body_end + tid; i < r1; i += kThreads) {
        const T vi = v[i];
#pragma unroll
        for (int k = 0; k < CB; ++k) {
            const T x0 = X.template load<1>(cp[k], i, cj[k]).v[0];
            const T x = SQ ? x0 * x0 : x0;
            acc[k] = fma(x, vi, acc[k]);
        }
    }

    __shared__ T red[kThreads / 64][CB];
    panel_epilogue<false>(acc, red, cb, ncols, c0, cols, nullptr, out, split, nsplit, sub_scale, sub_vec);
}

template <class T>
__global__ void sweep_reduce_kernel(const T* __restrict__ part, T* __restrict__ out, int64_t ncols, int nsplit,
                                    int64_t c0, const int32_t* __restrict__ cols, const T* __restrict__ sub_scale,
                                    const T* __restrict__ sub_vec) {
    const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= ncols) return;
    T s = T(0);
    for (int r = 0; r < nsplit; ++r) s += part[int64_t(r) * ncols + c];
    out[c] = centred(s, cols ? int64_t(cols[c]) : c0 + c, sub_scale, sub_vec);
}

template <class T, class Acc, int VEC>
void sweep_dispatch(Acc acc, const T* v, T* out, int64_t n, int64_t c0, int64_t ncols, const int32_t* cols,
                    const T* sub_scale, const T* sub_vec, bool square, T* work, hipStream_t s) {
    if (ncols <= 0) return;
    int64_t blocks_c, rows_per_split;
    int nsplit;
    sweep_shape(n, ncols, VEC, blocks_c, nsplit, rows_per_split);
    dim3 grid((unsigned)blocks_c, (unsigned)nsplit);
    T* dst = nsplit == 1 ? out : work;
    const auto kernel = square ? sweep_kernel<T, Acc, kSweepCB, VEC, true> : sweep_kernel<T, Acc, kSweepCB, VEC, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, s, acc, v, dst, n, c0, ncols, cols, rows_per_split, nsplit, sub_scale,
                       sub_vec);
    if (nsplit > 1) launch_sweep_reduce(work, out, ncols, nsplit, c0, cols, sub_scale, sub_vec, s);
}

// ---- axpy_cols --------------------------------------------------------------------------------------
template <class T, class Acc, int VEC>
__global__ __launch_bounds__(kThreads) void axpy_cols_kernel(Acc X, int64_t n, const int32_t* __restrict__ cols,
                                                             const T* __restrict__ coef,
                                                             const int32_t* __restrict__ count_dev, int32_t count,
                                                             T sign, T* __restrict__ out) {
    const int K = count_dev ? count_dev[0] : count;
    if (K <= 0) return;
    const int64_t i = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * VEC;
    if (i >= n) return;
    if (i + VEC <= n) {
        T acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = T(0);
        int k = 0;
        for (; k + 4 <= K; k += 4) {
            Pack<T, VEC> xx[4];
            T cf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t j = cols[k + u];
                cf[u] = coef[k + u];
                xx[u] = X.template load<VEC>(X.colptr(j), i, j);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = fma(cf[u], xx[u].v[e], acc[e]);
        }
        for (; k < K; ++k) {
            const int64_t j = cols[k];
            const T cf = coef[k];
            const Pack<T, VEC> xx = X.template load<VEC>(X.colptr(j), i, j);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = fma(cf, xx.v[e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) out[i + e] += sign * acc[e];
    } else {
        for (int64_t r = i; r < n; ++r) {
            T acc = T(0);
            for (int k = 0; k < K; ++k) {
                const int64_t j = cols[k];
                acc = fma(coef[k], X.template load<1>(X.colptr(j), r, j).v[0], acc);
            }
            out[r] += sign * acc;
        }
    }
}

template <class T, class Acc, int VEC>
__global__ __launch_bounds__(kThreads) void sp_tmul_kernel(Acc X, int64_t n, const int64_t* __restrict__ indptr,
                                                           const int64_t* __restrict__ indices,
                                                           const T* __restrict__ values, T* __restrict__ out) {
    const int64_t l = blockIdx.y;
    const int64_t e0 = indptr[l], e1 = indptr[l + 1];
    const int64_t i = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * VEC;
    if (i >= n) return;
    T* o = out + l * n;
    if (i + VEC <= n) {
        T acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = T(0);
        int64_t k = e0;
        for (; k + 4 <= e1; k += 4) {
            Pack<T, VEC> xx[4];
            T cf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t j = indices[k + u];
                cf[u] = values[k + u];
                xx[u] = X.template load<VEC>(X.colptr(j), i, j);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] = fma(cf[u], xx[u].v[e], acc[e]);
        }
        for (; k < e1; ++k) {
            const int64_t j = indices[k];
            const T cf = values[k];
            const Pack<T, VEC> xx = X.template load<VEC>(X.colptr(j), i, j);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = fma(cf, xx.v[e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[i + e] = acc[e];
    } else {
        for (int64_t r = i; r < n; ++r) {
            T acc = T(0);
            for (int64_t k = e0; k < e1; ++k) {
                const int64_t j = indices[k];
                acc = fma(values[k], X.template load<1>(X.colptr(j), r, j).v[0], acc);
            }
            o[r] = acc;
        }
    }
}

template <class T>
__global__ void vmul_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, int64_t n) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        out[i] = a[i] * b[i];
}
template <class T>
__global__ void fill_kernel(T* __restrict__ out, T value, int64_t n) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        out[i] = value;
}

} // namespace

template <class T>
void launch_sweep_reduce(const T* part, T* out, int64_t ncols, int nsplit, int64_t c0, const int32_t* cols, const T* sub_scale,
                         const T* sub_vec, hipStream_t s) {
    hipLaunchKernelGGL((sweep_reduce_kernel<T>), dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, s, part, out, ncols, nsplit,
                       c0, cols, sub_scale, sub_vec);
}

// row splits of the nibble-table sweep of a 2-bit design (sweep_snp_lut_kernel): ~8000 workgroups of 256 columns (five are
// resident per compute unit: six or more rounds, so that the last, partial round costs little), at least eight 256-row tiles
// per split
constexpr int kLutTile = 256;
inline void lut_shape(int64_t n, int64_t ncols, int64_t& blocks_c, int64_t& ns, int64_t& rps) {
    blocks_c = (ncols + kThreads - 1) / kThreads;
    ns = std::max<int64_t>(1, (8192 + blocks_c - 1) / blocks_c);
    ns = std::min<int64_t>(std::min(ns, std::max<int64_t>(1, n / (int64_t(kLutTile) * 8))), 65535);
    rps = (n + ns - 1) / ns;
    rps = ((rps + 2 * kLutTile - 1) / (2 * kLutTile)) * (2 * kLutTile); // whole 128-byte lines of a column (two tiles)
    ns = (n + rps - 1) / rps;
}
int64_t sweep_work_elems(int64_t n, int64_t ncols) {
    if (ncols <= 0) return 0;
    int64_t blocks_c, rps;
    int ns;
    sweep_shape(n, ncols, 1, blocks_c, ns, rps); // VEC=1 gives the largest split count
    int64_t a = int64_t(ns) * ncols;
    sweep_shape(n, ncols, 4, blocks_c, ns, rps);
    int64_t b = int64_t(ns) * ncols;
    int64_t lns;
    lut_shape(n, ncols, blocks_c, lns, rps);
    return std::max(std::max(a, b), lns * ncols) + 16;
}

template <class T>
void launch_vmul(const T* a, const T* b, T* out, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL((vmul_kernel<T>), dim3(grid1d(n, 256)), dim3(256), 0, s, a, b, out, n);
}
template <class T>
void launch_fill(T* out, T value, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL((fill_kernel<T>), dim3(grid1d(n, 256)), dim3(256), 0, s, out, value, n);
}

template <class T>
void launch_sweep(const DenseView<T>& X, const T* v, T* out, int64_t c0, int64_t ncols, const int32_t* cols,
                  const T* sub_scale, const T* sub_vec, bool square, T* work, hipStream_t s) {
    DenseAcc<T> acc{X.X, X.ld};
    if (dense_vec_ok(X) && (reinterpret_cast<uintptr_t>(v) % 16) == 0)
        sweep_dispatch<T, DenseAcc<T>, VecOf<T>::N>(acc, v, out, X.n, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
    else
        sweep_dispatch<T, DenseAcc<T>, 1>(acc, v, out, X.n, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
}
// ---- 2-bit sweep through nibble tables ------------------------------------------------------------------------------
// out[c] = sum_i x_ic v_i with x in {0, 1, 2, impute_c}.  The decode-and-multiply form above spends five integer / convert
// instructions and a multiply-add per call and is bound by their issue (5.8 ms for the 500k x 50k design of config 4, 1.08 TB/s).
// Here a thread owns a COLUMN and a workgroup walks row tiles of TR = 256 rows: per tile it first builds, in LDS, for every
// pair of rows (i, i+1) the 16 possible contributions of a nibble (two calls),
//     T012[b] = c0' v_i + c1' v_{i+1}   (c' = code if code < 3 else 0),     T3[b] = [c0 = 3] v_i + [c1 = 3] v_{i+1},
// — the vector v is the same for all columns, so a table serves every column of the workgroup — and then every thread adds
// one T012 entry per nibble of its column and one entry per BYTE of a second table that holds, for four rows, the sum of v over
// any subset of them (indexed by the four missing-call flags of the byte: three mask operations per word bring them
// together) — three LDS reads per four calls where a T3 entry per nibble made it four, the kernel being bound by what LDS
// delivers; the imputed value enters once at the end, S012 + impute_c * S3.  A table of 16 entries of 8 bytes is one row of LDS banks:
// any mix of indices over the lanes is conflict-free.  Columns are 128-byte aligned and padded (SnpView::ldb): a line of a
// column is two tiles.  Fixed summation order; row splits leave partials for sweep_reduce_kernel as above.
constexpr int LUT_TR = 256;
static_assert(LUT_TR == 256, "lut_shape's tile");
// How the columns come in.  A thread owning a column and fetching it 16 bytes at a time makes EIGHT separate requests for every
// 128-byte line, each wave instruction touching 64 different lines; with ~20 resident waves per compute unit the lines leave
// the L1 and even the L2 (5 MB in flight per XCD against 4 MB) between two of them: 13.6-14.3 GB of counter traffic per sweep
// of the 6.25 GB design (2.2 x; profiles/r05_cfg4_*, and unchanged when a thread merely takes the whole line in one trip:
// profiles/r06_cfg4_lut_line_per_trip.txt).  So the workgroup fetches cooperatively: per trip of 512 rows (one line per
// column) eight adjacent lanes take the eight 16-byte pieces of one column's line -- every line is requested once, whole, by
// one instruction -- and the pieces go through a 32 KB staging array in LDS (rotated by the column index: conflict-free in
// both directions) from which every thread reads back its own column.  The next trip's pieces are in flight while the
// current one is looked up.
// SQ: the squared design (x^2: the weighted column variances of an IRLS iteration): the table holds c'^2, the end impute^2.
template <class T, bool SQ>
__global__ __launch_bounds__(kThreads) void sweep_snp_lut_kernel(const uint8_t* __restrict__ bits, int64_t ldb,
                                                                 const T* __restrict__ impute, const T* __restrict__ v,
                                                                 T* __restrict__ out, int64_t n, int64_t c0, int64_t ncols,
                                                                 const int32_t* __restrict__ cols, int64_t rows_per_split,
                                                                 int nsplit, const T* __restrict__ sub_scale,
                                                                 const T* __restrict__ sub_vec) {
    static_assert(kThreads == 256, "256 columns per workgroup, 8 lanes per line");
    constexpr int NP = LUT_TR / 2;              // row pairs per tile
    typedef unsigned u4_t __attribute__((ext_vector_type(4)));
    constexpr int NQ = LUT_TR / 4;              // row quads per tile
    __shared__ T t012[NP][16];
    __shared__ T t3q[NQ][16];                   // missing calls, four rows per look-up: entry = sum of v over the set bits
    __shared__ u4_t stage[kThreads * 8];        // [column][piece rotated by the column]
    __shared__ int64_t cofs[kThreads];          // byte offset of the workgroup's columns
    const int tid = threadIdx.x;
    const int split = blockIdx.y;
    const int64_t r0 = int64_t(split) * rows_per_split; // (a multiple of 2 * LUT_TR: whole lines)
    const int64_t r1 = min(n, r0 + rows_per_split);
    int64_t c = int64_t(blockIdx.x) * kThreads + tid;
    const bool live = c < ncols;
    if (!live) c = ncols - 1;
    const int64_t cj = cols ? int64_t(cols[c]) : c0 + c;
    cofs[tid] = cj * ldb;
    __syncthreads();
    // fetch role: piece tid & 7 of the lines of columns (tid >> 3) + 32 u
    const int fp = tid & 7, fc = tid >> 3;
    const uint8_t* fptr[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) fptr[u] = bits + cofs[fc + 32 * u] + fp * 16;
    // table role of this thread: pair tid / 2, entries 8 * (tid & 1) .. + 8 of T012; quad tid / 4, entries 4 * (tid & 3) .. + 4 of T3
    const int tp = tid >> 1, te0 = (tid & 1) * 8;
    const int tq = tid >> 2, tqe0 = (tid & 3) * 4;
    T a = T(0), b = T(0);
    u4_t w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(fptr[u] + r0 / 4));
    for (int64_t base = r0; base < r1; base += 2 * LUT_TR) {
        __syncthreads(); // the previous trip's lookups are done: the staging array is free
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int col = fc + 32 * u;
            stage[col * 8 + ((fp + col) & 7)] = w[u];
        }
        const int64_t nbase = base + 2 * LUT_TR;
        if (nbase < r1) {
#pragma unroll
            for (int u = 0; u < 8; ++u) w[u] = __builtin_nontemporal_load(reinterpret_cast<const u4_t*>(fptr[u] + nbase / 4));
        }
        T vv[4], vq[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t i0 = base + h * LUT_TR + 2 * tp;
            vv[2 * h] = i0 < r1 ? v[i0] : T(0);
            vv[2 * h + 1] = i0 + 1 < r1 ? v[i0 + 1] : T(0);
            const int64_t j0 = base + h * LUT_TR + 4 * tq;
#pragma unroll
            for (int k = 0; k < 4; ++k) vq[4 * h + k] = j0 + k < r1 ? v[j0 + k] : T(0);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const T v0 = vv[2 * h], v1 = vv[2 * h + 1];
            if (h == 1) __syncthreads(); // tile 0's lookups are done
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int idx = te0 + e, k0 = idx & 3, k1 = idx >> 2;
                t012[tp][idx] = (k0 < 3 ? T(SQ ? k0 * k0 : k0) : T(0)) * v0 + (k1 < 3 ? T(SQ ? k1 * k1 : k1) : T(0)) * v1;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { // the missing calls of FOUR rows per entry (fixed order of the additions: rows ascending)
                const int idx = tqe0 + e;
                t3q[tq][idx] = (((idx & 1) ? vq[4 * h] : T(0)) + ((idx & 2) ? vq[4 * h + 1] : T(0))) +
                               (((idx & 4) ? vq[4 * h + 2] : T(0)) + ((idx & 8) ? vq[4 * h + 3] : T(0)));
            }
            __syncthreads(); // (h == 0: also makes the staged pieces visible)
            u4_t wd[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) wd[u] = stage[tid * 8 + ((4 * h + u + tid) & 7)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int hh = 0; hh < 4; ++hh) {
                    const unsigned wq = wd[u][hh];
                    // bit 2k of `ms`: call k of the word is missing (code 3); then the four flags of every byte in its low nibble
                    unsigned ms = wq & (wq >> 1) & 0x55555555u;
                    ms = (ms | (ms >> 1)) & 0x33333333u;
                    ms = (ms | (ms >> 2)) & 0x0F0F0F0Fu;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int pr = (u * 4 + hh) * 8 + k; // row pair of this nibble (compile-time)
                        a += t012[pr][(wq >> (4 * k)) & 15u];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int qr = (u * 4 + hh) * 4 + k; // row quad of this byte
                        b += t3q[qr][(ms >> (8 * k)) & 15u];
                    }
                }
            }
        }
    }
    if (!live) return;
    const T imp = impute[cj];
    store_sum(fma(SQ ? imp * imp : imp, b, a), out, c, cj, split, nsplit, ncols, sub_scale, sub_vec);
}

template <class T>
void launch_sweep_snp(const SnpView& X, const T* impute, const T* v, T* out, int64_t c0, int64_t ncols,
                      const int32_t* cols, const T* sub_scale, const T* sub_vec, bool square, T* work, hipStream_t s) {
    if (ncols >= 512 && X.n >= 4096 && X.ldb % 128 == 0 && (reinterpret_cast<uintptr_t>(X.bits) % 128) == 0) {
        // the same partial layout and reduce as sweep_dispatch (`work`: sweep_work_elems covers lut_shape's splits)
        int64_t blocks_c, ns, rps;
        lut_shape(X.n, ncols, blocks_c, ns, rps);
        T* dst = ns == 1 ? out : work;
        const auto kernel = square ? sweep_snp_lut_kernel<T, true> : sweep_snp_lut_kernel<T, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks_c, (unsigned)ns), dim3(kThreads), 0, s, X.bits, X.ldb, impute, v, dst,
                           X.n, c0, ncols, cols, rps, int(ns), sub_scale, sub_vec);
        if (ns > 1) launch_sweep_reduce(work, out, ncols, int(ns), c0, cols, sub_scale, sub_vec, s);
        return;
    }
    SnpAcc<T> acc{X.bits, X.ldb, impute};
    sweep_dispatch<T, SnpAcc<T>, VecOf<T>::N>(acc, v, out, X.n, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
}

// ---- axpy_cols and sp_tmul over any accessor; vec_ok: the design's columns can be read 16 bytes at a time -----------------
// (SCALAR_TOO = false: the accessor always takes the vector path, and its scalar kernel is not compiled)
template <bool SCALAR_TOO, class T, class Acc>
static void axpy_cols_any(Acc acc, int64_t n, bool vec_ok, const int32_t* cols, const T* coef, const int32_t* count_dev,
                          int32_t count, T sign, T* out, hipStream_t s) {
    if (n <= 0 || (!count_dev && count <= 0)) return;
    constexpr int V = VecOf<T>::N;
    auto kernel = axpy_cols_kernel<T, Acc, V>;
    if constexpr (SCALAR_TOO) {
        if (!vec_ok) kernel = axpy_cols_kernel<T, Acc, 1>;
    } else vec_ok = true;
    const int64_t rows = int64_t(kThreads) * (vec_ok ? V : 1); // rows per workgroup
    hipLaunchKernelGGL(kernel, dim3(unsigned((n + rows - 1) / rows)), dim3(kThreads), 0, s, acc, n, cols, coef, count_dev,
                       count, sign, out);
}
// (the vector kernel has no row tail of its own: n must be whole vectors as well)
template <class T, class Acc>
static void sp_tmul_any(Acc acc, int64_t n, bool vec_ok, int64_t L, const int64_t* indptr, const int64_t* indices,
                        const T* values, T* out, hipStream_t s) {
    if (L <= 0 || n <= 0) return;
    constexpr int V = VecOf<T>::N;
    const bool vec = vec_ok && n % V == 0;
    const auto kernel = vec ? sp_tmul_kernel<T, Acc, V> : sp_tmul_kernel<T, Acc, 1>;
    const int64_t rows = int64_t(kThreads) * (vec ? V : 1); // rows per workgroup
    for (int64_t l0 = 0; l0 < L; l0 += 65535) {
        const unsigned ly = unsigned(L - l0 < 65535 ? L - l0 : 65535);
        hipLaunchKernelGGL(kernel, dim3(unsigned((n + rows - 1) / rows), ly), dim3(kThreads), 0, s, acc, n, indptr + l0,
                           indices, values, out + l0 * n);
    }
}

template <class T>
void launch_axpy_cols(const DenseView<T>& X, const int32_t* cols, const T* coef, const int32_t* count_dev,
                      int32_t count, T sign, T* out, hipStream_t s) {
    axpy_cols_any<true>(DenseAcc<T>{X.X, X.ld}, X.n, dense_vec_ok(X), cols, coef, count_dev, count, sign, out, s);
}
template <class T>
void launch_axpy_cols_snp(const SnpView& X, const T* impute, const int32_t* cols, const T* coef,
                          const int32_t* count_dev, int32_t count, T sign, T* out, hipStream_t s) {
    axpy_cols_any<false>(SnpAcc<T>{X.bits, X.ldb, impute}, X.n, true, cols, coef, count_dev, count, sign, out, s);
}

template <class T>
void launch_sp_tmul(const DenseView<T>& X, int64_t L, const int64_t* indptr, const int64_t* indices, const T* values,
                    T* out, hipStream_t s) {
    sp_tmul_any(DenseAcc<T>{X.X, X.ld}, X.n, dense_vec_ok(X), L, indptr, indices, values, out, s);
}
template <class T>
void launch_sp_tmul_snp(const SnpView& X, const T* impute, int64_t L, const int64_t* indptr, const int64_t* indices,
                        const T* values, T* out, hipStream_t s) {
    sp_tmul_any(SnpAcc<T>{X.bits, X.ldb, impute}, X.n, true, L, indptr, indices, values, out, s);
}

// ---- a design made of pieces (kernels.hpp: PiecesView) -----------------------------------------------------------------------
template <class T>
int64_t sweep_work_elems_pieces(const PiecesView<T>& X, int64_t c0, int64_t ncols) {
    int64_t need = sweep_work_elems(X.n, ncols); // (a sweep over a column list)
    PieceRange rg[kMaxPieces];
    const int nr = pieces_split(X.first, X.k, c0, ncols, rg);
    for (int r = 0; r < nr; ++r) need = std::max(need, sweep_work_elems(X.n, rg[r].count));
    return need;
}
template <class T>
void launch_sweep_pieces(const PiecesView<T>& X, const T* v, T* out, int64_t c0, int64_t ncols, const int32_t* cols,
                         const T* sub_scale, const T* sub_vec, bool square, T* work, hipStream_t s) {
    if (ncols <= 0) return;
    if (!cols) { // a column range: piece by piece with the pieces' own launches (in order on s: they share `work`)
        PieceRange rg[kMaxPieces];
        const int nr = pieces_split(X.first, X.k, c0, ncols, rg);
        for (int r = 0; r < nr; ++r) {
            const int m = rg[r].piece;
            const T* sv = sub_vec ? sub_vec + X.first[m] : nullptr; // (the piece's launch indexes it by its own columns)
            if (X.is_snp(m))
                launch_sweep_snp<T>(X.snp_piece(m), X.impute[m], v, out + rg[r].out0, rg[r].local0, rg[r].count, nullptr, sub_scale, sv,
                                    square, work, s);
            else
                launch_sweep<T>(X.dense_piece(m), v, out + rg[r].out0, rg[r].local0, rg[r].count, nullptr, sub_scale, sv, square, work, s);
        }
        return;
    }
    const PiecesAcc<T> acc = pieces_acc<T>(X);
    if (X.vec_ok() && (reinterpret_cast<uintptr_t>(v) % 16) == 0)
        sweep_dispatch<T, PiecesAcc<T>, VecOf<T>::N>(acc, v, out, X.n, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
    else
        sweep_dispatch<T, PiecesAcc<T>, 1>(acc, v, out, X.n, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
}
template <class T>
void launch_axpy_cols_pieces(const PiecesView<T>& X, const int32_t* cols, const T* coef, const int32_t* count_dev, int32_t count,
                             T sign, T* out, hipStream_t s) {
    axpy_cols_any<true>(pieces_acc<T>(X), X.n, X.vec_ok(), cols, coef, count_dev, count, sign, out, s);
}
template <class T>
void launch_sp_tmul_pieces(const PiecesView<T>& X, int64_t L, const int64_t* indptr, const int64_t* indices, const T* values,
                           T* out, hipStream_t s) {
    sp_tmul_any(pieces_acc<T>(X), X.n, X.vec_ok(), L, indptr, indices, values, out, s);
}

#define INST(T)                                                                                                        \
    template int64_t sweep_work_elems_pieces<T>(const PiecesView<T>&, int64_t, int64_t);                               \
    template void launch_sweep_pieces<T>(const PiecesView<T>&, const T*, T*, int64_t, int64_t, const int32_t*, const T*, \
                                         const T*, bool, T*, hipStream_t);                                             \
    template void launch_axpy_cols_pieces<T>(const PiecesView<T>&, const int32_t*, const T*, const int32_t*, int32_t, T, T*, \
                                             hipStream_t);                                                             \
    template void launch_sp_tmul_pieces<T>(const PiecesView<T>&, int64_t, const int64_t*, const int64_t*, const T*, T*, \
                                           hipStream_t);                                                               \
    template void launch_vmul<T>(const T*, const T*, T*, int64_t, hipStream_t);                                        \
    template void launch_fill<T>(T*, T, int64_t, hipStream_t);                                                         \
    template void launch_sweep<T>(const DenseView<T>&, const T*, T*, int64_t, int64_t, const int32_t*, const T*,       \
                                  const T*, bool, T*, hipStream_t);                                                    \
    template void launch_sweep_snp<T>(const SnpView&, const T*, const T*, T*, int64_t, int64_t, const int32_t*,        \
                                      const T*, const T*, bool, T*, hipStream_t);                                      \
    template void launch_axpy_cols<T>(const DenseView<T>&, const int32_t*, const T*, const int32_t*, int32_t, T, T*,   \
                                      hipStream_t);                                                                    \
    template void launch_axpy_cols_snp<T>(const SnpView&, const T*, const int32_t*, const T*, const int32_t*, int32_t, \
                                          T, T*, hipStream_t);                                                         \
    template void launch_sp_tmul<T>(const DenseView<T>&, int64_t, const int64_t*, const int64_t*, const T*, T*,        \
                                    hipStream_t);                                                                      \
    template void launch_sp_tmul_snp<T>(const SnpView&, const T*, int64_t, const int64_t*, const int64_t*, const T*,   \
                                        T*, hipStream_t);                                                              \
    template void launch_sweep_reduce<T>(const T*, T*, int64_t, int, int64_t, const int32_t*, const T*, const T*,      \
                                         hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
