// kernels_factor.hip — one-hot and pairwise-interaction designs built from a table of features Z (gfx950 / CDNA4).
//
//   factor_expand   X = the expanded (n, P) design, written once from the resident Z: replaces the lazy column generation of
//                   MatrixNaiveOneHotDense / MatrixNaiveInteractionDense (reference matrix_naive_one_hot.ipp,
//                   matrix_naive_interaction.ipp:78-200) -- every other kernel of this library then streams X as a dense design.
//   sweep_factor    out[c] = X[:, c] . v for ALL P columns without reading X: a block of L (one-hot) or l0 * l1 (interaction)
//                   columns is a function of one or two columns of Z, so a workgroup that owns up to kFactorChunk columns of one
//                   block reads z_a, z_b and v once per row and forms the columns' entries in registers (compare-and-select).
//                   n * (2 or 3) values per chunk instead of n per column: the traffic of the full gradient sweep
//                   (solver_gaussian_naive.hpp:377-393) drops by about kFactorChunk / 3 on wide blocks and the kernel is bound
//                   by vector-ALU issue (3 to 5 instructions per entry) instead of HBM.
//
// Both kernels decide a row's level with factor_level(), so the sweep sums exactly the entries the expansion stores.  The sweep
// is order-deterministic: a thread adds its rows ascending, lanes and waves are combined in a fixed order (wavered.hpp), the
// row slices leave partial sums in `work` that a second kernel adds in slice order.  No floating-point atomics.
#include "kernels.hpp"
#include "wavered.hpp"
#include <algorithm>

namespace ahip {

namespace {

constexpr int kThreads = 256;
constexpr int CH = kFactorChunk;

// level of a discrete value: z itself when it is one of 0 .. l - 1, else -1 (a row that belongs to no level: its block
// entries are all zero, like the reference's `==`)
template <class T>
__device__ __forceinline__ int factor_level(T z, int l) {
    const bool in = z >= T(0) && z < T(l); // (false for NaN)
    const T zc = in ? z : T(0);
    const int i = int(zc);
    return (in && T(i) == zc) ? i : -1;
}

// entry of the block's product column (k0, k1) in a row whose two Z values are a and b.  `flags` as in FactorBlock.
template <class T>
__device__ __forceinline__ T factor_entry(const FactorBlock& bk, T a, T b, int k0, int k1) {
    const T fa = (bk.flags & 1) ? (factor_level(a, bk.l0) == k0 ? T(1) : T(0)) : (k0 ? a : T(1));
    const T fb = (bk.flags & 4) ? T(1) : ((bk.flags & 2) ? (factor_level(b, bk.l1) == k1 ? T(1) : T(0)) : (k1 ? b : T(1)));
    return fa * fb; // 0, 1, a value of Z, or one product of two values of Z
}

template <class T>
__global__ __launch_bounds__(kThreads) void factor_expand_kernel(FactorView<T> F, int64_t chunk0, T* __restrict__ X,
                                                                 int64_t ld) {
    const FactorChunk ck = F.chunk[chunk0 + blockIdx.y];
    const FactorBlock bk = F.blk[ck.blk];
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= F.n) return;
    const T a = F.Z[i + int64_t(bk.i0) * F.ldz];
    const T b = F.Z[i + int64_t(bk.i1) * F.ldz];
    T* dst = X + i + int64_t(bk.col0 + ck.t0) * ld;
    for (int c = 0; c < ck.cnt; ++c) {
        const int g = ck.t0 + c + bk.shift;
        dst[int64_t(c) * ld] = factor_entry<T>(bk, a, b, g % bk.l0, g / bk.l0);
    }
}

// One workgroup: columns [t0, t0 + cnt) of one block over the rows [r0, r1).  FLAGS is the block's case.  In a row, at most
// two columns of a block with a discrete basis are non-zero; the row names them by their position in the chunk (h0, h1; a
// negative or large position hits nothing) with their entries (w0, w1), and column c adds `c == h0 ? w0 : c == h1 ? w1 : 0`
// times v: compares against the literal c, no per-column constants in registers.
//   A discrete, B absent / discrete:  the column of the row's level (pair of levels, k0 + l0 k1), entry 1
//   A discrete, B = [1, b]:           columns k0 (entry 1) and l0 + k0 (entry b)
//   A = [1, a], B discrete:           columns 2 k1 (entry 1) and 2 k1 + 1 (entry a)
// Blocks of continuous bases only ([a], or [a, b, a b]) are one short chunk and are written out.
template <class T, int FLAGS>
__device__ __forceinline__ void factor_sweep_body(const FactorView<T>& F, const FactorBlock& bk, const FactorChunk& ck,
                                                  const T* __restrict__ v, int64_t r0, int64_t r1, T (&acc)[CH]) {
    const T* __restrict__ z0 = F.Z + int64_t(bk.i0) * F.ldz;
    const T* __restrict__ z1 = F.Z + int64_t(bk.i1) * F.ldz;
    const int cnt = ck.cnt, t0 = ck.t0, l0 = bk.l0, l1 = bk.l1;
#pragma unroll 2
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kThreads) {
        const T vi = v[i];
        const T a = z0[i];
        const T b = (FLAGS & 4) ? T(1) : z1[i];
        if constexpr (FLAGS == 4) {
            acc[0] = fma(a, vi, acc[0]);
        } else if constexpr (FLAGS == 0) {
            acc[0] = fma(a, vi, acc[0]);
            acc[1] = fma(b, vi, acc[1]);
            acc[2] = fma(a * b, vi, acc[2]);
        } else {
            int h0, h1 = -1;
            T w1 = T(0);
            if constexpr (FLAGS == 5) {
                const int ia = factor_level(a, l0);
                h0 = ia < 0 ? -1 : ia - t0;
            } else if constexpr (FLAGS == 3) {
                const int ia = factor_level(a, l0), ib = factor_level(b, l1);
                h0 = (ia < 0 || ib < 0) ? -1 : ia + l0 * ib - t0;
            } else if constexpr (FLAGS == 1) {
                const int ia = factor_level(a, l0);
                h0 = ia < 0 ? -1 : ia - t0;
                h1 = ia < 0 ? -1 : ia + l0 - t0;
                w1 = b;
            } else { // FLAGS == 2
                const int ib = factor_level(b, l1);
                h0 = ib < 0 ? -1 : 2 * ib - t0;
                h1 = ib < 0 ? -1 : 2 * ib + 1 - t0;
                w1 = a;
            }
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (c < cnt) {
                    T x = (c == h0) ? T(1) : T(0);
                    if constexpr (FLAGS == 1 || FLAGS == 2) x = (c == h1) ? w1 : x;
                    acc[c] = fma(x, vi, acc[c]);
                }
        }
    }
}

template <class T>
__global__ __launch_bounds__(kThreads) void factor_sweep_kernel(FactorView<T> F, const T* __restrict__ v,
                                                                T* __restrict__ part, int64_t rows_per_split) {
    const FactorChunk ck = F.chunk[blockIdx.x];
    const FactorBlock bk = F.blk[ck.blk];
    const int split = blockIdx.y;
    const int64_t r0 = int64_t(split) * rows_per_split;
    const int64_t r1 = min(F.n, r0 + rows_per_split);
    T acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = T(0);
    switch (bk.flags) { // (uniform over the workgroup)
        case 0: factor_sweep_body<T, 0>(F, bk, ck, v, r0, r1, acc); break;
        case 1: factor_sweep_body<T, 1>(F, bk, ck, v, r0, r1, acc); break;
        case 2: factor_sweep_body<T, 2>(F, bk, ck, v, r0, r1, acc); break;
        case 3: factor_sweep_body<T, 3>(F, bk, ck, v, r0, r1, acc); break;
        case 4: factor_sweep_body<T, 4>(F, bk, ck, v, r0, r1, acc); break;
        default: factor_sweep_body<T, 5>(F, bk, ck, v, r0, r1, acc); break;
    }
    __shared__ T red[kThreads / 64][CH];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const T s = wave_sum64(acc[c]);
        if (lane == 0) red[wv][c] = s;
    }
    __syncthreads();
    if (tid < ck.cnt) {
        T s = T(0);
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) s += red[w][tid];
        part[int64_t(split) * F.p + bk.col0 + ck.t0 + tid] = s;
    }
}

template <class T>
__global__ void factor_reduce_kernel(const T* __restrict__ part, T* __restrict__ out, int64_t p, int nsplit,
                                     const T* __restrict__ sub_scale, const T* __restrict__ sub_vec) {
    const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= p) return;
    T s = T(0);
    for (int r = 0; r < nsplit; ++r) s += part[int64_t(r) * p + c];
    if (sub_vec) s -= sub_scale[0] * sub_vec[c];
    out[c] = s;
}

// Row slices: about 2048 workgroups in all (eight per compute unit) so that a design of few chunks still covers the chip, at
// least eight rows per thread and slice, at most 1024 slices (the partial sums are nsplit * p values).
inline void factor_shape(int64_t n, int64_t nchunk, int& nsplit, int64_t& rows_per_split) {
    const int64_t unit = kThreads;
    const int64_t max_split = std::max<int64_t>(1, (n + unit * 8 - 1) / (unit * 8));
    int64_t ns = (2048 + nchunk - 1) / std::max<int64_t>(nchunk, 1);
    ns = std::max<int64_t>(1, std::min<int64_t>(std::min(ns, max_split), 1024));
    rows_per_split = (n + ns - 1) / ns;
    rows_per_split = ((rows_per_split + unit - 1) / unit) * unit;
    ns = std::max<int64_t>(1, (n + rows_per_split - 1) / rows_per_split);
    nsplit = int(ns);
}

} // namespace

int64_t factor_sweep_work_elems(int64_t n, int64_t p, int64_t nchunk) {
    int ns;
    int64_t rps;
    factor_shape(n, nchunk, ns, rps);
    return int64_t(ns) * p + 16;
}

template <class T>
void launch_factor_expand(const FactorView<T>& F, T* X, int64_t ld, hipStream_t s) {
    if (F.n <= 0 || F.nchunk <= 0) return;
    const unsigned gx = unsigned((F.n + kThreads - 1) / kThreads);
    for (int64_t c0 = 0; c0 < F.nchunk; c0 += 65535) {
        const unsigned gy = unsigned(std::min<int64_t>(65535, F.nchunk - c0));
        hipLaunchKernelGGL((factor_expand_kernel<T>), dim3(gx, gy), dim3(kThreads), 0, s, F, c0, X, ld);
    }
}

template <class T>
void launch_sweep_factor(const FactorView<T>& F, const T* v, T* out, const T* sub_scale, const T* sub_vec, T* work,
                         hipStream_t s) {
    if (F.n <= 0 || F.p <= 0 || F.nchunk <= 0) return;
    int nsplit;
    int64_t rps;
    factor_shape(F.n, F.nchunk, nsplit, rps);
    hipLaunchKernelGGL((factor_sweep_kernel<T>), dim3(unsigned(F.nchunk), unsigned(nsplit)), dim3(kThreads), 0, s, F, v, work,
                       rps);
    const int bt = 256;
    hipLaunchKernelGGL((factor_reduce_kernel<T>), dim3(unsigned((F.p + bt - 1) / bt)), dim3(bt), 0, s, work, out, F.p, nsplit,
                       sub_scale, sub_vec);
}

#define INST(T)                                                                                    \
    template void launch_factor_expand<T>(const FactorView<T>&, T*, int64_t, hipStream_t);         \
    template void launch_sweep_factor<T>(const FactorView<T>&, const T*, T*, const T*, const T*, T*, hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
