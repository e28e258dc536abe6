// kernels_relu.hip — gated / signed convex-ReLU designs built from a base matrix Z and a boolean mask (gfx950 / CDNA4).
//
//   relu_expand   X = the expanded (n, P) design [D_1 Z, ..., D_m Z] (and its negation for the signed form), written once from
//                 the resident Z and mask: replaces the lazy column generation of MatrixNaiveConvexGatedReluDense /
//                 MatrixNaiveConvexReluDense (reference matrix_naive_convex_gated_relu.ipp, matrix_naive_convex_relu.ipp:10-30)
//                 -- every other kernel of this library then streams X as a dense design.
//   sweep_relu    out[j_m d + j_d] = sum_i Z[i, j_d] mask[i, j_m] v[i] for ALL columns without reading X: this is the (d, m)
//                 matrix product Z^T (mask o v) reduced over the rows, n d values of Z and n m bytes of mask instead of the
//                 n m d values of X.  It runs on the matrix cores (16x16x4, f64 / f32): the A operand is a 16-column tile of
//                 Z, the B operand a 16-column tile of `mask ? v : 0` formed in registers.  The signed half is the negated copy.
//
// The instruction's k index is a row of the design, and any assignment of rows to k serves as long as A and B agree.  Lane
// (c = lane & 15, q = lane >> 4) loads the run of kReluRun consecutive rows [k + q R, k + (q + 1) R) of ITS column -- 16-byte
// loads of Z, one 8-byte load per mask tile, the run of v -- and the e-th instruction of a step multiplies the e-th row of the
// four runs.  A wave keeps one tile of Z against kReluMT mask tiles in accumulators, so Z is read once per row slice and
// group of 64 mask columns.  No LDS, no barrier: a wave owns a row slice by itself.  Columns beyond d / m and rows beyond n
// count as zeros (the last tile of either, the last step of the last slice).
//
// The sweep is order-deterministic: a wave adds its rows in a fixed order, the slices leave partial sums in `work` that a
// second kernel adds in a fixed order (runs of slices in slice order, then the runs in order).  No floating-point atomics.
#include "gram_common.hpp"
#include <algorithm>

namespace ahip {

namespace {

constexpr int kThreads = 256;
constexpr int R = kReluRun, MT = kReluMT, TL = kReluTile;

// One thread: row i of the mask columns blockIdx.y, blockIdx.y + gridDim.y, ...: the d entries of each, rows along lanes
// (coalesced stores).  A select, not a product with 0 / 1: a masked-out row holds a zero whatever Z holds there.
template <class T>
__global__ __launch_bounds__(kThreads) void relu_expand_kernel(ReluView<T> F, T* __restrict__ X, int64_t ld) {
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= F.n) return;
    const int64_t md = F.m * F.d;
    for (int64_t jm = blockIdx.y; jm < F.m; jm += gridDim.y) {
        const bool on = F.mask[i + jm * F.ldm] != 0;
        T* dst = X + i + jm * F.d * ld;
        for (int64_t jd = 0; jd < F.d; ++jd) {
            const T z = F.Z[i + jd * F.ldz];
            dst[jd * ld] = on ? z : T(0);
            if (!F.gated) dst[(md + jd) * ld] = on ? -z : T(0);
        }
    }
}

// what a lane holds of one step: its run of Z, of v, and of each mask tile (a byte per row)
template <class T, int NMT>
struct ReluStage {
    T z[R], v[R];
    uint64_t mk[NMT];
};

// The runs [k, k + R) of the lane's column zc of Z, of v and of its column mc[t] of every mask tile.  FULL: all of them lie
// below n (16-byte loads of Z, 8-byte loads of the mask, no bounds); otherwise rows >= n read as zero.
template <class T, int NMT, bool VOK, bool FULL>
__device__ __forceinline__ void relu_fetch(const ReluView<T>& F, const T* __restrict__ v, const T* __restrict__ zc,
                                           const uint8_t* const (&mc)[NMT], int64_t k, ReluStage<T, NMT>& st) {
    constexpr int V = VecOf<T>::N;
    using VT = typename VecOf<T>::type;
    if constexpr (FULL) {
#pragma unroll
        for (int u = 0; u < R / V; ++u) { // (ldz is a multiple of V and k of R: aligned)
            const VT x = *reinterpret_cast<const VT*>(zc + k + u * V);
#pragma unroll
            for (int e = 0; e < V; ++e) st.z[u * V + e] = x[e];
        }
        if constexpr (VOK) {
#pragma unroll
            for (int u = 0; u < R / V; ++u) {
                const VT x = *reinterpret_cast<const VT*>(v + k + u * V);
#pragma unroll
                for (int e = 0; e < V; ++e) st.v[u * V + e] = x[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < R; ++e) st.v[e] = v[k + e];
        }
#pragma unroll
        for (int t = 0; t < NMT; ++t) st.mk[t] = *reinterpret_cast<const uint64_t*>(mc[t] + k); // (ldm, k: multiples of 8)
    } else {
#pragma unroll
        for (int e = 0; e < R; ++e) {
            const bool in = k + e < F.n;
            st.z[e] = in ? zc[k + e] : T(0);
            st.v[e] = in ? v[k + e] : T(0);
        }
#pragma unroll
        for (int t = 0; t < NMT; ++t) {
            uint64_t b = 0;
#pragma unroll
            for (int e = 0; e < R; ++e)
                if (k + e < F.n) b |= uint64_t(mc[t][k + e] != 0) << (8 * e);
            st.mk[t] = b;
        }
    }
}

template <class T, int NMT>
__device__ __forceinline__ void relu_step(const ReluStage<T, NMT>& st, typename Mfma<T>::acc_t (&acc)[NMT]) {
#pragma unroll
    for (int e = 0; e < R; ++e) {
#pragma unroll
        for (int t = 0; t < NMT; ++t) {
            const T b = ((st.mk[t] >> (8 * e)) & 0xffu) ? st.v[e] : T(0);
            acc[t] = Mfma<T>::run(st.z[e], b, acc[t]);
        }
    }
}

// One wave: the tile dt of Z against the NMT mask tiles from column jm0 on, over the rows [r0, r1).  A lane whose column of Z
// or of the mask lies beyond d / m reads column 0 instead: row i of the product depends on row i of A alone and column j on
// column j of B alone, and those rows and columns are never stored.
template <class T, int NMT, bool VOK>
__device__ __forceinline__ void relu_sweep_body(const ReluView<T>& F, const T* __restrict__ v, T* __restrict__ dst, int64_t dt,
                                                int64_t jm0, int64_t r0, int64_t r1, int lane) {
    const int fr = lane & 15, fk = lane >> 4;
    const int64_t jd = dt * TL + fr;
    const T* __restrict__ zc = F.Z + (jd < F.d ? jd : 0) * F.ldz;
    const uint8_t* mc[NMT];
#pragma unroll
    for (int t = 0; t < NMT; ++t) {
        const int64_t jm = jm0 + t * TL + fr;
        mc[t] = F.mask + (jm < F.m ? jm : 0) * F.ldm;
    }
    typename Mfma<T>::acc_t acc[NMT];
#pragma unroll
    for (int t = 0; t < NMT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = T(0);

    ReluStage<T, NMT> st;
    const int64_t off = int64_t(fk) * R;
    const int64_t rfull = r0 + ((r1 - r0) / kReluStep) * kReluStep; // (uniform over the wave)
    int64_t k = r0;
    for (; k < rfull; k += kReluStep) {
        relu_fetch<T, NMT, VOK, true>(F, v, zc, mc, k + off, st);
        relu_step<T, NMT>(st, acc);
    }
    if (k < r1) { // the last slice's last step: rows beyond n count as zero
        relu_fetch<T, NMT, VOK, false>(F, v, zc, mc, k + off, st);
        relu_step<T, NMT>(st, acc);
    }
    // acc[t][e] = the sum for column Mfma::row(lane, e) of the Z tile and column lane & 15 of mask tile t
#pragma unroll
    for (int t = 0; t < NMT; ++t) {
        const int64_t jm = jm0 + t * TL + fr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t jz = dt * TL + Mfma<T>::row(lane, e);
            if (jm < F.m && jz < F.d) dst[jm * F.d + jz] = acc[t][e];
        }
    }
}

// grid: x = (tile of 16 columns of Z) + d_tiles * (group of MT tiles of 16 mask columns), y = kReluWaves row slices (one per
// wave).  Latency is hidden by the waves of a SIMD taking turns, not by prefetching: two workgroups per SIMD at the least.
template <class T, bool VOK>
__global__ __launch_bounds__(kThreads, 2) void relu_sweep_kernel(ReluView<T> F, const T* __restrict__ v, T* __restrict__ part,
                                                                 int64_t d_tiles, int64_t nslice, int64_t rows_per_slice) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t slice = int64_t(blockIdx.y) * kReluWaves + wv;
    if (slice >= nslice) return;
    const int64_t dt = int64_t(blockIdx.x) % d_tiles, mg = int64_t(blockIdx.x) / d_tiles;
    const int64_t jm0 = mg * (TL * MT);
    const int nmt = int(std::min<int64_t>(MT, (F.m - jm0 + TL - 1) / TL));
    const int64_t r0 = slice * rows_per_slice;
    const int64_t r1 = std::min<int64_t>(F.n, r0 + rows_per_slice);
    T* dst = part + slice * (F.m * F.d);
    static_assert(MT == 4, "one case per count of mask tiles");
    switch (nmt) { // (uniform over the workgroup)
        case 1: relu_sweep_body<T, 1, VOK>(F, v, dst, dt, jm0, r0, r1, lane); break;
        case 2: relu_sweep_body<T, 2, VOK>(F, v, dst, dt, jm0, r0, r1, lane); break;
        case 3: relu_sweep_body<T, 3, VOK>(F, v, dst, dt, jm0, r0, r1, lane); break;
        default: relu_sweep_body<T, 4, VOK>(F, v, dst, dt, jm0, r0, r1, lane); break;
    }
}

// Adds the slices' partial sums in a fixed order, applies the epilogue of the dense sweep per column and writes the negated
// sum into the signed half.  A workgroup owns kRedCols columns; thread (column, q) adds the q-th of kRedParts contiguous runs
// of slices in slice order, and the runs' sums are added in run order: with hundreds of slices and a few thousand columns, one
// thread per column would walk its slices alone on a handful of compute units.
constexpr int kRedCols = 16, kRedParts = 16;
template <class T>
__global__ __launch_bounds__(kRedCols * kRedParts) void relu_reduce_kernel(const T* __restrict__ part, T* __restrict__ out,
                                                                           int64_t md, int64_t nslice, int gated,
                                                                           const T* __restrict__ sub_scale,
                                                                           const T* __restrict__ sub_vec) {
    __shared__ T red[kRedParts][kRedCols];
    const int cl = threadIdx.x % kRedCols, q = threadIdx.x / kRedCols;
    const int64_t c = int64_t(blockIdx.x) * kRedCols + cl;
    const int64_t per = (nslice + kRedParts - 1) / kRedParts;
    const int64_t s0 = q * per, s1 = std::min<int64_t>(nslice, s0 + per);
    T s = T(0);
    if (c < md) {
#pragma unroll 4
        for (int64_t r = s0; r < s1; ++r) s += part[r * md + c];
    }
    red[q][cl] = s;
    __syncthreads();
    if (q != 0 || c >= md) return;
    s = red[0][cl];
#pragma unroll
    for (int u = 1; u < kRedParts; ++u) s += red[u][cl];
    T pos = s, neg = -s;
    if (sub_vec) {
        pos -= sub_scale[0] * sub_vec[c];
        if (!gated) neg -= sub_scale[0] * sub_vec[md + c];
    }
    out[c] = pos;
    if (!gated) out[md + c] = neg;
}

} // namespace

template <class T>
void launch_relu_expand(const ReluView<T>& F, T* X, int64_t ld, hipStream_t s) {
    if (F.n <= 0 || F.d <= 0 || F.m <= 0) return;
    const unsigned gx = unsigned((F.n + kThreads - 1) / kThreads);
    const unsigned gy = unsigned(std::min<int64_t>(65535, F.m));
    hipLaunchKernelGGL((relu_expand_kernel<T>), dim3(gx, gy), dim3(kThreads), 0, s, F, X, ld);
}

template <class T>
void launch_sweep_relu(const ReluView<T>& F, const T* v, T* out, const T* sub_scale, const T* sub_vec, T* work, hipStream_t s) {
    if (F.d <= 0 || F.m <= 0) return;
    const ReluShape sh = relu_shape(F.n, F.d, F.m);
    const int64_t md = F.m * F.d;
    // (n == 0: one slice without rows leaves zeros).  d_tiles * m_groups < 2^31 as m * d is; at most 1024 slices.
    const dim3 grid(unsigned(sh.d_tiles * sh.m_groups), unsigned((sh.nslice + kReluWaves - 1) / kReluWaves));
    const bool vok = reinterpret_cast<uintptr_t>(v) % 16 == 0;
    if (vok) hipLaunchKernelGGL((relu_sweep_kernel<T, true>), grid, dim3(kThreads), 0, s, F, v, work, sh.d_tiles, sh.nslice, sh.rows_per_slice);
    else hipLaunchKernelGGL((relu_sweep_kernel<T, false>), grid, dim3(kThreads), 0, s, F, v, work, sh.d_tiles, sh.nslice, sh.rows_per_slice);
    hipLaunchKernelGGL((relu_reduce_kernel<T>), dim3(unsigned((md + kRedCols - 1) / kRedCols)), dim3(kRedCols * kRedParts), 0, s,
                       work, out, md, sh.nslice, F.gated, sub_scale, sub_vec);
}

#define INST(T)                                                                                  \
    template void launch_relu_expand<T>(const ReluView<T>&, T*, int64_t, hipStream_t);           \
    template void launch_sweep_relu<T>(const ReluView<T>&, const T*, T*, const T*, const T*, T*, hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
