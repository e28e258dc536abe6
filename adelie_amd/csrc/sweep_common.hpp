// sweep_common.hpp — device and launch pieces shared by the streaming kernel files (kernels_sweep.hip, kernels_filter.hip,
// kernels_convert.hip): the workgroup size, the wave reduction, the vector load, and the one epilogue every panel sweep ends in.
// The filter's exact columns carry "the bits the full sweep gives" because both go through the functions below.
#pragma once
#include "kernels.hpp"
#include "accessors.hpp"
#include "sweep_shape.hpp"

namespace ahip {

// out[c] = sum of the nsplit row-split partials part[r * ncols + c], in split order, minus the centring term (kernels_sweep.hip)
template <class T>
void launch_sweep_reduce(const T* part, T* out, int64_t ncols, int nsplit, int64_t c0, const int32_t* cols, const T* sub_scale,
                         const T* sub_vec, hipStream_t s);

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kSweepThreads, "sweep_shape.hpp counts rows per iteration of a kThreads workgroup");

// (the __shfl_down ladder: its order of additions is part of every sweep's bits)
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

template <class T, int VEC>
__device__ __forceinline__ Pack<T, VEC> load_vec(const T* p) {
    Pack<T, VEC> r;
    if constexpr (VEC == 1) r.v[0] = p[0];
    else {
        using V = typename VecOf<T>::type;
        V x = *reinterpret_cast<const V*>(p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) r.v[e] = x[e];
    }
    return r;
}

template <class T>
inline bool dense_vec_ok(const DenseView<T>& X) {
    constexpr int V = VecOf<T>::N;
    return (X.ld % V == 0) && ((reinterpret_cast<uintptr_t>(X.X) % 16) == 0);
}

inline unsigned grid1d(int64_t n, int bt, int64_t cap = 4096) {
    int64_t g = (n + bt - 1) / bt;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return unsigned(g);
}

// s minus the centring term of column j (sub_vec == nullptr: no such term)
template <class T>
__device__ __forceinline__ T centred(T s, int64_t j, const T* sub_scale, const T* sub_vec) {
    if (sub_vec) s -= sub_scale[0] * sub_vec[j];
    return s;
}

// Where the finished sum of output c (column j of the design) goes: with one row split the centred value to out[c], else
// row split `split`'s partial to out[split * stride + c] for a reduce launch to add up
template <class T>
__device__ __forceinline__ void store_sum(T s, T* out, int64_t c, int64_t j, int split, int nsplit, int64_t stride,
                                          const T* sub_scale, const T* sub_vec) {
    if (nsplit == 1) out[c] = centred(s, j, sub_scale, sub_vec);
    else out[int64_t(split) * stride + c] = s; // partial
}

// The end of a panel kernel (CB columns per workgroup, panel cb of ncols outputs): the wave sums of every column through LDS,
// the waves added in order by thread k for column k, SCALED: the sum times scale[c] (one rounding), then store_sum; the
// duplicated columns of a tail panel are dropped here.  Output c is column cols ? cols[c] : c0 + c of the design.
template <bool SCALED, class T, int CB>
__device__ __forceinline__ void panel_epilogue(const T (&acc)[CB], T (&red)[kThreads / 64][CB], int64_t cb, int64_t ncols,
                                               int64_t c0, const int32_t* cols, const double* scale, T* out, int split,
                                               int nsplit, const T* sub_scale, const T* sub_vec) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < CB; ++k) {
        const T s = wave_sum(acc[k]);
        if (lane == 0) red[wv][k] = s;
    }
    __syncthreads();
    if (tid < CB) {
        const int64_t c = cb * CB + tid;
        if (c < ncols) {
            T s = T(0);
#pragma unroll
            for (int w = 0; w < kThreads / 64; ++w) s += red[w][tid];
            if constexpr (SCALED) s = __dmul_rn(s, scale[c]);
            store_sum(s, out, c, cols ? int64_t(cols[c]) : c0 + c, split, nsplit, ncols, sub_scale, sub_vec);
        }
    }
}

} // namespace
} // namespace ahip
