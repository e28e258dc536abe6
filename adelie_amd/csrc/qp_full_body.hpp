// qp_full_body.hpp — the device side of adelie_hip_qp_full_solve (kernels_qp_full.hip): the three scalar updates of
// optimization/nnqp_full.hpp, lasso_full.hpp and pinball_full.hpp as rules, and the two kernels that run the reference's
// cyclic coordinate descent on  min 1/2 x'Qx - v'x + pen(x)  with Q a full (d, d) matrix.
//
// A visit of coordinate i (nnqp_full.hpp:76-92, lasso_full.hpp:82-100, pinball_full.hpp:92-113), operation for operation:
//     xn  = Rule::update(q_ii, g_i, x_i, pa_i, pb_i)
//     del = xn - x_i;   del == 0: nothing else happens
//     convg = max(convg, q_ii * del * del)
//     g_a = g_a - del * Q[a, i]   for every a, a multiply and then a subtract; Q[., i] is the i-th contiguous slice of the buffer
// Every operation is one correctly rounded IEEE operation of the value type (contraction is off in this file), in the
// reference's order, and nothing is summed across lanes: the result has the bits of the scalar loop run on a host.
//
// Two forms, one visit:
//   wave form (d <= 64)   one wavefront owns a problem.  Q is copied once into LDS (odd leading dimension); lane a carries x_a,
//                         g_a, q_aa and the two penalties in registers and the scalars of visit i are read out of lane i with a
//                         uniform index.  No barrier, reduction or atomic on the visit chain.
//   block form (d > 64)   one workgroup owns a problem, in the scheme of cd_fit_kernel (cd_fit_body.hpp): every thread evaluates the
//                         scalar update redundantly from broadcast reads, g and x are double-buffered, a changed visit ends
//                         with its one barrier and an unchanged visit has none.  The column of Q comes from global memory.  The
//                         per-coordinate state lives in dynamic LDS or, under the LDS = false instantiation, in global scratch.
// A launch covers a list of problems (one workgroup each) described by a table in device memory.
#pragma once
#include "common.hpp"
#include "wavered.hpp"

#pragma clang fp contract(off)

namespace ahip {
namespace {

constexpr int kQpWave = 64;           // lanes = largest d of the wave form
constexpr int kQpBlockThreads = 1024; // largest workgroup of the block form

// one problem of a batch, as the kernels read it
struct QpFullProb {
    const void* Q;     // (d, d) contiguous, device
    const void* pa;    // (d,) penalty (lasso) / penalty_neg (pinball); unused by nnqp
    const void* pb;    // (d,) penalty_pos (pinball)
    void* x;           // (d,) in / out
    void* g;           // (d,) in / out
    char* scratch;     // block form, global state: qp_block_state_bytes(d) bytes
    int64_t* report;   // out: {iters, status}
    double thr;        // the sweep's threshold, already rounded to the value type
    int64_t max_iters;
    int32_t d;
    int32_t pad;
};

// bytes of the block form's per-coordinate state: g x 2, x x 2, the diagonal, the two penalties
template <class T>
constexpr size_t qp_block_state_bytes(int64_t d) {
    return size_t(d) * 7 * sizeof(T);
}

// nnqp_full.hpp:77-82
template <class T>
struct NnqpFullRule {
    static __device__ __forceinline__ T update(T qii, T gi, T xi, T, T) {
#pragma clang fp contract(off)
        const T step = (qii <= T(0)) ? T(0) : (gi / qii);
        const T cand = xi + step;
        return (cand < T(0)) ? T(0) : cand; // std::max(cand, 0)
    }
};

__device__ __forceinline__ float qp_copysign(float m, float s) { return __builtin_copysignf(m, s); }
__device__ __forceinline__ double qp_copysign(double m, double s) { return __builtin_copysign(m, s); }

// lasso_full.hpp:83-90
template <class T>
struct LassoFullRule {
    static __device__ __forceinline__ T update(T qii, T gi, T xi, T pi, T) {
#pragma clang fp contract(off)
        const T gi0 = gi + qii * xi;
        const T gi0_abs = qp_copysign(gi0, T(1)); // std::abs(gi0)
        return (gi0_abs <= pi) ? T(0) : qp_copysign((gi0_abs - pi) / qii, gi0);
    }
};

// pinball_full.hpp:93-103; pni = penalty_neg, ppi = penalty_pos
template <class T>
struct PinballFullRule {
    static __device__ __forceinline__ T update(T qii, T gi, T xi, T pni, T ppi) {
#pragma clang fp contract(off)
        const T gi0 = gi + qii * xi;
        const T lo = -pni - gi0, hi = gi0 - ppi;
        const T m = (lo < hi) ? hi : lo;     // std::max(lo, hi)
        const T mag = (m < T(0)) ? T(0) : m; // std::max(m, 0)
        return qp_copysign(mag, gi0 + pni) / qii;
    }
};

// ---- wave form ------------------------------------------------------------------------------------------------------------
template <class T, class Rule>
__global__ __launch_bounds__(kQpWave) void qp_full_wave_kernel(const QpFullProb* __restrict__ tab, const int32_t* __restrict__ list) {
    __shared__ T Qs[kQpWave * (kQpWave + 1)];
    const QpFullProb P = tab[list[blockIdx.x]];
    const int lane = threadIdx.x, d = P.d, LD = d | 1;
    const T* Q = static_cast<const T*>(P.Q);
    for (int idx = lane; idx < d * d; idx += kQpWave) {
        const int c = idx / d, r = idx - c * d;
        Qs[c * LD + r] = Q[idx];
    }
    const bool in = lane < d;
    T x = in ? static_cast<const T*>(P.x)[lane] : T(0);
    T g = in ? static_cast<const T*>(P.g)[lane] : T(0);
    const T qd = in ? Q[int64_t(lane) * d + lane] : T(0);
    const T pa = (in && P.pa) ? static_cast<const T*>(P.pa)[lane] : T(0);
    const T pb = (in && P.pb) ? static_cast<const T*>(P.pb)[lane] : T(0);
    __syncthreads();

    const T thr = T(P.thr);
    const int64_t max_iters = P.max_iters;
    int64_t iters = 0;
    int status = ADELIE_HIP_QP_FULL_MAX_ITERS;
    while (iters < max_iters) {
        T convg = T(0);
        ++iters;
        for (int i = 0; i < d; ++i) {
            const T qii = prdl(qd, i), gi = prdl(g, i), xi = prdl(x, i);
            const T xn = Rule::update(qii, gi, xi, prdl(pa, i), prdl(pb, i));
            const T del = xn - xi;
            if (del == T(0)) continue;
            const T sds = qii * del * del;
            convg = (convg < sds) ? sds : convg;
            if (lane == i) x = xn;
            if (in) g = g - del * Qs[i * LD + lane];
        }
        if (convg < thr) {
            status = ADELIE_HIP_QP_FULL_OK;
            break;
        }
    }
    if (in) {
        static_cast<T*>(P.x)[lane] = x;
        static_cast<T*>(P.g)[lane] = g;
    }
    if (lane == 0) {
        P.report[0] = iters;
        P.report[1] = status;
    }
}

// ---- block form -----------------------------------------------------------------------------------------------------------
template <class T, bool LDS, class Rule>
__global__ __launch_bounds__(kQpBlockThreads) void qp_full_block_kernel(const QpFullProb* __restrict__ tab,
                                                                        const int32_t* __restrict__ list) {
    extern __shared__ __attribute__((aligned(16))) char qp_full_sm[];
    const QpFullProb P = tab[list[blockIdx.x]];
    const int tid = threadIdx.x, bd = blockDim.x, d = P.d;
    // no __restrict__ on the state: the same arrays are read and written across barriers
    char* base = LDS ? qp_full_sm : P.scratch;
    T* g0 = reinterpret_cast<T*>(base);
    T* g1 = g0 + d;
    T* x0 = g1 + d;
    T* x1 = x0 + d;
    T* qd = x1 + d;
    T* pa = qd + d;
    T* pb = pa + d;
    const T* Q = static_cast<const T*>(P.Q);
    for (int a = tid; a < d; a += bd) {
        g0[a] = static_cast<const T*>(P.g)[a];
        x0[a] = static_cast<const T*>(P.x)[a];
        qd[a] = Q[int64_t(a) * d + a];
        pa[a] = P.pa ? static_cast<const T*>(P.pa)[a] : T(0);
        pb[a] = P.pb ? static_cast<const T*>(P.pb)[a] : T(0);
    }
    __syncthreads();

    const T thr = T(P.thr);
    const int64_t max_iters = P.max_iters;
    int64_t iters = 0;
    int cur = 0, status = ADELIE_HIP_QP_FULL_MAX_ITERS;
    while (iters < max_iters) {
        T convg = T(0);
        ++iters;
        for (int i = 0; i < d; ++i) {
            const T* gc = cur ? g1 : g0;
            const T* xc = cur ? x1 : x0;
            const T qii = qd[i], gi = gc[i], xi = xc[i];
            const T xn = Rule::update(qii, gi, xi, pa[i], pb[i]);
            const T del = xn - xi;
            if (del == T(0)) continue;
            const T sds = qii * del * del;
            convg = (convg < sds) ? sds : convg;
            T* gn = cur ? g0 : g1;
            T* xw = cur ? x0 : x1;
            const T* Qi = Q + int64_t(i) * d;
            for (int a = tid; a < d; a += bd) {
                gn[a] = gc[a] - del * Qi[a];
                xw[a] = a == i ? xn : xc[a];
            }
            cur ^= 1;
            __syncthreads();
        }
        if (convg < thr) {
            status = ADELIE_HIP_QP_FULL_OK;
            break;
        }
    }
    const T* gc = cur ? g1 : g0;
    const T* xc = cur ? x1 : x0;
    for (int a = tid; a < d; a += bd) {
        static_cast<T*>(P.x)[a] = xc[a];
        static_cast<T*>(P.g)[a] = gc[a];
    }
    if (tid == 0) {
        P.report[0] = iters;
        P.report[1] = status;
    }
}

} // namespace
} // namespace ahip
