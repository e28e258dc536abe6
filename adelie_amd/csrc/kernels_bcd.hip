// kernels_bcd.hip — the group elastic net update, a batch per call (adelie.bcd.solve with solver "newton" / "newton_abs":
// bcd/unconstrained/newton.hpp, bcd/utils.hpp, optimization/newton.hpp).  The C-ABI entry point adelie_hip_bcd_solve, its host
// driver and the kernels.
//
// One solve is a short chain of d-term sums: two per Newton step, one per bisection probe.  That is latency, not bytes, so a
// problem's q + l2, v and the current 1 / ((q + l2) h + l1) stay where they are cheapest to reach for the whole solve, and a
// wavefront is filled with as many problems as fit:
//   team       d <= 64            a team of W = 4, 8, 16, 32 or 64 lanes (the smallest >= d) owns a problem, 64 / W problems share
//                                 a wavefront; one value per lane in registers; lanes past d hold q + l2 = 1, v = 0 and add
//                                 exact zeros.  The wavefront loops until all its teams are done; a finished team's state is
//                                 frozen by predicate.
//   wave       64 < d <= 1024     a wavefront per problem, NT = 2, 4, 8 or 16 values per lane in registers (value lane + 64 k in
//                                 slot k), lane-local partial sums in the order of k.
//   workgroup  d > 1024           256 threads per problem; q + l2 and v staged once in LDS while both fit, read from global
//                                 memory in every pass beyond that; thread-local partial sums over i = tid, tid + 256, ..., the
//                                 four waves' sums combined through LDS in wave order.
// Every sum ends in the same xor butterfly over the team's (wave's) lanes, after which all of them hold the same bits, so the
// scalar part of the iteration is computed redundantly and nothing is broadcast.  The order of a problem's sums depends on its
// own d only: its beta and iters have the same bits in whatever batch, position and neighbourhood it is solved.
//
// The host buckets the problems by class (five team widths, four wave tile counts, the workgroup tier staged or not), builds one
// index array with the classes' launch lists back to back, and issues one launch per non-empty class on one stream.
#include "common.hpp"
#include "wavered.hpp"

#pragma clang fp contract(off)

namespace ahip {
namespace {

constexpr int kBcdBlock = 256;
constexpr int kBcdWaveMaxD = 1024;
// the workgroup tier stages q + l2 and v in LDS while 2 d values and the reduction slots fit in gfx950's 160 KB
constexpr size_t kBcdLdsBytes = size_t(160) << 10, kBcdLdsReserve = 1024;
template <class T> constexpr int64_t bcd_lds_max_d() { return int64_t((kBcdLdsBytes - kBcdLdsReserve) / (2 * sizeof(T))); }

// what every kernel of a call reads
template <class T>
struct BcdParams {
    const int64_t* off;  // (B + 1)
    const T *quad, *lin; // flat
    const T *l1, *l2;    // (B)
    T* beta;             // flat
    int64_t* iters;      // (B)
    int32_t* status;     // (B)
    T tol;
    int64_t max_iters;
    int solver;
};

// ---- the butterflies: after one, every lane of the W-lane team holds the same bits ----------------------------------------------
// xor 1 and xor 2 by quad_perm; the two mirrors stand for xor 4 and xor 8 (their source lanes lie in the other half, whose lanes
// already agree); xor 16 and xor 32 cross rows.
struct OpAdd { template <class T> static __device__ __forceinline__ T f(T a, T b) { return a + b; } };
struct OpMin { template <class T> static __device__ __forceinline__ T f(T a, T b) { return b < a ? b : a; } };
template <int W, class Op, class T>
__device__ __forceinline__ T bfly(T x) {
    if (W >= 2) x = Op::f(x, pdpp<0xB1>(x));
    if (W >= 4) x = Op::f(x, pdpp<0x4E>(x));
    if (W >= 8) x = Op::f(x, pdpp<0x141>(x));
    if (W >= 16) x = Op::f(x, pdpp<0x140>(x));
    if (W >= 32) x = Op::f(x, __shfl_xor(x, 16, 64));
    if (W >= 64) x = Op::f(x, __shfl_xor(x, 32, 64));
    return x;
}

// ---- where a problem's values live: the three tiers ------------------------------------------------------------------------------
// Each offers  sum2(f, s0, s1): f(a, v, r, ok, t0, t1) names two terms per value, summed over the group;  vmin(f);
// each(f): f(a, v, r, i) once per real value with its index in the problem.  a = q + l2, r = the held 1 / (a h + l1), ok = a real
// value (not padding).  kHoldsR: r survives between calls.

// W lanes own the problem, lane j value j
template <class T, int W>
struct TeamGroup {
    static constexpr bool kHoldsR = true;
    T a, v, r;
    bool ok;
    int j;
    template <class F> __device__ __forceinline__ void sum2(F f, T& s0, T& s1) {
        T t0, t1;
        f(a, v, r, ok, t0, t1);
        s0 = bfly<W, OpAdd>(t0), s1 = bfly<W, OpAdd>(t1);
    }
    template <class F> __device__ __forceinline__ T vmin(F f) { return bfly<W, OpMin>(f(a, v, ok)); }
    template <class F> __device__ __forceinline__ void each(F f) {
        if (ok) f(a, v, r, int64_t(j));
    }
};

// a wavefront owns the problem, lane l values l + 64 k
template <class T, int NT>
struct WaveGroup {
    static constexpr bool kHoldsR = true;
    T a[NT], v[NT], r[NT];
    int lane, d;
    template <class F> __device__ __forceinline__ void sum2(F f, T& s0, T& s1) {
        T p0 = T(0), p1 = T(0);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            T t0, t1;
            f(a[k], v[k], r[k], lane + 64 * k < d, t0, t1);
            p0 += t0, p1 += t1;
        }
        s0 = bfly<64, OpAdd>(p0), s1 = bfly<64, OpAdd>(p1);
    }
    template <class F> __device__ __forceinline__ T vmin(F f) {
        T m = f(a[0], v[0], lane < d);
#pragma unroll
        for (int k = 1; k < NT; ++k) m = OpMin::f(m, f(a[k], v[k], lane + 64 * k < d));
        return bfly<64, OpMin>(m);
    }
    template <class F> __device__ __forceinline__ void each(F f) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
            if (lane + 64 * k < d) f(a[k], v[k], r[k], int64_t(lane + 64 * k));
    }
};

// a workgroup of 256 owns the problem; LDS: a and v staged in sa / sv, else read from q (+ l2) / lin in every pass
template <class T, bool LDS>
struct BlockGroup {
    static constexpr bool kHoldsR = false;
    const T *sa, *sv; // LDS copies (LDS) or the problem's quad / linear in global memory
    T l2;
    T* red;           // 2 x 4 slots in LDS
    int64_t d;
    int tid;
    __device__ __forceinline__ T get_a(int64_t i) const { return LDS ? sa[i] : sa[i] + l2; }
    template <class Op> __device__ __forceinline__ void combine(T& p0, T& p1) {
        p0 = bfly<64, Op>(p0), p1 = bfly<64, Op>(p1);
        __syncthreads(); // the slots' last readers are done
        if ((tid & 63) == 0) red[tid >> 6] = p0, red[4 + (tid >> 6)] = p1;
        __syncthreads();
        p0 = Op::f(Op::f(Op::f(red[0], red[1]), red[2]), red[3]);
        p1 = Op::f(Op::f(Op::f(red[4], red[5]), red[6]), red[7]);
    }
    template <class F> __device__ __forceinline__ void sum2(F f, T& s0, T& s1) {
        T p0 = T(0), p1 = T(0), r = T(0);
        for (int64_t i = tid; i < d; i += kBcdBlock) {
            T t0, t1;
            f(get_a(i), sv[i], r, true, t0, t1);
            p0 += t0, p1 += t1;
        }
        combine<OpAdd>(p0, p1);
        s0 = p0, s1 = p1;
    }
    template <class F> __device__ __forceinline__ T vmin(F f) {
        T m = T(1) / T(0), m1 = m;
        for (int64_t i = tid; i < d; i += kBcdBlock) m = OpMin::f(m, f(get_a(i), sv[i], true));
        combine<OpMin>(m, m1);
        return m;
    }
    template <class F> __device__ __forceinline__ void each(F f) {
        for (int64_t i = tid; i < d; i += kBcdBlock) f(get_a(i), sv[i], T(0), i);
    }
};

// std::max<T>(x, c) as the reference writes it: a NaN x stays a NaN (and then ends the iteration it is in)
template <class T> __device__ __forceinline__ T ref_max(T x, T c) { return x < c ? c : x; }

// ---- one solve, the same text for every tier ---------------------------------------------------------------------------------------
// Every lane of the group runs this with the same scalars (the butterflies leave them equal), and several groups may share the
// wavefront: loops run while any group of the wavefront is in them, and a group outside a loop keeps its state by predicate.
// `live`: the group has a problem (the last wavefront of a team launch may have spare teams).  x points at the problem's beta.
template <class T, class G>
__device__ __forceinline__ void bcd_solve_group(G& g, const BcdParams<T>& P, T l1, int64_t d, bool live, T* __restrict__ x,
                                                int64_t& iters_out, int32_t& status_out) {
    const T INF = T(1) / T(0);
    const T tol = P.tol;
    T s0, s1;
    // newton.hpp:61-75: the two easy cases
    g.sum2([](T, T v, T&, bool, T& t0, T& t1) { t0 = v * v, t1 = T(0); }, s0, s1);
    const T v_l2 = sqrt(s0);
    const bool zero = v_l2 <= l1;
    const bool closed = !zero && l1 <= T(0);
    const bool hard = live && !zero && !closed;

    T h = T(0);
    if (P.solver == ADELIE_HIP_BCD_NEWTON_ABS) { // newton.hpp:229-266
        // root_lower_bound (utils.hpp:29-40); padding must not count in the sums of a
        T sa, saa;
        g.sum2([](T a, T, T&, bool ok, T& t0, T& t1) { t0 = ok ? a : T(0), t1 = ok ? a * a : T(0); }, sa, saa);
        T v_l1, hm2;
        g.sum2([](T a, T v, T&, bool, T& t0, T& t1) {
            t0 = fabs(v);
            const T z = v / a;
            t1 = z * z;
        }, v_l1, hm2);
        const T b = l1 * sa;
        const T c = l1 * l1 * T(d) - v_l1 * v_l1;
        const T discr = b * b - saa * c;
        T h_min = (double(discr) > -1e-12) ? (-b + sqrt(ref_max(discr, T(0)))) / saa : T(0);
        h_min = ref_max(h_min, T(0));
        // root_upper_bound (utils.hpp:70-95), zero_tol = 1e-14
        const T zero_tol = T(1e-14);
        const T a_min = g.vmin([INF](T a, T, bool ok) { return ok ? a : INF; });
        T h_max = sqrt(hm2), min_nnz = a_min;
        const bool small = a_min <= zero_tol;
        if (__any(hard && small)) { // utils.hpp:81-89
            T hs, v_S;
            g.sum2([zero_tol](T a, T v, T&, bool ok, T& t0, T& t1) {
                const T vi2 = v * v;
                t0 = (ok && a > zero_tol) ? vi2 / (a * a) : T(0);
                t1 = (ok && a <= T(0)) ? vi2 : T(0);
            }, hs, v_S);
            const T mn = g.vmin([INF, zero_tol](T a, T, bool ok) { return (ok && a > zero_tol) ? a : INF; });
            if (small) {
                min_nnz = mn;
                h_max = sqrt(ref_max(hs / (T(1) - v_S / (l1 * l1)), T(0)));
            }
        }
        // newton.hpp:241-263: a small bracket starts at h_min, else adaptive bisection from h_max towards h_min
        h = h_min;
        const bool probes = hard && !(double(h_max - h_min) <= 1e-1);
        bool bis = probes;
        T hc = h_max;
        while (__any(bis)) {
            const T w = ref_max(l1 / (min_nnz * hc + l1), T(0.05));
            const T hn = w * h_min + (T(1) - w) * hc;
            T t;
            g.sum2([hn, l1](T a, T v, T&, bool, T& t0, T& t1) { // root_function (utils.hpp:107)
                const T z = v / (a * hn + l1);
                t0 = z * z, t1 = T(0);
            }, t, s1);
            const T fh = t - T(1);
            if (bis) {
                // (probes step down towards h_min; one that rounding keeps from stepping down would repeat for ever: it ends the loop)
                bis = fh < T(0) && fabs(fh) > tol && hn < hc;
                hc = hn;
            }
        }
        if (probes) h = hc;
    }

    // newton.hpp:83-93; `commit`: the group takes this step (else its held r stays)
    auto step_f = [&](T hh, bool commit, T& fh, T& dfh) {
        T t, s;
        g.sum2([hh, l1, commit](T a, T v, T& r, bool, T& t0, T& t1) {
            const T rn = T(1) / (a * hh + l1);
            const T z = v * rn;
            const T xi = z * z;
            t0 = xi;
            t1 = xi * a * rn;
            if (commit) r = rn;
        }, t, s);
        const T sqrt_t = sqrt(t);
        fh = T(double(t) - 1.0);
        dfh = -s * (T(1) + sqrt_t) / t;
    };
    // optimization/newton.hpp:44-64
    T fh, dfh;
    step_f(h, true, fh, dfh);
    int64_t iters = 0;
    bool act = hard && fabs(fh) > tol && iters < P.max_iters;
    while (__any(act)) {
        const T hn = ref_max(h - fh / dfh, T(0));
        T fn, dfn;
        step_f(hn, act, fn, dfn);
        if (act) {
            h = hn, fh = fn, dfh = dfn;
            ++iters;
            act = fabs(fh) > tol && iters < P.max_iters;
        }
    }

    if (!live) return;
    if (zero) g.each([x](T, T, T, int64_t i) { x[i] = T(0); });
    else if (closed) g.each([x](T a, T v, T, int64_t i) { x[i] = v / a; });
    else
        g.each([x, h, l1](T a, T v, T r, int64_t i) {
            if (!G::kHoldsR) r = T(1) / (a * h + l1); // the bits step_f had at this h
            x[i] = h * v * r;
        });
    iters_out = iters;
    status_out = (hard && fabs(fh) > tol) ? ADELIE_HIP_BCD_MAX_ITERS : ADELIE_HIP_BCD_OK;
}

// ---- the kernels ----------------------------------------------------------------------------------------------------------------------
// list: the class's problems in launch order, n of them
template <class T, int W>
__global__ __launch_bounds__(kBcdBlock) void bcd_team_kernel(BcdParams<T> P, const int32_t* __restrict__ list, int64_t n) {
    const int tid = threadIdx.x;
    const int64_t pos = int64_t(blockIdx.x) * (kBcdBlock / W) + tid / W;
    const bool live = pos < n;
    TeamGroup<T, W> g;
    g.j = tid % W;
    g.a = T(1), g.v = T(0), g.r = T(0), g.ok = false;
    T l1 = T(1);
    int64_t begin = 0, d = 0;
    int32_t k = 0;
    if (live) {
        k = list[pos];
        begin = P.off[k];
        d = P.off[k + 1] - begin;
        l1 = P.l1[k];
        if (g.j < d) {
            g.a = P.quad[begin + g.j] + P.l2[k];
            g.v = P.lin[begin + g.j];
            g.ok = true;
        }
    }
    int64_t iters = 0;
    int32_t status = 0;
    bcd_solve_group<T>(g, P, l1, d, live, P.beta + begin, iters, status);
    if (live && g.j == 0) P.iters[k] = iters, P.status[k] = status;
}

template <class T, int NT>
__global__ __launch_bounds__(64) void bcd_wave_kernel(BcdParams<T> P, const int32_t* __restrict__ list) {
    const int32_t k = list[blockIdx.x];
    const int64_t begin = P.off[k];
    const int64_t d = P.off[k + 1] - begin;
    const T l1 = P.l1[k], l2 = P.l2[k];
    WaveGroup<T, NT> g;
    g.lane = threadIdx.x, g.d = int(d);
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        const int i = g.lane + 64 * m;
        const bool ok = i < g.d;
        g.a[m] = ok ? P.quad[begin + i] + l2 : T(1);
        g.v[m] = ok ? P.lin[begin + i] : T(0);
        g.r[m] = T(0);
    }
    int64_t iters = 0;
    int32_t status = 0;
    bcd_solve_group<T>(g, P, l1, d, true, P.beta + begin, iters, status);
    if (threadIdx.x == 0) P.iters[k] = iters, P.status[k] = status;
}

template <class T, bool LDS>
__global__ __launch_bounds__(kBcdBlock) void bcd_block_kernel(BcdParams<T> P, const int32_t* __restrict__ list) {
    extern __shared__ __attribute__((aligned(16))) char bcd_sm[];
    __shared__ T red[8];
    const int32_t k = list[blockIdx.x];
    const int64_t begin = P.off[k];
    const int64_t d = P.off[k + 1] - begin;
    const T l1 = P.l1[k], l2 = P.l2[k];
    BlockGroup<T, LDS> g;
    g.red = red, g.d = d, g.tid = threadIdx.x, g.l2 = l2;
    if (LDS) {
        T* sa = reinterpret_cast<T*>(bcd_sm);
        T* sv = sa + d;
        for (int64_t i = threadIdx.x; i < d; i += kBcdBlock) sa[i] = P.quad[begin + i] + l2, sv[i] = P.lin[begin + i];
        g.sa = sa, g.sv = sv;
        __syncthreads();
    } else {
        g.sa = P.quad + begin, g.sv = P.lin + begin;
    }
    int64_t iters = 0;
    int32_t status = 0;
    bcd_solve_group<T>(g, P, l1, d, true, P.beta + begin, iters, status);
    if (threadIdx.x == 0) P.iters[k] = iters, P.status[k] = status;
}

// ---- the host driver ---------------------------------------------------------------------------------------------------------------
constexpr int kBcdClasses = 11; // team 4, 8, 16, 32, 64; wave 2, 4, 8, 16 tiles; workgroup staged, workgroup from global memory

inline int bcd_class(int64_t d, int64_t lds_max_d) {
    if (d <= 4) return 0;
    if (d <= 8) return 1;
    if (d <= 16) return 2;
    if (d <= 32) return 3;
    if (d <= 64) return 4;
    if (d <= 128) return 5;
    if (d <= 256) return 6;
    if (d <= 512) return 7;
    if (d <= kBcdWaveMaxD) return 8;
    return d <= lds_max_d ? 9 : 10;
}

// synchronises the stream and hands it back before the buffers declared in front of it are parked
struct BcdStream {
    hipStream_t s = StreamPool::take();
    ~BcdStream() {
        (void)hipStreamSynchronize(s);
        StreamPool::give(s);
    }
};

template <class T, int W>
void bcd_launch_team(const BcdParams<T>& P, const int32_t* list, int64_t n, hipStream_t s) {
    const int64_t per_block = kBcdBlock / W;
    hipLaunchKernelGGL((bcd_team_kernel<T, W>), dim3(unsigned((n + per_block - 1) / per_block)), dim3(kBcdBlock), 0, s, P, list, n);
}

template <class T>
void bcd_run(const adelie_hip_bcd_args* a) {
    const int64_t B = a->n_problems;
    const int64_t total = a->offsets[B];
    AHIP_CHECK(hipSetDevice(a->device));
    int lds_limit = 0;
    if (hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, a->device) != hipSuccess || lds_limit <= 0) {
        (void)hipGetLastError();
        lds_limit = 65536;
    }
    const int64_t lds_max_d = std::min<int64_t>(bcd_lds_max_d<T>(), (int64_t(lds_limit) - int64_t(kBcdLdsReserve)) / int64_t(2 * sizeof(T)));

    // the launch lists: counting sort of the problems by class (problems of no values have nothing to solve)
    int64_t count[kBcdClasses] = {}, first[kBcdClasses + 1] = {};
    int64_t max_d_lds = 0;
    std::vector<int8_t> cls(static_cast<size_t>(B));
    for (int64_t k = 0; k < B; ++k) {
        const int64_t d = a->offsets[k + 1] - a->offsets[k];
        cls[size_t(k)] = d > 0 ? int8_t(bcd_class(d, lds_max_d)) : int8_t(-1);
        if (d > 0) ++count[cls[size_t(k)]];
        if (d > 0 && cls[size_t(k)] == 9) max_d_lds = std::max(max_d_lds, d);
    }
    for (int c = 0; c < kBcdClasses; ++c) first[c + 1] = first[c] + count[c];
    std::vector<int32_t> list(static_cast<size_t>(std::max<int64_t>(first[kBcdClasses], 1)));
    {
        int64_t at[kBcdClasses];
        std::copy(first, first + kBcdClasses, at);
        for (int64_t k = 0; k < B; ++k)
            if (cls[size_t(k)] >= 0) list[size_t(at[cls[size_t(k)]]++)] = int32_t(k);
    }

    DevBuf<int64_t> d_off, d_iters;
    DevBuf<int32_t> d_list, d_status;
    DevBuf<T> d_quad, d_lin, d_l1, d_l2, d_beta;
    BcdStream bs;
    hipStream_t s = bs.s;
    auto input = [s](DevBuf<T>& buf, const void* src, bool is_dev, int64_t n) -> const T* {
        if (is_dev) return static_cast<const T*>(src);
        buf.reserve(size_t(n));
        buf.upload(static_cast<const T*>(src), size_t(n), s);
        return buf.p;
    };
    BcdParams<T> P{};
    d_off.reserve(size_t(B + 1)), d_off.upload(a->offsets, size_t(B + 1), s);
    d_list.reserve(list.size()), d_list.upload(list.data(), list.size(), s);
    P.off = d_off.p;
    P.quad = input(d_quad, a->quad, a->quad_is_dev != 0, total);
    P.lin = input(d_lin, a->linear, a->linear_is_dev != 0, total);
    P.l1 = input(d_l1, a->l1, a->l1_is_dev != 0, B);
    P.l2 = input(d_l2, a->l2, a->l2_is_dev != 0, B);
    P.beta = a->beta_is_dev ? static_cast<T*>(a->beta) : d_beta.reserve(size_t(total));
    P.iters = d_iters.reserve(size_t(B));
    P.status = d_status.reserve(size_t(B));
    P.tol = T(a->tol);
    P.max_iters = a->max_iters;
    P.solver = a->solver;

    const int32_t* L = d_list.p;
    auto n_of = [&](int c) { return count[c]; };
    auto at = [&](int c) { return L + first[c]; };
    if (n_of(0)) bcd_launch_team<T, 4>(P, at(0), n_of(0), s);
    if (n_of(1)) bcd_launch_team<T, 8>(P, at(1), n_of(1), s);
    if (n_of(2)) bcd_launch_team<T, 16>(P, at(2), n_of(2), s);
    if (n_of(3)) bcd_launch_team<T, 32>(P, at(3), n_of(3), s);
    if (n_of(4)) bcd_launch_team<T, 64>(P, at(4), n_of(4), s);
    if (n_of(5)) hipLaunchKernelGGL((bcd_wave_kernel<T, 2>), dim3(unsigned(n_of(5))), dim3(64), 0, s, P, at(5));
    if (n_of(6)) hipLaunchKernelGGL((bcd_wave_kernel<T, 4>), dim3(unsigned(n_of(6))), dim3(64), 0, s, P, at(6));
    if (n_of(7)) hipLaunchKernelGGL((bcd_wave_kernel<T, 8>), dim3(unsigned(n_of(7))), dim3(64), 0, s, P, at(7));
    if (n_of(8)) hipLaunchKernelGGL((bcd_wave_kernel<T, 16>), dim3(unsigned(n_of(8))), dim3(64), 0, s, P, at(8));
    if (n_of(9)) {
        const size_t dyn = size_t(max_d_lds) * 2 * sizeof(T);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bcd_block_kernel<T, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, int(dyn));
        (void)hipGetLastError();
        hipLaunchKernelGGL((bcd_block_kernel<T, true>), dim3(unsigned(n_of(9))), dim3(kBcdBlock), dyn, s, P, at(9));
    }
    if (n_of(10)) hipLaunchKernelGGL((bcd_block_kernel<T, false>), dim3(unsigned(n_of(10))), dim3(kBcdBlock), 0, s, P, at(10));
    AHIP_CHECK(hipGetLastError());

    std::vector<int32_t> status(static_cast<size_t>(B));
    if (!a->beta_is_dev) d_beta.download(static_cast<T*>(a->beta), size_t(total), s);
    d_iters.download(a->iters, size_t(B), s);
    d_status.download(status.data(), size_t(B), s);
    AHIP_CHECK(hipStreamSynchronize(s));
    for (int64_t k = 0; k < B; ++k)
        if (cls[size_t(k)] < 0) a->iters[k] = 0, status[size_t(k)] = ADELIE_HIP_BCD_OK; // (no kernel wrote them)
    if (a->status) std::copy(status.begin(), status.end(), a->status);
}

} // namespace
} // namespace ahip

using namespace ahip;

extern "C" int adelie_hip_bcd_solve(const adelie_hip_bcd_args* a) {
    ABI_TRY
    const auto t0 = std::chrono::steady_clock::now();
    if (!a) throw make_core_error("null argument.");
    if (a->solver != ADELIE_HIP_BCD_NEWTON && a->solver != ADELIE_HIP_BCD_NEWTON_ABS) throw make_core_error("bcd: unknown solver.");
    if (a->dtype != ADELIE_HIP_F32 && a->dtype != ADELIE_HIP_F64) throw make_core_error("bcd: bad dtype.");
    const int64_t B = a->n_problems;
    if (B < 0 || B > (int64_t(1) << 24)) throw make_core_error("bcd: n_problems must be in [0, 2^24].");
    if (a->tol < 0) throw make_solver_error("tol must be >= 0.");
    if (a->max_iters < 0) throw make_core_error("bcd: max_iters must be >= 0.");
    if (B > 0) {
        if (!a->offsets || !a->l1 || !a->l2 || !a->iters) throw make_core_error("null argument.");
        if (a->offsets[0] != 0) throw make_core_error("bcd: offsets must start at 0.");
        for (int64_t k = 0; k < B; ++k)
            if (a->offsets[k + 1] < a->offsets[k]) throw make_core_error("bcd: offsets must not decrease.");
        if (a->offsets[B] > 0 && (!a->quad || !a->linear || !a->beta)) throw make_core_error("null argument.");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess) {
            (void)hipGetLastError();
            count = 0;
        }
        if (a->device < 0 || a->device >= count) throw make_core_error("bcd: no such device (adelie_amd has no CPU fallback).");
        DTYPE_DISPATCH(a, bcd_run<T>(a))
    }
    if (a->time_elapsed) *a->time_elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ABI_CATCH
}
