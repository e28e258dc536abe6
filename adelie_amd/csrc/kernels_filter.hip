// kernels_filter.hip — the filtered invariance sweep: a float32 or 16-bit shadow of a dense f64 design (gfx950 / CDNA4).
//
// The per-lambda gradient sweep is consumed almost only through comparisons with thresholds (KKT, the screening rules).  With
// xs_j = column j rounded to float32 and e_j = ||x_j - xs_j||_2 measured when the copy is made, |x_j.v - xs_j.v| <= e_j ||v||_2:
// a sweep of the copy (half the bytes) proves most columns to lie below every threshold, and only the others are swept
// again in f64.  The exact sweeps over a column list (list_column_sum) repeat, per column, the arithmetic of sweep_kernel
// (kernels_sweep.hip) on the row splits of the FULL design, so their values are the bits the full sweep gives.
// One filtered sweep is four launches (enqueue_filtered_sweep, the one sequence the solver and the test entry share):
//   vmul_sq_kernel          v = w o r and the partial sums of v^2
//   shadow_sweep_kernel     the shadow over all columns (panels of kShadowCB = 8 columns: 16 B of v per 64 B of design) and,
//                           in workgroups of its own first in the grid, the columns that are exact whatever the shadow says
//                           (screen columns, columns of groups without a penalty), their split partials into staging
//   filter_classify_kernel  ||v||; the staged columns reduced in split order, guarded against their shadow values and stored;
//                           the open groups listed in group order.  It owns the four meta words: no memset ahead of it
//   sweep_list_kernel       the listed columns (it reads their count from the device)
// (a shape whose shadow or list splits the rows adds the reduce launch of those partials).
// The copy has two kinds (shadow_kind_host.hpp picks one per design): float32 values, or q15 -- int16 values with one f64 scale
// per column, a quarter of the design's bytes, with e_j about 4e-5 ||x_j|| on Gaussian columns.  Nothing but the build kernel
// and the shadow part of the second launch (ShadowF32 / ShadowQ15) knows the kind: the bound is the measured e_j either way.
#include "sweep_common.hpp"
#include <algorithm>
#include <cfloat>

namespace ahip {

namespace {

__global__ __launch_bounds__(kThreads) void shadow_build_kernel(const double* __restrict__ X, int64_t ld, int64_t n,
                                                                float* __restrict__ Xs, int64_t lds, double* __restrict__ err,
                                                                double* __restrict__ nrm, int32_t* __restrict__ bad) {
    const int64_t j = blockIdx.x;
    const int tid = threadIdx.x;
    const double* col = X + j * ld;
    float* dst = Xs + j * lds;
    double e2 = 0, n2 = 0;
    bool any_bad = false;
    for (int64_t i = tid; i < lds; i += kThreads) {
        float f = 0.f;
        if (i < n) {
            const double x = col[i];
            const bool ok = fabs(x) <= double(FLT_MAX); // (false for NaN and +-inf as well)
            any_bad = any_bad || !ok;
            f = ok ? float(x) : 0.f;
            const double d = x - double(f);
            e2 = fma(d, d, e2);
            n2 = fma(double(f), double(f), n2);
        }
        dst[i] = f;
    }
    __shared__ double red[2][kThreads / 64];
    const int lane = tid & 63, wv = tid >> 6;
    e2 = wave_sum(e2);
    n2 = wave_sum(n2);
    if (lane == 0) { red[0][wv] = e2; red[1][wv] = n2; }
    __syncthreads();
    if (tid == 0) {
        double a = 0, b = 0;
        for (int w = 0; w < kThreads / 64; ++w) { a += red[0][w]; b += red[1][w]; }
        // (rounded up a little: the sums above carry their own rounding error)
        err[j] = sqrt(a) * (1.0 + 1e-9);
        nrm[j] = sqrt(b) * (1.0 + 1e-9);
    }
    if (any_bad) atomicOr(bad, 1);
}

// The q15 copy of one column per workgroup, in two passes: m = max_i |x_i|, then q_i = clamp(rint(x_i * (32767 / m)), +-32767) with
// scale[j] = m / 32767 (one multiplication, round-half-even: a numpy restatement gives the same integers).  The copy it stands
// for is xs_i = fl(scale q_i): a 0/1 column has err 0.  err is summed on (x_i - xs_i) / scale and nrm on q_i, so neither overflows
// on a column of huge entries.  A column whose m is 0, or so small that 32767 / m overflows or m / 32767 is subnormal (m below
// about 7.3e-304), is stored as zeros with scale 0 and err = sqrt(n) m >= ||x_j||: every scale in use is a normal number, which
// the fp_term of the kind assumes.  Rows n .. lds-1 are written as 0.
__global__ __launch_bounds__(kThreads) void shadow_build_q15_kernel(const double* __restrict__ X, int64_t ld, int64_t n,
                                                                    int16_t* __restrict__ Xq, int64_t lds,
                                                                    double* __restrict__ scale, double* __restrict__ err,
                                                                    double* __restrict__ nrm, int32_t* __restrict__ bad) {
#pragma clang fp contract(off) // x - fl(scale q) must not become one fma: the copy is fl(scale q), and a 0/1 column has err 0
    const int64_t j = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double* col = X + j * ld;
    int16_t* dst = Xq + j * lds;
    __shared__ double red[2][kThreads / 64];
    double m = 0;
    bool any_bad = false;
    for (int64_t i = tid; i < n; i += kThreads) {
        const double a = fabs(col[i]);
        const bool ok = a <= DBL_MAX; // (false for NaN and +-inf)
        any_bad = any_bad || !ok;
        m = ok ? fmax(m, a) : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
    if (lane == 0) red[0][wv] = m;
    __syncthreads();
    m = red[0][0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) m = fmax(m, red[0][w]);
    __syncthreads();
    double inv = m > 0 ? 32767.0 / m : 0.0;
    double sc = m / 32767.0;
    if (!(inv <= DBL_MAX) || !(sc >= DBL_MIN)) { inv = 0; sc = 0; } // (a subnormal scale would round absolutely, not relatively)
    double e2 = 0, q2 = 0;
    for (int64_t i = tid; i < lds; i += kThreads) {
        int q = 0;
        if (i < n && sc > 0) {
            double x = col[i];
            if (!(fabs(x) <= DBL_MAX)) x = 0;
            const double t = fmin(fmax(rint(__dmul_rn(x, inv)), -32767.0), 32767.0);
            q = int(t);
            const double d = (x - __dmul_rn(sc, t)) / sc;
            e2 = fma(d, d, e2);
            q2 = fma(t, t, q2);
        }
        dst[i] = int16_t(q);
    }
    e2 = wave_sum(e2);
    q2 = wave_sum(q2);
    if (lane == 0) { red[0][wv] = e2; red[1][wv] = q2; }
    __syncthreads();
    if (tid == 0) {
        double a = 0, b = 0;
        for (int w = 0; w < kThreads / 64; ++w) { a += red[0][w]; b += red[1][w]; }
        scale[j] = sc;
        // (rounded up a little: the sums above carry their own rounding error)
        err[j] = (sc > 0 ? sc * sqrt(a) : sqrt(double(n)) * m) * (1.0 + 1e-9);
        nrm[j] = sc * sqrt(b) * (1.0 + 1e-9);
    }
    if (any_bad) atomicOr(bad, 1);
}

// out = a * b and, per workgroup, the sum of squares of its products (fixed grid, fixed order: ||out||_2 is reproducible)
__global__ __launch_bounds__(kThreads) void vmul_sq_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                           double* __restrict__ out, int64_t n, double* __restrict__ part) {
    double acc = 0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
        const double x = a[i] * b[i];
        out[i] = x;
        acc = fma(x, x, acc);
    }
    __shared__ double red[kThreads / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    acc = wave_sum(acc);
    if (lane == 0) red[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0;
        for (int w = 0; w < kThreads / 64; ++w) s += red[w];
        part[blockIdx.x] = s;
    }
}

// |exact - shadow| <= bound must hold for every column swept both ways: a design modified after the copy was made shows here
__device__ __forceinline__ void shadow_guard(double exact, double approx, int64_t j, const double* __restrict__ err,
                                             const double* __restrict__ nrm, double fp_term, const double* __restrict__ vnorm,
                                             int32_t* __restrict__ flags) {
    const double bound = (err[j] + fp_term * nrm[j]) * vnorm[0];
    if (!(fabs(exact - approx) <= bound)) atomicOr(flags, 2);
}

// One column, one row split: per thread the loop of sweep_kernel, then its wave and workgroup reductions (any CB gives a
// column the same bits).  The sum is valid in thread 0; red: kThreads / 64 doubles of LDS.
template <int VEC>
__device__ __forceinline__ double list_column_sum(const DenseAcc<double>& X, const double* __restrict__ v, int64_t j, int64_t r0,
                                                  int64_t r1, double* red) {
    const int tid = threadIdx.x;
    const double* cp = X.colptr(j);
    double acc = 0;
    const int64_t body_end = r0 + ((r1 - r0) / VEC) * VEC;
#pragma unroll 8
    for (int64_t i = r0 + int64_t(tid) * VEC; i < body_end; i += int64_t(kThreads) * VEC) {
        const Pack<double, VEC> vv = load_vec<double, VEC>(v + i);
        const Pack<double, VEC> xx = X.template load<VEC>(cp, i, j);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc = fma(xx.v[e], vv.v[e], acc);
    }
    for (int64_t i = body_end + tid; i < r1; i += kThreads) acc = fma(X.template load<1>(cp, i, j).v[0], v[i], acc);
    const int lane = tid & 63, wv = tid >> 6;
    const double ws = wave_sum(acc);
    if (lane == 0) red[wv] = ws;
    __syncthreads();
    double s = 0;
    if (tid == 0) {
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) s += red[w];
    }
    return s;
}

// The two kinds of copy as the shadow sweep sees them: the element type, the 16-byte load of VEC rows of one column, row e of
// a loaded vector as a double (the sweep takes e = 0 .. VEC-1 in order), the panel width CB, whether the body loop is the
// rotation of two half panels (kPipelined) or the plain loop unrolled kUnroll times, the waves per SIMD the compiler has to
// leave room for (1: no demand), and whether a column's sum is multiplied by scale[c] before the centring term.
struct ShadowF32 {
    using elem = float;
    using vec = f4_t;
    static constexpr int CB = kShadowCB, VEC = kShadowVec, kUnroll = 2;
    static constexpr bool kScaled = false, kPipelined = false;
    static constexpr int kMinWaves = 1;
    static __device__ __forceinline__ double row(vec x, int e) { return double(x[e]); }
};
// q15: 16-byte non-temporal loads of 8 rows per lane and column, q . v accumulated in f64 and the sum of a workgroup's rows
// multiplied by scale[c] once (a row split's partial is scaled before it is stored: sweep_reduce_kernel is shared).
// The body loop is pipelined (shadow_sweep_kernel): 88 VGPRs, no scratch, 5 waves per SIMD, and per column the fmas of the plain
// loop in its order, so the values are those it gave (profiles/shadow_q15_rate.txt).
// fp_term of this kind (ShadowView::fp_term), with u = 2^-53, xs_i = fl(scale q_i) the copy that err / nrm were measured on
// (scale is 0 or a normal number, shadow_build_q15_kernel, so a product with it rounds relatively):
//   q_i is exact in f64 and every product enters through an fma, so the sum of n terms in any order, with the one rounding of
//   the multiplication by scale somewhere in its tree, is off by at most n u scale sum|q_i v_i| <= n u (1 + u) nrm ||v||;
//   scale q_i against xs_i: u nrm ||v||;
//   the f64 sweep it is compared with: n u ||x_j|| ||v||, with ||x_j|| <= nrm + err;
//   the subtractions of the same centring term from both: as in the float32 kind.
// (2 n + 1) u nrm, doubled as the float32 kind's 2 n u is, and rounded up: fp_term = (4 n + 8) u.
typedef int i4_t __attribute__((ext_vector_type(4)));
struct ShadowQ15 {
    using elem = int16_t;
    using vec = i4_t;
    static constexpr int CB = kShadowCB16, VEC = kShadowVec16;
    static constexpr bool kScaled = true, kPipelined = true;
    static constexpr int kMinWaves = 5;
    static_assert(VEC == 8, "one 16-byte load holds 8 rows");
    static __device__ __forceinline__ double row(vec x, int e) { // word w holds rows 2w (low half) and 2w + 1 (high half)
        return e % 2 ? double(x[e / 2] >> 16) : double(int(int16_t(x[e / 2])));
    }
};

// p, which every lane holds alike, as a value the compiler keeps in scalar registers (the address of a load is then this base
// plus the lane's 32-bit offset, and no lane spends two registers per column on it)
template <class T>
using global_ptr = const __attribute__((address_space(1))) T*;
template <class T>
__device__ __forceinline__ global_ptr<T> uniform_ptr(const T* p) {
    const uint64_t u = reinterpret_cast<uint64_t>(p);
    const uint32_t l = __builtin_amdgcn_readfirstlane(uint32_t(u)), h = __builtin_amdgcn_readfirstlane(uint32_t(u >> 32));
    return reinterpret_cast<global_ptr<T>>((uint64_t(h) << 32) | l);
}

// A workgroup of the exact part of the shadow launch: entry c of the lists xa, xb taken as one, row split xsplit of the FULL
// design's shape; the split's partial goes to stage[xsplit * (na + nb) + c].  red: kThreads / 64 doubles of LDS.
template <int XVEC>
__device__ __forceinline__ void exact_part(const DenseAcc<double>& X, const double* __restrict__ v, int64_t n,
                                           const int32_t* __restrict__ xa, int64_t na, const int32_t* __restrict__ xb,
                                           int64_t nb, int64_t x_rows_per_split, double* __restrict__ stage, double* red) {
    const int64_t ne = na + nb;
    const int64_t c = int64_t(blockIdx.x) % ne;
    const int64_t xsplit = int64_t(blockIdx.x) / ne;
    const int64_t j = c < na ? xa[c] : xb[c - na];
    const int64_t xr0 = xsplit * x_rows_per_split;
    const double s = list_column_sum<XVEC>(X, v, j, xr0, min(n, xr0 + x_rows_per_split), red);
    if (threadIdx.x == 0) stage[xsplit * ne + c] = s;
}

// One launch, two kinds of workgroup.  The first (na + nb) * x_nsplit workgroups sweep in f64 the columns that are exact
// whatever the shadow says (xa: the screen columns, xb: the columns of the groups without a penalty): exact_part.  They neither
// read nor write `out`: filter_classify_kernel reduces the staged partials, compares with the shadow value and stores the exact
// one.  The other blocks_c * nsplit workgroups: out[c] = sum_i xs[i, c] * v[i] over all columns of the copy (Kind), f64
// accumulation, per column rows ascending with one fma each; row splits (the shadow's own shape) and epilogue as sweep_kernel.
template <class Kind, int XVEC>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(Kind::kMinWaves))) void shadow_sweep_kernel(
                                                                const typename Kind::elem* __restrict__ Xs, int64_t ld,
                                                                const double* __restrict__ scale, const double* __restrict__ v,
                                                                double* __restrict__ out, int64_t n, int64_t ncols,
                                                                int64_t blocks_c, int64_t rows_per_split, int nsplit,
                                                                const double* __restrict__ sub_scale,
                                                                const double* __restrict__ sub_vec, DenseAcc<double> X,
                                                                const int32_t* __restrict__ xa, int64_t na,
                                                                const int32_t* __restrict__ xb, int64_t nb,
                                                                int64_t x_rows_per_split, int x_nsplit, double* __restrict__ stage) {
    constexpr int CB = Kind::CB, VEC = Kind::VEC;
    const int tid = threadIdx.x;
    const int64_t n_exact = (na + nb) * x_nsplit;
    __shared__ double red[kThreads / 64][CB];
    if (int64_t(blockIdx.x) < n_exact) {
        exact_part<XVEC>(X, v, n, xa, na, xb, nb, x_rows_per_split, stage, &red[0][0]);
        return;
    }
    const int64_t b = int64_t(blockIdx.x) - n_exact;
    const int64_t cb = b % blocks_c;
    const int split = int(b / blocks_c);
    const int64_t r0 = int64_t(split) * rows_per_split;
    const int64_t r1 = min(n, r0 + rows_per_split);
    const typename Kind::elem* cp[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k) {
        int64_t c = cb * CB + k;
        if (c >= ncols) c = ncols - 1; // duplicate work on the tail panel, discarded below
        cp[k] = Xs + c * ld;
    }
    double acc[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k) acc[k] = 0;
    // r0 is a multiple of 256 * VEC rows and ld of 16 bytes: every load below is 16-byte aligned and ends at or before row r1 <= n
    const int64_t body_end = r0 + ((r1 - r0) / VEC) * VEC;
    if constexpr (Kind::kPipelined) {
        // The trips in which every lane has a load (all but the last, when the split's rows are no multiple of kThreads * VEC)
        // run as two half panels in rotation: while the columns of one half are multiplied, the loads of the other half (of
        // the same rows, or of the next trip's) are in flight.  Per column and lane the fmas are those of the plain loop
        // below, in its order.  The trip count is uniform and a trip's addresses are uniform bases, advanced per trip, plus
        // the lane's offset of tid * VEC elements: the column pointers stay in scalar registers, which is what keeps the
        // rotation within the registers of 5 waves per SIMD.  The last, partial trip follows on its own.
        constexpr int H = CB / 2;
        static_assert(CB % 2 == 0, "two half panels");
        constexpr int64_t kStep = int64_t(kThreads) * VEC;
        const uint32_t lo = uint32_t(tid) * VEC;
        const int64_t full_trips = (body_end - r0) / kStep;
        int64_t row = r0; // the first row of the trip
        const auto xbase = [&](int k) { return uniform_ptr(cp[k] + row) + lo; };
        const auto vbase = [&]() { return uniform_ptr(v + row) + lo; };
        if (full_trips > 0) {
            d2_t vc[VEC / 2], vn[VEC / 2];
            typename Kind::vec ha[H], hb[H];
            // the fmas of one half panel between two scheduling barriers: the compiler keeps the loads written before them
            // before them and those written after them after them, which is the rotation
            const auto half = [&](typename Kind::vec(&x)[H], int k0) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < H; ++k) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[k0 + k] = fma(Kind::row(x[k], e), vc[e / 2][e % 2], acc[k0 + k]);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            const auto load_half = [&](typename Kind::vec(&x)[H], int k0) {
#pragma unroll
                for (int k = 0; k < H; ++k) x[k] = __builtin_nontemporal_load(reinterpret_cast<global_ptr<typename Kind::vec>>(xbase(k0 + k)));
            };
            const auto load_v = [&](d2_t(&vv)[VEC / 2]) {
#pragma unroll
                for (int e = 0; e < VEC / 2; ++e) vv[e] = *reinterpret_cast<global_ptr<d2_t>>(vbase() + 2 * e);
            };
            load_v(vc);
            load_half(ha, 0);
            load_half(hb, H);
            for (int64_t t = 1; t < full_trips; ++t) { // (every trip but the last loads the next one's rows: no load under a condition)
                row += kStep;
                half(ha, 0);
                load_half(ha, 0);
                load_v(vn);
                half(hb, H);
                load_half(hb, H);
#pragma unroll
                for (int e = 0; e < VEC / 2; ++e) vc[e] = vn[e];
                __builtin_amdgcn_sched_barrier(0);
            }
            row += kStep;
            half(ha, 0);
            half(hb, H);
        }
        if (row + int64_t(lo) < body_end) { // (row: the first row after the full trips)
            d2_t vv[VEC / 2];
#pragma unroll
            for (int e = 0; e < VEC / 2; ++e) vv[e] = *reinterpret_cast<global_ptr<d2_t>>(vbase() + 2 * e);
            typename Kind::vec xx[CB];
#pragma unroll
            for (int k = 0; k < CB; ++k) xx[k] = __builtin_nontemporal_load(reinterpret_cast<global_ptr<typename Kind::vec>>(xbase(k)));
#pragma unroll
            for (int k = 0; k < CB; ++k) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[k] = fma(Kind::row(xx[k], e), vv[e / 2][e % 2], acc[k]);
            }
        }
    } else {
#pragma unroll Kind::kUnroll
        for (int64_t i = r0 + int64_t(tid) * VEC; i < body_end; i += int64_t(kThreads) * VEC) {
            d2_t vv[VEC / 2];
#pragma unroll
            for (int e = 0; e < VEC / 2; ++e) vv[e] = *reinterpret_cast<const d2_t*>(v + i + 2 * e);
            typename Kind::vec xx[CB];
#pragma unroll
            for (int k = 0; k < CB; ++k) xx[k] = __builtin_nontemporal_load(reinterpret_cast<const typename Kind::vec*>(cp[k] + i));
#pragma unroll
            for (int k = 0; k < CB; ++k) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[k] = fma(Kind::row(xx[k], e), vv[e / 2][e % 2], acc[k]);
            }
        }
    }
    for (int64_t i = body_end + tid; i < r1; i += kThreads) {
        const double vi = v[i];
#pragma unroll
        for (int k = 0; k < CB; ++k) acc[k] = fma(double(cp[k][i]), vi, acc[k]);
    }
    panel_epilogue<Kind::kScaled>(acc, red, cb, ncols, 0, nullptr, scale, out, split, nsplit, sub_scale, sub_vec);
}

// One column per workgroup, the first *count_dev (or max_cols) entries of `cols`: list_column_sum on the row splits the caller
// took from the full design's shape; the result goes to out[column].  err != nullptr: out[column] holds the shadow's value on
// entry (shadow_guard).
template <int VEC>
__global__ __launch_bounds__(kThreads) void sweep_list_kernel(DenseAcc<double> X, const double* __restrict__ v,
                                                              double* __restrict__ out, double* __restrict__ part, int64_t n,
                                                              const int32_t* __restrict__ cols, int64_t max_cols,
                                                              const int32_t* __restrict__ count_dev, int64_t rows_per_split,
                                                              int nsplit, const double* __restrict__ sub_scale,
                                                              const double* __restrict__ sub_vec, const double* __restrict__ err,
                                                              const double* __restrict__ nrm, double fp_term,
                                                              const double* __restrict__ vnorm, int32_t* __restrict__ flags) {
    const int64_t c = blockIdx.x;
    const int64_t count = count_dev ? min(int64_t(count_dev[0]), max_cols) : max_cols;
    if (c >= count) return;
    const int split = blockIdx.y;
    const int64_t r0 = int64_t(split) * rows_per_split;
    const int64_t j = cols[c];
    __shared__ double red[kThreads / 64];
    double s = list_column_sum<VEC>(X, v, j, r0, min(n, r0 + rows_per_split), red);
    if (threadIdx.x == 0) {
        if (nsplit == 1) { // (not store_sum: shadow_guard has to see the centred value before it replaces the shadow's in out[j])
            s = centred(s, j, sub_scale, sub_vec);
            if (err) shadow_guard(s, out[j], j, err, nrm, fp_term, vnorm, flags);
            out[j] = s;
        } else {
            part[int64_t(split) * max_cols + c] = s;
        }
    }
}
__global__ void sweep_list_reduce_kernel(const double* __restrict__ part, double* __restrict__ out,
                                         const int32_t* __restrict__ cols, int64_t max_cols,
                                         const int32_t* __restrict__ count_dev, int nsplit, const double* __restrict__ sub_scale,
                                         const double* __restrict__ sub_vec, const double* __restrict__ err,
                                         const double* __restrict__ nrm, double fp_term, const double* __restrict__ vnorm,
                                         int32_t* __restrict__ flags) {
    const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t count = count_dev ? min(int64_t(count_dev[0]), max_cols) : max_cols;
    if (c >= count) return;
    const int64_t j = cols[c];
    double s = 0;
    for (int r = 0; r < nsplit; ++r) s += part[int64_t(r) * max_cols + c];
    s = centred(s, j, sub_scale, sub_vec);
    if (err) shadow_guard(s, out[j], j, err, nrm, fp_term, vnorm, flags);
    out[j] = s;
}

// One workgroup, the step after the fused shadow launch.
//  - ||v||_2 from the partial sums of vmul_sq_kernel.
//  - The columns swept exactly inside the shadow launch (xa, then xb: entry c of the two lists taken as one has its x_nsplit
//    split partials at stage[split * (na + nb) + c]): partials added in split order, the centring term, shadow_guard against
//    the shadow's value in grad, then grad[column] = the exact value.  xb after xa, a barrier between: a column in both lists
//    is compared the second time with what the first pass stored, as two list sweeps one after the other would.
//  - Per group outside the screen set (slot < 0) with a positive penalty: approximate norm a of its gradient block and the
//    bound eps on its distance from the exact one; the columns of every group that a + eps cannot place below
//    thr_g = tstar * penalty_g are appended to `list`, in group order.  Per trip of kClassifyThreads * kClassifyRun groups
//    a thread loads the descriptors of kClassifyRun groups together, then their entries together (two round trips to memory,
//    coalesced), the counts pass through LDS, and the workgroup scans once over threads that each own kClassifyRun
//    consecutive groups.  kClassifyRun = 6 is what 128 VGPRs (1024 threads on one CU) hold without spilling.
// meta_i: [0] columns listed (at most cap), [1] flags (bit 0: more than cap, bit 1: shadow_guard), [2] columns wanted, [3] 0:
// all four are written here and nothing before this kernel touches them; the open-list sweep that follows ORs into [1].
// meta_d: [0] the inflated ||v||_2 the bounds use, [1] a copy of sub_scale[0] (what a later exact sweep of the same residual
// subtracts).
constexpr int kClassifyThreads = 1024, kClassifyRun = 6;
__global__ __launch_bounds__(kClassifyThreads) void filter_classify_kernel(
    double* __restrict__ grad, const int64_t* __restrict__ groups, const int64_t* __restrict__ group_sizes, int64_t G,
    const int32_t* __restrict__ slot, const double* __restrict__ penalty, double tstar, const double* __restrict__ err,
    const double* __restrict__ nrm, double fp_term, const double* __restrict__ sq_part, int n_part,
    const double* __restrict__ sub_scale, const double* __restrict__ sub_vec, const double* __restrict__ stage,
    const int32_t* __restrict__ xa, int64_t na, const int32_t* __restrict__ xb, int64_t nb, int x_nsplit,
    int32_t* __restrict__ list, int64_t cap, int32_t* __restrict__ meta_i, double* __restrict__ meta_d) {
    constexpr int NW = kClassifyThreads / 64, R = kClassifyRun;
    __shared__ double sred[NW];
    __shared__ int32_t wtot[NW];
    __shared__ double s_vnorm;
    __shared__ int32_t s_first[kClassifyThreads * R], s_want[kClassifyThreads * R]; // per group of a trip: first column, columns wanted
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    {
        double a = 0;
        for (int i = tid; i < n_part; i += kClassifyThreads) a += sq_part[i];
        a = wave_sum(a);
        if (lane == 0) sred[wv] = a;
        __syncthreads();
        if (tid == 0) {
            double s = 0;
            for (int w = 0; w < NW; ++w) s += sred[w];
            s_vnorm = sqrt(s) * (1.0 + 1e-6);
            meta_d[0] = s_vnorm;
            meta_d[1] = sub_scale ? sub_scale[0] : 0.0;
            meta_i[1] = 0;
            meta_i[3] = 0;
        }
        __syncthreads();
    }
    const double vnorm = s_vnorm;
    const int64_t ne = na + nb;
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t* xl = pass ? xb : xa;
        const int64_t c0 = pass ? na : 0, cnt = pass ? nb : na;
        for (int64_t c = tid; c < cnt; c += kClassifyThreads) {
            const int64_t j = xl[c];
            double s = 0;
            for (int r = 0; r < x_nsplit; ++r) s += stage[int64_t(r) * ne + c0 + c];
            s = centred(s, j, sub_scale, sub_vec);
            shadow_guard(s, grad[j], j, err, nrm, fp_term, &s_vnorm, meta_i + 1);
            grad[j] = s;
        }
        __syncthreads();
    }
    int64_t run = 0;
    for (int64_t base = 0; base < G; base += int64_t(kClassifyThreads) * R) {
        // the loads of R groups per thread, consecutive threads on consecutive groups: descriptors together, entries together
        int32_t k[R], sz[R];
        double thr[R], a2[R], b2[R];
        {
            int32_t sl[R];
            double pn[R];
            int64_t kk[R], ss[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int64_t gu = base + int64_t(u) * kClassifyThreads + tid;
                const int64_t g = gu < G ? gu : G - 1;
                sl[u] = slot[g];
                pn[u] = penalty[g];
                kk[u] = groups[g];
                ss[u] = group_sizes[g];
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const bool on = base + int64_t(u) * kClassifyThreads + tid < G && sl[u] < 0 && pn[u] > 0 && ss[u] > 0;
                k[u] = int32_t(kk[u]);
                sz[u] = on ? int32_t(ss[u]) : 0;
                thr[u] = tstar * pn[u];
                a2[u] = 0;
                b2[u] = 0;
            }
        }
        int32_t longest = 0;
#pragma unroll
        for (int u = 0; u < R; ++u) longest = max(longest, sz[u]);
        for (int32_t t = 0; t < longest; ++t) {
            double x[R], e[R], m[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int64_t at = t < sz[u] ? int64_t(k[u]) + t : 0;
                x[u] = grad[at];
                e[u] = err[at];
                m[u] = nrm[at];
            }
#pragma unroll
            for (int u = 0; u < R; ++u)
                if (t < sz[u]) {
                    const double b = e[u] + fp_term * m[u];
                    a2[u] = fma(x[u], x[u], a2[u]);
                    b2[u] = fma(b, b, b2[u]);
                }
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            if (sz[u] > 0) {
                const double reach = (sqrt(a2[u]) + sqrt(b2[u]) * vnorm * (1.0 + 1e-9)) * (1.0 + 1e-9);
                if (reach < thr[u]) sz[u] = 0;
            }
            s_first[u * kClassifyThreads + tid] = k[u];
            s_want[u * kClassifyThreads + tid] = sz[u];
        }
        __syncthreads();
        // a thread takes R consecutive groups of the trip: one exclusive scan of the per-thread counts over the workgroup
        int32_t mine = 0;
#pragma unroll
        for (int u = 0; u < R; ++u) mine += s_want[tid * R + u];
        int32_t inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t y = __shfl_up(inc, off, 64);
            if (lane >= off) inc += y;
        }
        if (lane == 63) wtot[wv] = inc;
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int w = 0; w < NW; ++w) {
            const int32_t t = wtot[w];
            if (w < wv) before += t;
            total += t;
        }
        int64_t at = run + before + inc - mine;
        if (mine > 0)
            for (int u = 0; u < R; ++u) {
                const int32_t first = s_first[tid * R + u], want = s_want[tid * R + u];
                for (int32_t t = 0; t < want; ++t, ++at)
                    if (at < cap) list[at] = first + t;
            }
        run += total;
        __syncthreads();
    }
    if (tid == 0) {
        meta_i[0] = int32_t(run < cap ? run : cap);
        if (run > cap) atomicOr(meta_i + 1, 1);
        meta_i[2] = int32_t(run < int64_t(0x7fffffff) ? run : int64_t(0x7fffffff));
    }
}

} // namespace

void launch_shadow_build(const DenseView<double>& X, float* Xs, int64_t lds, double* err, double* nrm, int32_t* bad,
                         hipStream_t s) {
    if (X.p <= 0) return;
    hipLaunchKernelGGL(shadow_build_kernel, dim3((unsigned)X.p), dim3(kThreads), 0, s, X.X, X.ld, X.n, Xs, lds, err, nrm, bad);
}
int64_t shadow_q15_ld(int64_t n) { return (n + kShadowPad16 - 1) / kShadowPad16 * kShadowPad16; }
void launch_shadow_build_q15(const DenseView<double>& X, int16_t* Xq, int64_t lds, double* scale, double* err, double* nrm,
                             int32_t* bad, hipStream_t s) {
    if (X.p <= 0) return;
    hipLaunchKernelGGL(shadow_build_q15_kernel, dim3((unsigned)X.p), dim3(kThreads), 0, s, X.X, X.ld, X.n, Xq, lds, scale, err, nrm,
                       bad);
}
int filter_norm_parts(int64_t n) { return int(grid1d(n, kThreads, 1024)); }

namespace {
struct ListShape {
    bool vec;
    int ns;
    int64_t rps;
};
// the row splits of the FULL design's sweep, whatever the length of a list
ListShape list_shape(const DenseView<double>& X, const double* v) {
    ListShape L;
    L.vec = dense_vec_ok(X) && (reinterpret_cast<uintptr_t>(v) % 16) == 0;
    int64_t blocks_c;
    sweep_shape(X.n, X.p, L.vec ? VecOf<double>::N : 1, blocks_c, L.ns, L.rps);
    return L;
}
// exact sweep of the first min(*count_dev, max_cols) columns of `cols`: out[cols[c]] = the bits launch_sweep over all X.p
// columns gives that column; out holds the shadow's values on entry and *flags |= 2 when a pair differs by more than its bound
void launch_sweep_list(const DenseView<double>& X, const double* v, double* out, const int32_t* cols, int64_t max_cols,
                       const int32_t* count_dev, const double* sub_scale, const double* sub_vec, const ShadowView& guard,
                       const double* vnorm, int32_t* flags, double* work, hipStream_t s) {
    if (max_cols <= 0) return;
    DenseAcc<double> acc{X.X, X.ld};
    const ListShape L = list_shape(X, v);
    const auto kernel = L.vec ? sweep_list_kernel<VecOf<double>::N> : sweep_list_kernel<1>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)max_cols, (unsigned)L.ns), dim3(kThreads), 0, s, acc, v, out, work, X.n, cols,
                       max_cols, count_dev, L.rps, L.ns, sub_scale, sub_vec, guard.err, guard.nrm, guard.fp_term(), vnorm, flags);
    if (L.ns > 1)
        hipLaunchKernelGGL(sweep_list_reduce_kernel, dim3((unsigned)((max_cols + 255) / 256)), dim3(256), 0, s, work, out, cols,
                           max_cols, count_dev, L.ns, sub_scale, sub_vec, guard.err, guard.nrm, guard.fp_term(), vnorm, flags);
}
// (the larger of the two kinds' split counts: the work buffer is sized before the kind is known to its owner)
int64_t shadow_work_elems(int64_t n, int64_t p) {
    int64_t blocks_c, rps;
    int ns, ns16;
    sweep_shape(n, p, kShadowVec, blocks_c, ns, rps, kShadowCB);
    sweep_shape(n, p, kShadowVec16, blocks_c, ns16, rps, kShadowCB16);
    return int64_t(std::max(ns, ns16)) * p + 16;
}
int64_t list_work_elems(int64_t n, int64_t p, int64_t max_cols) {
    int64_t blocks_c, rps;
    int ns;
    sweep_shape(n, p, 1, blocks_c, ns, rps); // VEC=1 gives the largest split count
    return int64_t(ns) * max_cols + 16;
}
// the fused launch over a copy of kind Kind (its own shape: split partials to a.work and a reduce launch when it splits the
// rows), the exact part on the list shape L with its partials to `stage`
template <class Kind, int XVEC>
void launch_shadow_sweep(const DenseView<double>& X, const ShadowView& S, const FilteredSweep& a, int64_t na, int64_t nb,
                         const ListShape& L, double* stage, hipStream_t s) {
    int64_t blocks_c, rps;
    int ns;
    sweep_shape(S.n, S.p, Kind::VEC, blocks_c, ns, rps, Kind::CB);
    hipLaunchKernelGGL((shadow_sweep_kernel<Kind, XVEC>), dim3((unsigned)((na + nb) * L.ns + blocks_c * ns)), dim3(kThreads), 0, s,
                       static_cast<const typename Kind::elem*>(S.X), S.ld, S.scale, a.v, ns == 1 ? a.grad : a.work, S.n, S.p,
                       blocks_c, rps, ns, a.sub_scale, a.sub_vec, DenseAcc<double>{X.X, X.ld}, a.screen_cols, na, a.pen0_cols, nb,
                       L.rps, L.ns, stage);
    if (ns > 1) launch_sweep_reduce<double>(a.work, a.grad, S.p, ns, 0, nullptr, a.sub_scale, a.sub_vec, s);
}
} // namespace

int64_t filtered_sweep_work_elems(int64_t n, int64_t p, int64_t n_before, int64_t cap) {
    return shadow_work_elems(n, p) + list_work_elems(n, p, std::max(n_before, cap));
}
void enqueue_filtered_sweep(const DenseView<double>& X, const ShadowView& S, const FilteredSweep& a, hipStream_t s) {
    if (S.p <= 0) return;
    const int64_t na = a.screen_cols ? a.n_screen_cols : 0, nb = a.pen0_cols ? a.n_pen0_cols : 0;
    // work: the shadow's split partials, then the staged partials of the exact part (the open-list sweep's after them)
    double* stage = a.work + shadow_work_elems(S.n, S.p);
    hipLaunchKernelGGL(vmul_sq_kernel, dim3(grid1d(S.n, kThreads, 1024)), dim3(kThreads), 0, s, a.w, a.r, a.v, S.n, a.sq_part);
    const ListShape L = list_shape(X, a.v);
    constexpr int V = VecOf<double>::N;
    if (S.kind == kShadowQ15) {
        if (L.vec) launch_shadow_sweep<ShadowQ15, V>(X, S, a, na, nb, L, stage, s);
        else launch_shadow_sweep<ShadowQ15, 1>(X, S, a, na, nb, L, stage, s);
    } else {
        if (L.vec) launch_shadow_sweep<ShadowF32, V>(X, S, a, na, nb, L, stage, s);
        else launch_shadow_sweep<ShadowF32, 1>(X, S, a, na, nb, L, stage, s);
    }
    hipLaunchKernelGGL(filter_classify_kernel, dim3(1), dim3(kClassifyThreads), 0, s, a.grad, a.groups, a.group_sizes, a.G, a.slot,
                       a.penalty, a.tstar, S.err, S.nrm, S.fp_term(), a.sq_part, filter_norm_parts(S.n), a.sub_scale, a.sub_vec,
                       stage, a.screen_cols, na, a.pen0_cols, nb, L.ns, a.list, a.cap, a.meta_i, a.meta_d);
    launch_sweep_list(X, a.v, a.grad, a.list, a.cap, a.meta_i, a.sub_scale, a.sub_vec, S, a.meta_d, a.meta_i + 1, stage, s);
}

} // namespace ahip
