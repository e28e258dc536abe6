// kernels_cons_wide.hip — box / one-sided constraint objects on groups of 65 .. 128 coefficients, solved on the device.
//
// kernels_cons.hip runs the visit of such a group in one wavefront, "lane i owns component i", with the eigenbasis Q and the dual
// Hessian H both in LDS: 2 d (d|1) doubles, which stops fitting beyond d = 64.  This file is the same visit (same ConsVisitParams,
// same rotation into the eigenbasis, same driver decisions — constraint/utils.hpp:24-243 —, same status mapping and epilogue) for
// 64 < d <= 128 as ONE WORKGROUP OF 256 THREADS (four wavefronts), laid out as follows.
//
//   vectors   thread t < d (the first two waves) owns component t of every d-vector of the driver, in registers.  A sum over the
//             components is a wave sum in each of those two waves (wavered.hpp) and the two results added by every thread in the
//             same order, through a double-buffered LDS slot: one barrier per sum, the value identical in all 256 threads, so every
//             decision of the driver is workgroup-uniform and a visit is bit-reproducible.
//   H         resident in LDS, d x (d|1) doubles (132 096 bytes at d = 128) plus ~10 KB of d-vectors.
//   Q         does not fit beside H: it stays where the solver keeps it (p.V, T, column-major, leading dimension d) and is read
//             through L2, converted on load.  Both products read it coalesced over all four waves:
//               Q x    thread t owns row t & 127 for one half of the columns (t >> 7); the two halves meet in LDS, low half first;
//               Q' x   wave w owns the columns [32 w, 32 w + 32): a lane multiplies rows lane and lane + 64 of eight columns at a
//                      time and reduce8 (wavered.hpp) sums the eight over the lanes in its fixed butterfly order.
//   H build   H = |x| Q diag(b2) Q' + l1 kappa |x| a a' is the O(d^3) part.  H's own LDS space is dead while it is rebuilt, so Q is
//             first staged there as doubles (one coalesced pass), then the 16 x 16 tiles of the LOWER triangle are accumulated in
//             registers with v_mfma_f64_16x16x4f64 (fragment layout of gram_common.hpp: a = Q[16 R + fr][k + fk],
//             b = Q[16 C + fr][k + fk] b2[k + fk]); wave w takes the tile rows w and nt - 1 - w (9 tiles of 36 at d = 128).  After a
//             barrier the elements on and below the diagonal are written together with their mirror images, so H is exactly
//             symmetric (the coordinate descent relies on it).
//   descent   cons_qp on the multipliers is strictly sequential over the coordinates: wave 0 alone runs it, two values of g / mu
//             per lane (components lane and lane + 64), the scalars of a coordinate read with readlane, column i of H from LDS, no
//             workgroup barrier inside; the other waves wait at the one barrier behind it.
//
// Arithmetic is double precision for either value type.  Every loop is bounded by a configuration value or a fixed cap.
#include <algorithm>
#include <stdexcept>
#include <string>
#include "kernels.hpp"
#include "wavered.hpp"

namespace ahip {

namespace {

constexpr int WT = 256;              // threads of the workgroup
constexpr int WD = 128;              // largest group
constexpr int WNT = WD / 16;         // tile rows of H at the most
constexpr double kMaxSolver = 1e100; // configs.hpp:13 max_solver_value

typedef double wd4_t __attribute__((ext_vector_type(4)));

enum ConsRc { CRC_OK = 0, CRC_PN = 1, CRC_QP = 2, CRC_UNEXPECTED = 3 };

// LDS behind H, in doubles
constexpr int OFF_VS = 0, OFF_YS = WD, OFF_PART = 2 * WD, OFF_B2 = 4 * WD, OFF_AL = 5 * WD, OFF_G = 6 * WD, OFF_MU = 7 * WD,
              OFF_VA = 8 * WD, OFF_VB = 9 * WD, OFF_RED = 10 * WD, OFF_END = 10 * WD + 16;

template <class T>
struct WCtx {
    int d, LD, tid, lane, wave;
    bool box, in;
    const T* V;   // Q in global memory, column-major, leading dimension d
    double* H;    // [d][LD], odd leading dimension
    double* sm;   // the vectors behind H (OFF_*)
    int slot;     // which half of the reduction slot the next sum uses
};

// sum over the components (threads t < d hand in theirs, the others anything): wave sums of the two owning waves, added by every
// thread in the same order
template <class T, int N>
__device__ __forceinline__ void bsum(WCtx<T>& c, double (&v)[N]) {
    double* red = c.sm + OFF_RED + c.slot * 8;
    if (c.wave < 2) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const double w = wave_sum64(c.in ? v[e] : 0.0);
            if (c.lane == 0) red[c.wave * 4 + e] = w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = red[e] + red[4 + e];
    c.slot ^= 1;
}
template <class T>
__device__ __forceinline__ double bsum1(WCtx<T>& c, double x) {
    double v[1] = {x};
    bsum(c, v);
    return v[0];
}

// y = Q x, component t to thread t < d
template <class T>
__device__ __forceinline__ double matvec(WCtx<T>& c, double x) {
    const int d = c.d;
    double* vs = c.sm + OFF_VS;
    double* part = c.sm + OFF_PART;
    __syncthreads();
    if (c.tid < WD) vs[c.tid] = c.in ? x : 0.0;
    __syncthreads();
    const int i = c.tid & (WD - 1), h = c.tid >> 7, jh = (d + 1) >> 1;
    const int j0 = h ? jh : 0, j1 = h ? d : jh;
    double acc = 0;
    if (i < d) {
        const T* col = c.V + i + size_t(j0) * d;
#pragma unroll 16
        for (int j = j0; j < j1; ++j, col += d) acc += double(*col) * vs[j];
    }
    part[c.tid] = acc;
    __syncthreads();
    return c.in ? part[c.tid] + part[WD + c.tid] : 0.0;
}
// y = Q' x
template <class T>
__device__ __forceinline__ double matvec_t(WCtx<T>& c, double x) {
    const int d = c.d;
    double* vs = c.sm + OFF_VS;
    double* ys = c.sm + OFF_YS;
    __syncthreads();
    if (c.tid < WD) vs[c.tid] = c.in ? x : 0.0;
    __syncthreads();
    const double x0 = vs[c.lane], x1 = vs[c.lane + 64];
    const bool in1 = c.lane + 64 < d;
#pragma unroll 1
    for (int b = 0; b < 4; ++b) { // (eight columns, sixteen loads, in flight at a time)
        const int jb = c.wave * 32 + b * 8;
        if (jb >= d) break; // (wave-uniform)
        double v[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int j = jb + m;
            v[m] = 0;
            if (j < d) {
                const T* col = c.V + size_t(j) * d;
                v[m] = double(col[c.lane]) * x0;
                if (in1) v[m] += double(col[c.lane + 64]) * x1;
            }
        }
        const double r = reduce8(v, c.lane);
        if (c.lane < 8) ys[jb + c.lane] = r;
    }
    __syncthreads();
    return c.in ? ys[c.tid] : 0.0;
}

// bcd/unconstrained/newton.hpp:35-142 + optimization/newton.hpp:28-65, started at h = 0: x, and the buffers b1 = L + l2,
// b2 = 1 / (b1 h + l1) the dual Hessian reads
template <class T>
__device__ __forceinline__ void group_prox(WCtx<T>& c, double L, double v, double l1, double l2, double& x, double& b1, double& b2) {
    const bool in = c.in;
    const double vn = sqrt(bsum1(c, v * v));
    if (vn <= l1) { x = 0; return; }
    if (l1 <= 0.0) { x = in ? v / (L + l2) : 0.0; return; }
    b1 = L + l2;
    double h = 0, fh, dfh;
    auto step_f = [&](double hh) {
        b2 = in ? 1.0 / (b1 * hh + l1) : 0.0;
        const double z = v * b2, zz = in ? z * z : 0.0;
        double ts[2] = {zz, zz * b1 * b2};
        bsum(c, ts);
        fh = ts[0] - 1.0;
        dfh = -ts[1] * (1.0 + sqrt(ts[0])) / ts[0];
    };
    step_f(h);
    for (int it = 0; fabs(fh) > 1e-12 && it < 100000; ++it) {
        h -= fh / dfh;
        h = fmax(h, 0.0);
        step_f(h);
    }
    x = in ? h * v * b2 : 0.0;
}

// The quadratic sub-problem in mu by coordinate descent (ProxNewton's newton_step), run by WAVE 0 ALONE on the vectors the owners
// left in LDS (OFF_G: gradient of the model at mu, OFF_MU: mu; OFF_VA / OFF_VB: the bounds): lane l carries the components l and
// l + 64.  Box: pinball_full.hpp:92-104 with penalty_neg = lo, penalty_pos = up; one-sided: nnqp_full.hpp:158-164 in the
// coordinates mu * sgn.  Leaves mu in OFF_MU.
template <class T>
__device__ __forceinline__ int cons_qp_wave0(const WCtx<T>& c, double var, double qp_tol, int64_t qp_max_iters) {
    const int d = c.d, LD = c.LD, lane = c.lane;
    const bool in1 = lane + 64 < d, box = c.box;
    double* sm = c.sm;
    const double* H = c.H;
    double g0 = sm[OFF_G + lane], g1 = sm[OFF_G + 64 + lane], mu0 = sm[OFF_MU + lane], mu1 = sm[OFF_MU + 64 + lane];
    const double va0 = sm[OFF_VA + lane], va1 = sm[OFF_VA + 64 + lane], vb0 = sm[OFF_VB + lane], vb1 = sm[OFF_VB + 64 + lane];
    if (!box) { g0 *= va0; g1 *= va1; mu0 *= va0; mu1 *= va1; } // (va = sgn)
    int rc = CRC_QP;
    for (int64_t it = 0; it < qp_max_iters; ++it) {
        double cm = 0;
        // one coordinate: its scalars (read out of lane l of the half that holds it) -> the new value, or no change
        auto visit = [&](int i, double gi, double old, double a_i, double b_i, double& nw) -> bool {
            const double qii = H[i + i * LD];
            if (box) { // lo = -lower >= 0, up = upper >= 0
                const double gi0 = gi + qii * old;
                nw = copysign(fmax(fmax(-a_i - gi0, gi0 - b_i), 0.0), gi0 + a_i) / qii;
            } else {
                const double step = (qii <= 0) ? 0.0 : gi / qii;
                nw = (a_i > 0) ? fmax(old + step, 0.0) : fmin(old + step, 0.0);
            }
            const double del = nw - old;
            if (del == 0) return false;
            cm = fmax(cm, qii * del * del);
            g0 -= del * H[lane + i * LD];
            if (in1) g1 -= del * H[lane + 64 + i * LD];
            return true;
        };
        for (int i = 0; i < 64; ++i) {
            double nw;
            if (visit(i, prdl(g0, i), prdl(mu0, i), prdl(va0, i), prdl(vb0, i), nw) && lane == i) mu0 = nw;
        }
        for (int i = 64; i < d; ++i) {
            const int l = i - 64;
            double nw;
            if (visit(i, prdl(g1, l), prdl(mu1, l), prdl(va1, l), prdl(vb1, l), nw) && lane == l) mu1 = nw;
        }
        if (cm < var * qp_tol) { rc = CRC_OK; break; }
    }
    if (rc == CRC_OK && !box) { mu0 *= va0; mu1 *= va1; }
    sm[OFF_MU + lane] = mu0;
    sm[OFF_MU + 64 + lane] = mu1;
    return rc;
}

// Hessian of the dual objective, constraint/utils.hpp:208-237: H = x_norm Q diag(b2) Q' + l1kn alpha alpha', exactly symmetric.
// b2 and alpha are in LDS (OFF_B2, OFF_AL, zero beyond d).
template <class T>
__device__ __forceinline__ void build_hessian(const WCtx<T>& c, double x_norm, double l1kn) {
    const int d = c.d, LD = c.LD, lane = c.lane;
    double* H = c.H;
    const double* b2s = c.sm + OFF_B2;
    const double* als = c.sm + OFF_AL;
    __syncthreads(); // (the descent's reads of the previous H are over)
    for (int e = c.tid; e < d * d; e += WT) H[(e % d) + (e / d) * LD] = double(c.V[e]);
    __syncthreads();
    const int nt = (d + 15) >> 4, fr = lane & 15, fk = lane >> 4;
    // this wave's tile rows: w and nt - 1 - w (neither when they have crossed, one when they meet)
    const int R0 = c.wave, R1 = nt - 1 - c.wave;
    const bool act0 = R0 <= R1, act1 = R0 < R1;
    wd4_t acc[2][WNT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int C = 0; C < WNT; ++C) acc[s][C] = wd4_t{0, 0, 0, 0};
    if (act0) {
        const int ra0 = R0 * 16 + fr, ra1 = R1 * 16 + fr;
        const int kend = (d + 3) & ~3;
        for (int k = 0; k < kend; k += 4) {
            const int j = k + fk;
            const bool jok = j < d;
            const int jo = (jok ? j : 0) * LD;
            const double wj = jok ? b2s[j] : 0.0;
            const double a0 = (jok && ra0 < d) ? H[ra0 + jo] : 0.0;
            const double a1 = (act1 && jok && ra1 < d) ? H[ra1 + jo] : 0.0;
#pragma unroll
            for (int C = 0; C < WNT; ++C)
                if (C <= R1) { // (wave-uniform; R1 >= R0)
                    const int rb = C * 16 + fr;
                    const double b = (jok && rb < d) ? H[rb + jo] * wj : 0.0;
                    if (C <= R0) acc[0][C] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][C], 0, 0, 0);
                    if (act1) acc[1][C] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][C], 0, 0, 0);
                }
        }
    }
    __syncthreads(); // every wave is done with the staged Q
    if (act0) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int R = s ? R1 : R0;
            const bool live = s == 0 || act1;
#pragma unroll
            for (int C = 0; C < WNT; ++C)
                if (live && C <= R) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = R * 16 + fk + 4 * e, col = C * 16 + fr; // (gram_common.hpp: Mfma<double>::row)
                        if (row < d && col <= row) {
                            const double val = x_norm * acc[s][C][e] + l1kn * (als[row] * als[col]);
                            H[row + col * LD] = val;
                            H[col + row * LD] = val;
                        }
                    }
                }
        }
    }
    __syncthreads();
}

// constraint/utils.hpp:24-243.  Thread t < d: x (in/out, eigen-coordinates), quad, linear, the bounds (box: lo = -lower, up;
// one-sided: sgn, b) and the multiplier mu (in/out).  Returns a ConsRc, the same in every thread.
template <class T>
__device__ __forceinline__ int cons_solve(WCtx<T>& c, double& x, double quad, double linear, double l1, double l2, double va, double vb,
                                          double& mu, const double* cfg) {
    const int d = c.d;
    const bool in = c.in;
    double* sm = c.sm;
    const int max_iters = int(cfg[0]);
    const double tol = cfg[1];
    const int64_t qp_max_iters = int64_t(cfg[2]);
    const double qp_tol = cfg[3], slack = cfg[4];
    auto At = [&](double m) { return c.box ? m : va * m; };      // A' mu (A = I / diag(sgn))
    if (sqrt(bsum1(c, linear * linear)) <= l1) { x = 0; mu = 0; return CRC_OK; } // box :119-123, one-sided :161-165
    const double Qv = matvec(c, linear);
    double grad_prev = 0, grad = 0, mu_prev = 0, b1 = 0, b2 = 0;
    // multipliers that best explain v while the primal stays zero (box :148-166, one-sided :190-208)
    auto min_mu_resid = [&](bool prev_valid_old, bool init) -> double {
        const double keep = mu;
        if (in) {
            if (c.box) {
                const double lb = (va <= 0) ? -kMaxSolver : 0.0, ub = (vb <= 0) ? kMaxSolver : 0.0;
                mu = fmin(fmax(Qv, lb), ub);
            } else {
                const double ub = (vb <= 0) ? kMaxSolver : 0.0;
                mu = fmin(fmax(va * Qv, 0.0), ub);
            }
        }
        const double e = in ? Qv - At(mu) : 0.0;
        const double nsq = bsum1(c, e * e);
        if ((init || prev_valid_old) && nsq > l1 * l1) mu = keep;
        return nsq;
    };
    const bool x_init_zero = !__syncthreads_or(in && x != 0);
    bool prev_valid = false, zero_checked = false;
    double resid_norm_prev = -1;
    if (x_init_zero) { // :78-83
        zero_checked = true;
        if (min_mu_resid(false, true) <= l1 * l1) return CRC_OK;
    }
    for (int iters = 1; iters <= max_iters; ++iters) {
        const double qtam = matvec_t(c, At(mu));
        const double mu_resid = in ? linear - qtam : 0.0;
        const double resid_norm = sqrt(bsum1(c, mu_resid * mu_resid)), resid_norm_sq = resid_norm * resid_norm;
        double x_norm = -1;
        bool in_ellipse = resid_norm <= l1;
        if (!in_ellipse) { // compute_primal :85-93
            group_prox(c, quad, mu_resid, l1, l2, x, b1, b2);
            x_norm = sqrt(bsum1(c, x * x));
            in_ellipse = x_norm <= 0;
            if (l1 <= 0) { b1 = quad + l2; b2 = in ? 1.0 / (b1 * x_norm + l1) : 0.0; } // (newton.hpp:72-75 leaves its buffers unset)
        }
        if (in_ellipse) {
            if (iters == 1 && x_init_zero) { x = 0; return CRC_OK; } // :117-120
            if (prev_valid) { // :124-129
                const double gp = c.box ? grad_prev : grad_prev + vb;
                if (fabs(bsum1(c, (mu - mu_prev) * gp) / double(d)) <= tol) { x = 0; return CRC_OK; }
            }
            if (!zero_checked) { // :136-164
                zero_checked = true;
                const bool prev_valid_old = prev_valid;
                if (!prev_valid_old) {
                    resid_norm_prev = resid_norm;
                    prev_valid = true;
                    mu_prev = mu;
                    grad_prev = c.box ? 0.0 : -vb;
                }
                if (min_mu_resid(prev_valid_old, false) <= l1 * l1) { x = 0; return CRC_OK; }
                if (!prev_valid_old) continue;
            }
            if (!prev_valid || (resid_norm_prev <= l1 * 0.9999) || (resid_norm > l1 * 1.0001)) return CRC_UNEXPECTED;
            const double target = (1 - slack) * l1 + slack * resid_norm_prev; // :177-185
            const double dm = in ? mu - mu_prev : 0.0;
            double ab[2] = {dm * dm, ((c.box ? Qv : va * Qv) - mu) * dm};
            bsum(c, ab);
            const double a = ab[0], bq = ab[1];
            const double cc = resid_norm_sq - target * target;
            const double t_star = (-bq + sqrt(fmax(bq * bq - a * cc, 0.0))) / a;
            const double step = fmin(fmax(1 - t_star, 0.0), 1.0);
            mu = mu_prev + step * (mu - mu_prev);
            continue;
        }
        const double z = matvec(c, x);              // primal_gradient: box x Q^T; one-sided sgn * (x Q^T) - b
        grad = in ? (c.box ? z : va * z - vb) : 0.0;
        bool opt; // hard_optimal
        if (c.box) opt = (grad <= vb && grad >= -va) && (fmax(mu, 0.0) * (grad - vb) == 0) && (fmin(mu, 0.0) * (grad + va) == 0);
        else opt = (grad <= 0) && (mu * grad == 0);
        if (!__syncthreads_or(in && !opt)) return CRC_OK;
        if (prev_valid && fabs(bsum1(c, (mu - mu_prev) * (grad_prev - grad)) / double(d)) <= tol) return CRC_OK;
        resid_norm_prev = resid_norm;
        prev_valid = true;
        mu_prev = mu;
        grad_prev = grad;
        // Hessian of the dual objective, :208-237: x_norm Q diag(b2) Q' + l1 kappa x_norm alpha alpha'
        const double alpha_tmp = in ? x * b2 / x_norm : 0.0;
        const double kappa = 1.0 / bsum1(c, x * b1 * alpha_tmp);
        const double alpha = matvec(c, alpha_tmp);
        const double l1kn = l1 * kappa * x_norm;
        if (c.tid < WD) {
            sm[OFF_B2 + c.tid] = in ? b2 : 0.0;
            sm[OFF_AL + c.tid] = in ? alpha : 0.0;
        }
        build_hessian(c, x_norm, l1kn);
        const double xq = matvec_t(c, x);           // x' S^-1 x by the Woodbury identity, :229-236
        double s3[3] = {x * xq, in ? xq * xq / b2 : 0.0, x * x * b2};
        bsum(c, s3);
        const double xy = s3[0], s1 = s3[1], s2 = s3[2];
        double var = (s1 - (xy * xy) / ((x_norm * x_norm) / (l1 * kappa) + s2)) / x_norm;
        var = fmax(var, 0.0);
        // the descent: the owners hand g and mu to wave 0 and take mu back
        if (c.tid < WD) {
            sm[OFF_G + c.tid] = in ? grad : 0.0;
            sm[OFF_MU + c.tid] = in ? mu : 0.0;
        }
        __syncthreads();
        if (c.wave == 0) {
            const int r = cons_qp_wave0(c, var, qp_tol, qp_max_iters);
            if (c.lane == 0) reinterpret_cast<int*>(sm + OFF_RED + 2 * 8 - 1)[0] = r; // (a word no sum uses: slot 1 holds 7 values)
        }
        __syncthreads();
        const int rc = reinterpret_cast<const int*>(sm + OFF_RED + 2 * 8 - 1)[0];
        if (in) mu = sm[OFF_MU + c.tid];
        if (rc != CRC_OK) return rc;
    }
    return CRC_PN;
}

template <class T>
__global__ __launch_bounds__(WT) void grp_cons_visit_wide_kernel(ConsVisitParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, d = p.q;
    WCtx<T> c;
    c.d = d; c.LD = d | 1; c.tid = tid; c.lane = tid & 63; c.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    c.box = p.native == ADELIE_HIP_NATIVE_BOX;
    c.in = tid < d;
    c.V = p.V;
    c.H = reinterpret_cast<double*>(smem_raw);
    c.sm = c.H + size_t(d) * c.LD;
    c.slot = 0;
    const bool in = c.in;
    const double gk = in ? double(p.gsrc[tid]) : 0.0, ak = in ? double(p.beta[tid]) : 0.0, Ak = in ? double(p.vars[tid]) : 0.0;
    double va = in ? double(p.va[tid]) : 0.0, vb = in ? double(p.vb[tid]) : 0.0;
    if (c.box) { // the class keeps lo = -lower and the bounds clamped to +-max_solver_value (adelie/constraint.py:262-263)
        const double lower = fmax(va, -kMaxSolver), upper = fmin(vb, kMaxSolver);
        va = -lower; vb = upper;
    } else {
        vb = fmin(vb, kMaxSolver);
    }
    if (tid < WD) { // (read by wave 0's descent; the first barrier of the products below publishes them)
        c.sm[OFF_VA + tid] = va;
        c.sm[OFF_VB + tid] = vb;
    }
    double mu = in ? double(p.mu[tid]) : 0.0;
    CdBlkState<T> bs = *p.st;
    if (p.first_of_pass) bs.cm = T(0);
    // into the eigenbasis: g V, beta V  (pin_naive:123-135)
    const double gt = matvec_t(c, gk), a_old_t = matvec_t(c, ak);
    double x = in ? a_old_t : 0.0;
    const double quad = Ak, lin = gt + Ak * a_old_t;
    const int rc = cons_solve(c, x, quad, lin, p.l1, p.l2, va, vb, mu, p.cfg);
    if (!in) x = 0;
    if (in) p.mu[tid] = T(mu);
    int status = bs.status;
    if (rc == CRC_PN) status = CD_CONS_PN;
    else if (rc == CRC_QP) status = c.box ? CD_CONS_QP_BOX : CD_CONS_QP_NNQP;
    else if (rc == CRC_UNEXPECTED) status = CD_CONS_UNEXPECTED;
    int nz = 0, add_at = -1;
    if (rc == CRC_OK) {
        const double dl = in ? x - a_old_t : 0.0;
        double s3[3] = {dl * dl, quad * dl * dl, dl * (2 * gt - dl * quad)};
        bsum(c, s3);
        if (!(sqrt(s3[0]) <= p.dbeta_tol * sqrt(double(d)))) { // :144: the group changed
            const T cmn = T(s3[1] / double(d));
            bs.cm = cmn > bs.cm ? cmn : bs.cm;     // pin_base:100-110
            bs.rsq += T(s3[2]);                     // pin_base:124-134
            const double a_new_d = matvec(c, x);    // back: beta = x V^T  (:156-157)
            const T a_new = T(a_new_d), ak_t = in ? p.beta[tid] : T(0);
            const T dlt = in ? a_new - ak_t : T(0);
            double rsum_l = 0;
            if (in) {
                p.beta[tid] = a_new;
                p.dcol[tid] = p.gram ? int32_t(p.b + tid) : int32_t(p.col0 + tid);
                p.dlt[tid] = dlt;
                if (!p.gram && p.sxm) rsum_l = double(p.sxm[tid]) * double(ak_t - a_new);
            }
            bs.resid_sum += T(bsum1(c, rsum_l));
            bs.n_updates += 1;
            nz = d;
            if (p.mark && !p.is_active[p.ss]) { // add_active_set, pin_naive:294-304
                if (bs.active_size >= p.max_active_size) status = CD_MAX_ACTIVE;
                else add_at = bs.active_size;
                if (status != CD_MAX_ACTIVE) bs.active_size += 1;
            }
        }
    }
    __syncthreads(); // (every thread has read is_active: thread 0 may write it)
    bs.nz = nz;
    bs.status = status;
    if (tid == 0) {
        if (add_at >= 0) {
            p.is_active[p.ss] = 1;
            p.active_set[add_at] = p.ss;
        }
        *p.st = bs;
        if (p.n_visits) p.n_visits[0] += 1;
        if (p.host_st && p.report_seq) {
            *p.host_st = bs;
            __threadfence_system();
            __hip_atomic_store(p.host_seq, p.report_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

} // namespace

size_t cons_visit_wide_lds(int q) { return (size_t(q) * size_t(q | 1) + size_t(OFF_END)) * sizeof(double); }

template <class T>
void launch_grp_cons_visit_wide(const ConsVisitParams<T>& p, hipStream_t s) {
    if (p.q <= 64 || p.q > WD) throw std::runtime_error("adelie_hip: the wide constraint visit takes groups of 65 to 128 coefficients.");
    if (!p.V) throw std::runtime_error("adelie_hip: the wide constraint visit needs the group's eigenbasis.");
    // the dynamic LDS of the largest group, against what this device gives a workgroup
    static const int lds_limit = [] {
        int dev = 0, limit = 0, optin = 0; // (the larger of the plain and the opt-in figure: hipFuncSetAttribute below opts in)
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) limit = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) optin = 0;
        (void)hipGetLastError();
        return std::max(limit, optin);
    }();
    const size_t need = cons_visit_wide_lds(p.q);
    if (size_t(lds_limit) < need)
        throw std::runtime_error("adelie_hip: grp_cons_visit_wide_kernel needs " + std::to_string(need) + " bytes of LDS, the device gives a workgroup " +
                                 std::to_string(lds_limit) + ".");
    static const bool raised = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(grp_cons_visit_wide_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  int(std::min(cons_visit_wide_lds(WD), size_t(lds_limit))));
        return true;
    }();
    (void)raised;
    (void)hipGetLastError();
    hipLaunchKernelGGL((grp_cons_visit_wide_kernel<T>), dim3(1), dim3(WT), need, s, p);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        throw std::runtime_error(std::string("adelie_hip: grp_cons_visit_wide_kernel launch refused: ") + hipGetErrorString(e));
}

template void launch_grp_cons_visit_wide<double>(const ConsVisitParams<double>&, hipStream_t);
template void launch_grp_cons_visit_wide<float>(const ConsVisitParams<float>&, hipStream_t);

} // namespace ahip
