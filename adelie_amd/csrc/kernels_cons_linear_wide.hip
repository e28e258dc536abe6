// kernels_cons_linear_wide.hip — `linear` constraint objects  lower <= A x <= upper  (A: m x d, 1 <= m <= 64 rows) on groups of
// 65 <= d <= 128 coefficients, solved on the device.
//
// kernels_cons_linear.hip runs the visit of such an object in one wavefront: lane i carries component i of every d-vector and all
// tiles of B = A V accumulate in that wave's registers, which stops at d = 64 (the 4 x 8 accumulators of B alone would take 256
// VGPRs).  This file is the same visit (same ConsVisitParams, same driver decisions — constraint/utils.hpp:24-243 with the hooks of
// constraint_linear.ipp:232-497 —, same status mapping, epilogue and pass report) as ONE WORKGROUP OF 256 THREADS (four wavefronts):
//
//   vectors   a d-vector is two components per lane (lane l carries l and l + 64, zero beyond d), an m-vector one component per
//             lane, the order / screen / active lists of the bounded least squares are register lists with 64-bit masks.  EVERY
//             WAVE CARRIES THE WHOLE STATE and runs the whole driver on it: the four copies see the same numbers and execute the
//             same instructions, so every decision is workgroup-uniform by construction, every barrier stands at one program point
//             for all four waves, and nothing has to be broadcast.  The strictly sequential parts (the pinball coordinate descent,
//             the sweeps of the bounded least squares) have no barrier inside; they run in the four SIMDs side by side, which costs
//             LDS reads (a column of H or a row of B per step) and no time.  Only wave 0 writes results to global memory.
//   wide work is split over the 256 threads with a fixed split, the parts meet in a double-buffered LDS slot (one barrier per
//             product) and every wave adds them in the same order:
//               B'mu   thread t: output column t & 127 over one half of the rows          B x    wave w: a quarter of the columns
//               V x    thread t: row t & 127 over one half of the columns (coalesced)      V'x    wave w: 32 columns, reduce8
//   B = A V   A is staged in B's own LDS space (one coalesced pass), then wave w accumulates the tile columns 2 w and 2 w + 1 (up to
//             4 x 2 tiles of v_mfma_f64_16x16x4f64, 32 accumulator doubles a lane) from LDS fragments of A and fragments of V read
//             through L2, converted on load: A and V are each read once.  After a barrier B replaces A, column by column with an
//             odd leading dimension.  V (up to 128 KB as doubles) is never stored; V'x of the pinball stopping rule reads it
//             through L2 once per Newton iteration.
//   H         H = |x| B diag(b2) B' + (l1 kappa |x|)(B a)(B a)', rebuilt once per Newton iteration: the up to 10 tiles of the lower
//             triangle go round the four waves (tile t to wave t & 3: 3, 3, 2, 2 tiles of depth d), both operands from LDS; every
//             element is written together with its mirror image, so H is exactly symmetric.
//   LDS       B d x (m|1) + H m x (m|1) + 6 KB of slots: 105 984 bytes at m = 64, d = 128.
//
// The same file holds the `linear` part of abs_grad for such groups: |grad - regul beta - A'mu| for a screened group, solve_zero
// (constraint_linear.ipp:520-603) for the others — the same bounded least squares with A staged in place of B.
//
// Arithmetic is double precision for either value type.  Every sum has one fixed order; there are no atomics.  Every loop is
// bounded by a configuration value or by m.
#include <algorithm>
#include <stdexcept>
#include <string>
#include "kernels.hpp"
#include "wavered.hpp"
#include "cons_common.hpp"

namespace ahip {

namespace {

constexpr int XT = 256;              // threads of the workgroup
constexpr int XD = 128;              // largest group
constexpr int XM = 64;               // most rows
constexpr int XMT = XM / 16;         // tile rows of B and of H at the most
constexpr double kMaxSolver = 1e100; // configs.hpp:13 max_solver_value
constexpr double kEps = 1e-16;       // constraint_linear.hpp:40: a multiplier at or below it counts as zero

typedef double xd4_t __attribute__((ext_vector_type(4)));

// components lane and lane + 64 of a d-vector; zero beyond d
struct V2 {
    double a, b;
};
__device__ __forceinline__ V2 operator+(V2 x, V2 y) { return V2{x.a + y.a, x.b + y.b}; }
__device__ __forceinline__ V2 operator-(V2 x, V2 y) { return V2{x.a - y.a, x.b - y.b}; }
__device__ __forceinline__ V2 operator*(V2 x, V2 y) { return V2{x.a * y.a, x.b * y.b}; }
__device__ __forceinline__ V2 operator*(double s, V2 x) { return V2{s * x.a, s * x.b}; }

__device__ __forceinline__ double wsum(double x) { return wave_sum64(x); }
__device__ __forceinline__ double dsum(V2 x) { return wave_sum64(x.a + x.b); }
__device__ __forceinline__ double rl(double x, int l) { return prdl(x, l); }
__device__ __forceinline__ int rli(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ double rl2(V2 x, int j) { return j < 64 ? prdl(x.a, j) : prdl(x.b, j - 64); } // (j wave-uniform)
__device__ __forceinline__ bool bit(uint64_t m, int k) { return (m >> k) & 1ull; }

constexpr int OFF_PART = 0, OFF_VS = 2 * XT, OFF_VS2 = 2 * XT + XD, OFF_B = 2 * XT + 2 * XD; // LDS, in doubles

struct XCtx {
    int m, d, tid, lane, wave, LDB, LDH;
    bool in1, in_m; // lane + 64 < d; lane < m
    double* part;   // [2][XT] where the parts of a product meet, double-buffered
    double* vs;     // [XD] b2 for the build of H
    double* vs2;    // [XD] B a for the build of H
    double* B;      // [d][LDB]: B[k + j LDB], rows k < m, columns j < d
    double* H;      // [m][LDH] dual Hessian
    int slot;       // which half of `part` the next product uses
};
__device__ __forceinline__ XCtx make_ctx(char* smem, int m, int d, int tid) {
    XCtx c;
    c.m = m; c.d = d; c.tid = tid; c.lane = tid & 63; c.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    c.LDB = m | 1; c.LDH = m | 1;
    c.in1 = c.lane + 64 < d; c.in_m = c.lane < m;
    double* sm = reinterpret_cast<double*>(smem);
    c.part = sm + OFF_PART; c.vs = sm + OFF_VS; c.vs2 = sm + OFF_VS2; c.B = sm + OFF_B;
    c.H = c.B + size_t(d) * c.LDB;
    c.slot = 0;
    return c;
}
// the slot of the next product: a wave may be writing the other half while a slower one still reads this one's predecessor
__device__ __forceinline__ double* next_part(XCtx& c) {
    double* p = c.part + c.slot * XT;
    c.slot ^= 1;
    return p;
}

// a list of distinct indices below 64 in the order they were added: lane t carries entry t
struct OList {
    int v = 0, n = 0;
    uint64_t mask = 0;
};
__device__ __forceinline__ void ol_push(OList& o, int k, int lane) {
    if (k < 0 || k >= XM || bit(o.mask, k)) return;
    if (lane == o.n) o.v = k;
    o.n += 1;
    o.mask |= 1ull << k;
}
__device__ __forceinline__ OList ol_filter(const OList& o, uint64_t keep, int lane) {
    OList r;
    for (int t = 0; t < o.n; ++t) {
        const int k = rli(o.v, t);
        if (bit(keep, k)) ol_push(r, k, lane);
    }
    return r;
}
// mu_to_sparse, constraint_linear.ipp:94-108: the entries that are still non-zero in their old order, then the new non-zeros
__device__ __forceinline__ OList active_order(const XCtx& c, const OList& o, double mu) {
    const uint64_t nz = __ballot(c.in_m && fabs(mu) > kEps);
    OList r = ol_filter(o, nz, c.lane);
    for (uint64_t rem = nz & ~o.mask; rem; rem &= rem - 1) ol_push(r, __builtin_ctzll(rem), c.lane);
    return r;
}

// B'mu: component j = sum_k B[k][j] mu_k.  Thread t: column t & 127 over the rows of half t >> 7, low half first.
__device__ __forceinline__ V2 bt_mul(XCtx& c, double mu) {
    double* part = next_part(c);
    const int j = c.tid & (XD - 1), mh = (c.m + 1) >> 1, h = c.wave >> 1;
    const int k0 = h ? mh : 0, k1 = h ? c.m : mh;
    const bool jok = j < c.d;
    const double* col = c.B + (jok ? j : 0) * c.LDB;
    double acc = 0;
    for (int k = k0; k < k1; ++k) acc += (jok ? col[k] : 0.0) * rl(mu, k);
    part[c.tid] = acc;
    __syncthreads();
    return V2{part[c.lane] + part[XD + c.lane], c.in1 ? part[64 + c.lane] + part[XD + 64 + c.lane] : 0.0};
}
// B x: row k = sum_j B[k][j] x_j.  Wave w: the columns of quarter w, the quarters added in pairs.
__device__ __forceinline__ double b_mul(XCtx& c, V2 x) {
    double* part = next_part(c);
    const int dq = (c.d + 3) >> 2, j0 = c.wave * dq, j1 = min(j0 + dq, c.d);
    double acc = 0;
    for (int j = j0; j < j1; ++j) acc += (c.in_m ? c.B[c.lane + j * c.LDB] : 0.0) * rl2(x, j);
    part[c.tid] = acc;
    __syncthreads();
    return (part[c.lane] + part[64 + c.lane]) + (part[128 + c.lane] + part[192 + c.lane]);
}
// V x: row i = sum_j V[i][j] x_j (V column-major, leading dimension d).  Thread t: row t & 127 over one half of the columns.
template <class T>
__device__ __forceinline__ V2 v_mul(XCtx& c, const T* __restrict__ V, V2 x) {
    double* part = next_part(c);
    const int d = c.d, i = c.tid & (XD - 1), jh = (d + 1) >> 1, h = c.wave >> 1;
    const int j0 = h ? jh : 0, j1 = h ? d : jh;
    const bool iok = i < d;
    const T* col = V + (iok ? i : 0) + size_t(j0) * d;
    double acc = 0;
    for (int j = j0; j < j1; ++j, col += d) acc += (iok ? double(*col) : 0.0) * rl2(x, j);
    part[c.tid] = acc;
    __syncthreads();
    return V2{part[c.lane] + part[XD + c.lane], c.in1 ? part[64 + c.lane] + part[XD + 64 + c.lane] : 0.0};
}
// V'x: column j = sum_i V[i][j] x_i.  Wave w: the columns [32 w, 32 w + 32), eight at a time through reduce8.
template <class T>
__device__ __forceinline__ V2 vt_mul(XCtx& c, const T* __restrict__ V, V2 x) {
    double* ys = next_part(c);
    const int d = c.d;
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
        const int jb = c.wave * 32 + b * 8;
        if (jb >= d) break; // (wave-uniform)
        double v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = jb + e;
            v[e] = 0;
            if (j < d) {
                const T* col = V + size_t(j) * d;
                v[e] = double(col[c.lane]) * x.a;
                if (c.in1) v[e] += double(col[c.lane + 64]) * x.b;
            }
        }
        const double r = reduce8(v, c.lane);
        if (c.lane < 8) ys[jb + c.lane] = r;
    }
    __syncthreads();
    return V2{ys[c.lane], c.in1 ? ys[c.lane + 64] : 0.0};
}

// A (m x d row-major doubles) into B's space, as B is laid out
__device__ __forceinline__ void stage_A(const XCtx& c, const double* __restrict__ A) {
    const int d = c.d, total = c.m * d;
    for (int e = c.tid; e < total; e += XT) c.B[(e / d) + (e % d) * c.LDB] = A[e];
    __syncthreads();
}

// B = A V with v_mfma_f64_16x16x4f64: fragment a = A[16 R + fr][i0 + fk] from the staged copy, b = V[i0 + fk][16 C + fr]; acc e is
// row 16 R + fk + 4 e, column 16 C + fr.  Wave w: the tile columns 2 w and 2 w + 1 over every tile row.
template <class T>
__device__ __forceinline__ void build_B(const XCtx& c, const double* __restrict__ A, const T* __restrict__ V) {
    const int m = c.m, d = c.d, fr = c.lane & 15, fk = c.lane >> 4, LDB = c.LDB;
    const int mt = (m + 15) >> 4, dt = (d + 15) >> 4, C0 = 2 * c.wave;
    stage_A(c, A);
    xd4_t acc[XMT][2];
#pragma unroll
    for (int R = 0; R < XMT; ++R)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc[R][s] = xd4_t{0, 0, 0, 0};
    if (C0 < dt) { // (wave-uniform)
        for (int i0 = 0; i0 < d; i0 += 4) {
            const int i = i0 + fk;
            const bool iok = i < d;
            double a[XMT], b[2];
#pragma unroll
            for (int R = 0; R < XMT; ++R) {
                const int r = R * 16 + fr;
                a[R] = (iok && r < m) ? c.B[r + i * LDB] : 0.0;
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int col = (C0 + s) * 16 + fr;
                b[s] = (iok && col < d) ? double(V[size_t(i) + size_t(col) * d]) : 0.0;
            }
#pragma unroll
            for (int R = 0; R < XMT; ++R)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    if (R < mt && C0 + s < dt) acc[R][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[R], b[s], acc[R][s], 0, 0, 0);
        }
    }
    __syncthreads(); // every wave is done with the staged A
#pragma unroll
    for (int R = 0; R < XMT; ++R)
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (R < mt && C0 + s < dt) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = R * 16 + fk + 4 * e, col = (C0 + s) * 16 + fr;
                    if (row < m && col < d) c.B[row + col * LDB] = acc[R][s][e];
                }
            }
    __syncthreads();
}

// H = x_norm B diag(b2) B' + l1kn (B a)(B a)', exactly symmetric.  b2 (zero beyond d) is in vs, B a (rows < m) in vs2.  Tile t of
// the lower triangle, counted row by row, belongs to wave t & 3.
__device__ __forceinline__ void build_H(const XCtx& c, double x_norm, double l1kn) {
    const int m = c.m, d = c.d, fr = c.lane & 15, fk = c.lane >> 4, LDB = c.LDB;
    const int mt = (m + 15) >> 4;
    int TR[3], TC[3];
    bool on[3];
    xd4_t acc[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int t = c.wave + 4 * s;
        TR[s] = t >= 6 ? 3 : (t >= 3 ? 2 : (t >= 1 ? 1 : 0));
        TC[s] = t - TR[s] * (TR[s] + 1) / 2;
        on[s] = t < 10 && TR[s] < mt; // (wave-uniform)
        acc[s] = xd4_t{0, 0, 0, 0};
    }
    for (int j0 = 0; j0 < d; j0 += 4) {
        const int j = j0 + fk;
        const bool jok = j < d;
        const double wj = jok ? c.vs[j] : 0.0;
#pragma unroll
        for (int s = 0; s < 3; ++s)
            if (on[s]) {
                const int ra = TR[s] * 16 + fr, rb = TC[s] * 16 + fr;
                const double a = (jok && ra < m) ? c.B[ra + j * LDB] : 0.0;
                const double b = (jok && rb < m) ? c.B[rb + j * LDB] * wj : 0.0;
                acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[s], 0, 0, 0);
            }
    }
    __syncthreads(); // (the descents' reads of the previous H are over)
#pragma unroll
    for (int s = 0; s < 3; ++s)
        if (on[s]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = TR[s] * 16 + fk + 4 * e, col = TC[s] * 16 + fr;
                if (row < m && col <= row) {
                    const double val = x_norm * acc[s][e] + l1kn * (c.vs2[row] * c.vs2[col]);
                    c.H[row + col * c.LDH] = val;
                    c.H[col + row * c.LDH] = val;
                }
            }
        }
    __syncthreads();
}

// bcd/unconstrained/newton.hpp:35-142 + optimization/newton.hpp:28-65, started at h = 0 (cons_common.hpp's group_prox on two
// components a lane): x, and the buffers b1 = L + l2, b2 = 1 / (b1 h + l1) the dual Hessian reads
__device__ __forceinline__ void group_prox2(const XCtx& c, V2 L, V2 v, double l1, double l2, V2& x, V2& b1, V2& b2) {
    const double vn = sqrt(dsum(v * v));
    if (vn <= l1) { x = V2{0, 0}; return; }
    if (l1 <= 0.0) { x = V2{v.a / (L.a + l2), c.in1 ? v.b / (L.b + l2) : 0.0}; return; }
    b1 = V2{L.a + l2, L.b + l2};
    double h = 0, fh, dfh;
    auto step_f = [&](double hh) {
        b2 = V2{1.0 / (b1.a * hh + l1), c.in1 ? 1.0 / (b1.b * hh + l1) : 0.0};
        const V2 z = v * b2, zz = z * z;
        const double t = dsum(zz);
        fh = t - 1.0;
        const double s = dsum(zz * b1 * b2);
        dfh = -s * (1.0 + sqrt(t)) / t;
    };
    step_f(h);
    for (int it = 0; fabs(fh) > 1e-12 && it < 100000; ++it) {
        h -= fh / dfh;
        h = fmax(h, 0.0);
        step_f(h);
    }
    x = h * (v * b2);
}

// The pinball-penalised quadratic model by coordinate descent (pinball_full.hpp:84-118): g = its gradient at mu (kept current),
// lo_pen = -lower, up_pen = upper, var * tol the stopping threshold.  No barrier inside: each wave runs it on its own copy.
__device__ __forceinline__ int lin_pinball(const XCtx& c, double& mu, double g, double lo_pen, double up_pen, double var, double tol,
                                           int64_t max_iters) {
    const int m = c.m;
    for (int64_t it = 0; it < max_iters; ++it) {
        double worst = 0;
        for (int i = 0; i < m; ++i) {
            const double h = c.H[i + i * c.LDH];
            if (h <= 0) continue;
            const double old = rl(mu, i), lo_i = rl(lo_pen, i), up_i = rl(up_pen, i);
            const double g0 = rl(g, i) + h * old;
            const double nw = copysign(fmax(fmax(-lo_i - g0, g0 - up_i), 0.0), g0 + lo_i) / h;
            const double dl = nw - old;
            if (dl == 0) continue;
            if (c.lane == i) mu = nw;
            worst = fmax(worst, h * dl * dl);
            if (c.in_m) g -= dl * c.H[c.lane + i * c.LDH];
        }
        if (worst < var * tol) return CRC_OK;
    }
    return CRC_QP;
}

struct BvlsCfg {
    int64_t max_iters;
    double tol;
};

// min |target - B'beta|^2 over slo <= beta <= shi by the reference's warm-started coordinate descent with a screen and an active
// set (solver_bvls.hpp): `target` and the residual as d-vectors, beta (in: the warm start; out: the fit, zero off the kept set), the
// bounds and the row variances per lane k < m; `order` in: the warm start's list, out: the kept multipliers in the order they
// entered.  can_stop: the early stop at 2 loss <= l1sq (the fit inside solve); without it the descent runs to the end.
__device__ __forceinline__ int lin_bvls(XCtx& c, V2 target, double& beta, OList& order, double va, double slo, double shi, double y_var,
                                        bool can_stop, double l1sq, const BvlsCfg& cfg, double& loss_out) {
    const int m = c.m, d = c.d, lane = c.lane;
    const bool in_m = c.in_m, in1 = c.in1;
    V2 resid = target - bt_mul(c, beta);
    double loss = 0.5 * dsum(resid * resid);
    OList screen = order, active = order;
    const int kappa = m < d ? m : d;
    const double thr = cfg.tol * y_var;
    int64_t iters = 0;
    auto good = [&]() { return can_stop && 2 * loss <= l1sq; };
    auto sweep = [&](const OList L, bool add_active) -> double {
        double worst = 0;
        for (int t = 0; t < L.n; ++t) {
            if (good()) return worst;
            const int k = rli(L.v, t);
            const double vk = rl(va, k), old = rl(beta, k);
            const V2 bk{c.B[k + lane * c.LDB], in1 ? c.B[k + (lane + 64) * c.LDB] : 0.0};
            const double gk = dsum(bk * resid);
            const double nw = fmin(fmax(old + (vk <= 0 ? 0.0 : gk / vk), rl(slo, k)), rl(shi, k));
            if (nw == old) continue;
            if (lane == k) beta = nw;
            const double dl = nw - old, sds = vk * dl * dl;
            worst = fmax(worst, sds);
            loss -= dl * gk - 0.5 * sds;
            resid = resid - dl * bk;
            if (add_active) ol_push(active, k, lane);
        }
        return worst;
    };
    auto prune = [&]() { active = ol_filter(active, __ballot(in_m && slo < beta && beta < shi), lane); };
    auto fit = [&]() -> int {
        for (;;) {
            ++iters;
            double worst = sweep(screen, true);
            if (iters >= cfg.max_iters) return CRC_BVLS;
            if (worst <= thr || good()) { prune(); return CRC_OK; }
            for (;;) {
                ++iters;
                worst = sweep(active, false);
                if (iters >= cfg.max_iters) return CRC_BVLS;
                if (worst <= thr) break;
            }
            prune();
        }
    };
    int n_kkt = 0;
    int pos = lane; // by_violation as positions: lane k stands at place pos in the list sorted so far
    for (;;) {
        const double before = loss;
        if (const int rc = fit(); rc != CRC_OK) return rc;
        if (good()) break;
        if (n_kkt > 0 && fabs(loss - before) < 1e-6 * fabs(y_var)) break;
        ++n_kkt;
        const double g = b_mul(c, resid);
        const double viol = in_m ? fmax(g, 0.0) * (beta < shi ? 1.0 : 0.0) - fmin(g, 0.0) * (beta > slo ? 1.0 : 0.0) : -1.0;
        int rank = 0; // stable sort by falling violation of the list as the last round left it
        for (int k2 = 0; k2 < m; ++k2) {
            const double v2 = rl(viol, k2);
            const int p2 = rli(pos, k2);
            rank += (v2 > viol || (v2 == viol && p2 < pos)) ? 1 : 0;
        }
        pos = rank;
        const int n_old = screen.n;
        bool passed = true;
        for (int r = 0; r < m; ++r) {
            const uint64_t at = __ballot(in_m && pos == r);
            if (!at) continue;
            const int k = __builtin_ctzll(at);
            if (bit(screen.mask, k) || !(rl(viol, k) > 0)) continue;
            passed = false;
            if (screen.n >= n_old + kappa) break;
            ol_push(screen, k, lane);
        }
        if (passed) break;
    }
    const uint64_t keep = __ballot(in_m && bit(active.mask, lane) && fabs(beta) > kEps);
    order = ol_filter(active, keep, lane);
    if (!bit(keep, lane)) beta = 0;
    loss_out = loss;
    return CRC_OK;
}

struct LinCfg {
    int max_iters;
    double tol;
    BvlsCfg nnls;
    int64_t qp_max_iters;
    double qp_tol, slack;
};

// constraint/utils.hpp:24-243 with the hooks of ConstraintLinear, in eigen-coordinates.  d-vectors: x (in/out), quad, v (the
// linear term); lane k < m: lo_pen = -lower, up_pen = upper, the row variances and mu (in/out).  `ord`: the multipliers' order.
template <class T>
__device__ __forceinline__ int lin_solve(XCtx& c, const T* __restrict__ V, V2& x, V2 quad, V2 v, double l1, double l2, double lo_pen,
                                         double up_pen, double avars, double& mu, OList& ord, const LinCfg& cfg) {
    const int d = c.d, lane = c.lane;
    const bool in1 = c.in1, in_m = c.in_m;
    const V2 zero{0, 0};
    const double vv = dsum(v * v), l1sq = l1 * l1;
    if (sqrt(vv) <= l1) { x = zero; mu = 0; ord = OList(); return CRC_OK; }
    // a negative multiplier needs an active lower bound at 0, a positive one an active upper bound (constraint_linear.ipp:286-293)
    const double slo = (-lo_pen >= 0) ? -kMaxSolver : 0.0, shi = (up_pen <= 0) ? kMaxSolver : 0.0;
    // multipliers that best explain v while the primal stays zero (:283-349); keeps the old ones when even those do not
    auto nearest_at_zero = [&](bool may_restore, double& gap) -> int {
        ord = active_order(c, ord, mu);
        V2 e = v - bt_mul(c, mu);
        gap = dsum(e * e);
        if (gap <= l1sq) return CRC_OK; // :281-283
        double cand = mu, loss = 0;
        OList oc = ord;
        if (const int rc = lin_bvls(c, v, cand, oc, avars, slo, shi, vv, true, l1sq, cfg.nnls, loss); rc != CRC_OK) return rc;
        e = v - bt_mul(c, cand);
        gap = dsum(e * e);
        if (may_restore && gap > l1sq) return CRC_OK;
        mu = cand;
        ord = oc;
        return CRC_OK;
    };
    const bool x_zero_start = (__ballot(x.a != 0) | __ballot(in1 && x.b != 0)) == 0ull;
    bool have_prev = false, zero_checked = false;
    V2 btmu_prev = zero, x_prev = zero, b1 = zero, b2 = zero;
    double mu_prev = 0, rn_prev = -1, gap = 0;
    OList ord_prev;
    if (x_zero_start) {
        zero_checked = true;
        if (const int rc = nearest_at_zero(true, gap); rc != CRC_OK) return rc;
        if (gap <= l1sq) { x = zero; return CRC_OK; }
    }
    for (int it = 1; it <= cfg.max_iters; ++it) {
        const V2 btmu = bt_mul(c, mu);
        const V2 resid = v - btmu;
        const double rn = sqrt(dsum(resid * resid));
        bool inside = rn <= l1;
        double xn = -1;
        if (!inside) {
            group_prox2(c, quad, resid, l1, l2, x, b1, b2);
            xn = sqrt(dsum(x * x));
            inside = xn <= 0;
            if (l1 <= 0) { // (newton.hpp:72-75 leaves its buffers unset)
                b1 = V2{quad.a + l2, quad.b + l2};
                b2 = V2{1.0 / (b1.a * xn + l1), in1 ? 1.0 / (b1.b * xn + l1) : 0.0};
            }
        }
        if (inside) {
            if (it == 1 && x_zero_start) { x = zero; return CRC_OK; }
            if (have_prev && fabs(dsum((btmu - btmu_prev) * x_prev) / double(d)) <= cfg.tol) { x = zero; return CRC_OK; }
            if (!zero_checked) {
                zero_checked = true;
                const bool had_prev = have_prev;
                if (!had_prev) {
                    rn_prev = rn; have_prev = true;
                    mu_prev = mu; btmu_prev = btmu; x_prev = zero;
                    ord_prev = ord;
                }
                if (const int rc = nearest_at_zero(had_prev, gap); rc != CRC_OK) return rc;
                if (gap <= l1sq) { x = zero; return CRC_OK; }
                if (!had_prev) continue;
            }
            if (!have_prev || rn_prev <= l1 * 0.9999 || rn > l1 * 1.0001) return CRC_UNEXPECTED;
            // back towards the ellipse |v - B'mu| = l1 along mu_prev -> mu (constraint_linear.ipp:351-382)
            const double target = (1 - cfg.slack) * l1 + cfg.slack * rn_prev;
            const V2 dbt = btmu - btmu_prev;
            const double a = dsum(dbt * dbt), b = dsum(resid * dbt), cc = rn * rn - target * target;
            const double t_star = (-b + sqrt(fmax(b * b - a * cc, 0.0))) / a;
            mu = mu_prev + fmin(fmax(1 - t_star, 0.0), 1.0) * (mu - mu_prev);
            for (int t = 0; t < ord_prev.n; ++t) ol_push(ord, rli(ord_prev.v, t), lane); // the current multipliers first, then the previous ones
            continue;
        }
        if (have_prev && fabs(dsum((btmu - btmu_prev) * (x_prev - x)) / double(d)) <= cfg.tol) return CRC_OK;
        rn_prev = rn; have_prev = true;
        mu_prev = mu; btmu_prev = btmu; x_prev = x;
        ord_prev = ord;
        // the dual Hessian and the variance scale of the descent's stopping rule (Woodbury), constraint/utils.hpp:208-237
        const V2 a_t{x.a * b2.a / xn, x.b * b2.b / xn};
        const double kappa = 1.0 / dsum(x * b1 * a_t);
        const double ba = b_mul(c, a_t);
        if (c.wave == 0) { // (the last build's reads of the two slots ended at its barriers)
            c.vs[lane] = b2.a; c.vs[lane + 64] = b2.b;
            c.vs2[lane] = in_m ? ba : 0.0;
        }
        __syncthreads();
        build_H(c, xn, l1 * kappa * xn);
        const V2 xq = vt_mul(c, V, x); // V'x, the one product B does not give
        const double xy = dsum(x * xq), s1 = dsum(V2{xq.a * xq.a / b2.a, in1 ? xq.b * xq.b / b2.b : 0.0}), s2 = dsum(x * x * b2);
        const double var = fmax((s1 - (xy * xy) / ((xn * xn) / (l1 * kappa) + s2)) / xn, 0.0);
        const double g = b_mul(c, x);
        ord = active_order(c, ord, mu);
        if (const int rc = lin_pinball(c, mu, g, lo_pen, up_pen, var, cfg.qp_tol, cfg.qp_max_iters); rc != CRC_OK) return rc;
        ord = active_order(c, ord, mu);
    }
    return CRC_PN;
}

__device__ __forceinline__ OList load_order(const int32_t* order, int n, int m, int lane) {
    OList o;
    for (int t = 0; t < n && t < m; ++t) {
        const int k = order[t];
        if (k < m) ol_push(o, k, lane);
    }
    return o;
}
__device__ __forceinline__ void store_order(const OList& o, int32_t* order, int32_t* norder, int m, int lane) {
    if (lane < m) order[lane] = lane < o.n ? o.v : -1;
    if (lane == 0) norder[0] = o.n;
}

template <class T>
__global__ __launch_bounds__(XT) void grp_cons_linear_wide_visit_kernel(ConsVisitParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int d = p.q, m = p.m;
    XCtx c = make_ctx(smem_raw, m, d, threadIdx.x);
    const int lane = c.lane, l1i = lane + 64;
    const bool in1 = c.in1, in_m = c.in_m, writer = c.wave == 0;
    const T* V = p.V;
    // everything the visit reads and later writes is read before the first barrier (only wave 0 writes, after the last one)
    const T ak0 = p.beta[lane], ak1 = in1 ? p.beta[l1i] : T(0);
    const V2 gk{double(p.gsrc[lane]), in1 ? double(p.gsrc[l1i]) : 0.0}, ak{double(ak0), double(ak1)};
    const V2 quad{double(p.vars[lane]), in1 ? double(p.vars[l1i]) : 0.0};
    // the class keeps the bounds clamped to +-max_solver_value
    const double lo_pen = in_m ? -fmax(p.llo[lane], -kMaxSolver) : 0.0, up_pen = in_m ? fmin(p.lup[lane], kMaxSolver) : 0.0;
    const double avars = in_m ? p.lvars[lane] : 0.0;
    double mu = in_m ? double(p.mu[lane]) : 0.0;
    OList ord = load_order(p.lorder, p.lnorder[0], m, lane);
    CdBlkState<T> bs = *p.st;
    const bool was_active = p.mark && p.is_active[p.ss];
    if (p.first_of_pass) bs.cm = T(0);
    build_B<T>(c, p.lA, V);
    // into the eigenbasis: g V, beta V  (pin_naive:123-135)
    const V2 gt = vt_mul(c, V, gk), a_old_t = vt_mul(c, V, ak);
    V2 x = a_old_t;
    const V2 lin = gt + quad * a_old_t;
    LinCfg cfg;
    cfg.max_iters = int(p.cfg[0]); cfg.tol = p.cfg[1]; cfg.qp_max_iters = int64_t(p.cfg[2]); cfg.qp_tol = p.cfg[3]; cfg.slack = p.cfg[4];
    cfg.nnls.max_iters = int64_t(p.lcfg[0]); cfg.nnls.tol = p.lcfg[1];
    const int rc = lin_solve<T>(c, V, x, quad, lin, p.l1, p.l2, lo_pen, up_pen, avars, mu, ord, cfg);
    const T mu_t = T(mu); // what the object holds, and the order brought up to date with it (ConstraintLinear::solve's last step)
    ord = active_order(c, ord, double(mu_t));
    if (writer) {
        if (in_m) p.mu[lane] = mu_t;
        store_order(ord, p.lorder, p.lnorder, m, lane);
    }
    int status = bs.status;
    if (rc == CRC_PN) status = CD_CONS_PN;
    else if (rc == CRC_QP) status = CD_CONS_QP_BOX;
    else if (rc == CRC_BVLS) status = CD_CONS_BVLS;
    else if (rc == CRC_UNEXPECTED) status = CD_CONS_UNEXPECTED;
    int nz = 0, add_at = -1;
    if (rc == CRC_OK) {
        const V2 dl = x - a_old_t;
        const double dn = dsum(dl * dl);
        if (!(sqrt(dn) <= p.dbeta_tol * sqrt(double(d)))) { // :144: the group changed
            const double cmv = dsum(quad * dl * dl), rs = dsum(dl * (2.0 * gt - dl * quad));
            const T cmn = T(cmv / double(d));
            bs.cm = cmn > bs.cm ? cmn : bs.cm;     // pin_base:100-110
            bs.rsq += T(rs);                        // pin_base:124-134
            const V2 a_new_d = v_mul(c, V, x);      // back: beta = x V^T  (:156-157)
            const T an0 = T(a_new_d.a), an1 = T(a_new_d.b);
            V2 rsum_l{0, 0};
            if (!p.gram && p.sxm) rsum_l = V2{double(p.sxm[lane]) * double(ak0 - an0), in1 ? double(p.sxm[l1i]) * double(ak1 - an1) : 0.0};
            if (writer) {
                p.beta[lane] = an0;
                p.dcol[lane] = p.gram ? int32_t(p.b + lane) : int32_t(p.col0 + lane);
                p.dlt[lane] = an0 - ak0;
                if (in1) {
                    p.beta[l1i] = an1;
                    p.dcol[l1i] = p.gram ? int32_t(p.b + l1i) : int32_t(p.col0 + l1i);
                    p.dlt[l1i] = an1 - ak1;
                }
            }
            bs.resid_sum += T(dsum(rsum_l));
            bs.n_updates += 1;
            nz = d;
            if (p.mark && !was_active) { // add_active_set, pin_naive:294-304
                if (bs.active_size >= p.max_active_size) status = CD_MAX_ACTIVE;
                else add_at = bs.active_size;
                if (status != CD_MAX_ACTIVE) bs.active_size += 1;
            }
        }
    }
    bs.nz = nz;
    bs.status = status;
    if (c.tid == 0) {
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

// abs_grad of the wide groups with linear objects, one workgroup per such group (solver_base.hpp:62-93)
template <class T>
__global__ __launch_bounds__(XT) void cons_linear_wide_abs_grad_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ native,
                                                                       const int64_t* __restrict__ groups, const int64_t* __restrict__ gsizes,
                                                                       const int32_t* __restrict__ slot, const T* __restrict__ grad,
                                                                       const T* __restrict__ beta, const T* __restrict__ penalty,
                                                                       T regul_scale, ConsLinearStore<T> ls, T* __restrict__ abs_grad) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int g = list[blockIdx.x];
    if (native[g] != ADELIE_HIP_NATIVE_LINEAR) return;
    const int d = int(gsizes[g]), m = ls.m[g];
    if (d <= 64 || d > XD || m < 1 || m > XM) return; // (cons_linear_abs_grad_kernel's groups)
    XCtx c = make_ctx(smem_raw, m, d, threadIdx.x);
    const int lane = c.lane, l1i = lane + 64;
    const bool in1 = c.in1, in_m = c.in_m, writer = c.wave == 0;
    const int64_t k0 = groups[g], o = ls.doff[g];
    const double* A = ls.A + ls.aoff[g];
    double mu = in_m ? double(ls.mu[o + lane]) : 0.0;
    const V2 v{double(grad[k0 + lane]), in1 ? double(grad[k0 + l1i]) : 0.0};
    const int b = slot[g]; // the group's first screen value, -1 outside the screen set
    if (b >= 0) {          // :69-75: the group's gradient minus the penalty's and the constraint's terms
        V2 atmu{0, 0};
        for (int k = 0; k < m; ++k) {
            const double mk = rl(mu, k);
            atmu.a += A[size_t(k) * d + lane] * mk;
            if (in1) atmu.b += A[size_t(k) * d + l1i] * mk;
        }
        const double regul = double(regul_scale) * double(penalty[g]);
        const V2 e{v.a - regul * double(beta[b + lane]) - atmu.a, in1 ? v.b - regul * double(beta[b + l1i]) - atmu.b : 0.0};
        const double acc = dsum(e * e);
        if (c.tid == 0) abs_grad[g] = T(sqrt(acc));
        return;
    }
    // :88-93 solve_zero (constraint_linear.ipp:520-603): warm-started from the multipliers held, run to the end
    const double lower = in_m ? fmax(ls.lower[o + lane], -kMaxSolver) : 0.0, upper = in_m ? fmin(ls.upper[o + lane], kMaxSolver) : 0.0;
    const double slo = (lower >= 0) ? -kMaxSolver : 0.0, shi = (upper <= 0) ? kMaxSolver : 0.0;
    const double avars = in_m ? ls.vars[o + lane] : 0.0;
    OList ord = active_order(c, load_order(ls.order + o, ls.norder[g], m, lane), mu);
    BvlsCfg cfg;
    cfg.max_iters = int64_t(ls.cfg[2 * size_t(g)]); cfg.tol = ls.cfg[2 * size_t(g) + 1];
    stage_A(c, A); // (its barrier also stands between the reads of mu / order above and wave 0's writes below)
    double loss = 0;
    const int rc = lin_bvls(c, v, mu, ord, avars, slo, shi, dsum(v * v), false, 0.0, cfg, loss);
    if (rc != CRC_OK) {
        if (c.tid == 0) ls.err[0] = CD_CONS_BVLS;
        return;
    }
    if (writer) {
        if (in_m) ls.mu[o + lane] = T(mu);
        store_order(ord, ls.order + o, ls.norder + g, m, lane);
        if (lane == 0) abs_grad[g] = T(sqrt(fmax(2 * loss, 0.0)));
    }
}

size_t wide_lds(int m, int d, bool with_H) {
    return (size_t(OFF_B) + size_t(d) * size_t(m | 1) + (with_H ? size_t(m) * size_t(m | 1) : size_t(0))) * sizeof(double);
}

// the larger of the plain and the opt-in LDS figure of this device: hipFuncSetAttribute opts in
int lds_limit() {
    static const int limit = [] {
        int dev = 0, plain = 0, optin = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&plain, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) plain = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) optin = 0;
        (void)hipGetLastError();
        return std::max(plain, optin);
    }();
    return limit;
}
template <class K>
void raise_lds(K kernel, const char* name, size_t need) {
    if (size_t(lds_limit()) < need)
        throw std::runtime_error(std::string("adelie_hip: ") + name + " needs " + std::to_string(need) + " bytes of LDS, the device gives a workgroup " +
                                 std::to_string(lds_limit()) + ".");
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(need));
    (void)hipGetLastError();
}

} // namespace

size_t cons_visit_linear_wide_lds(int m, int q) { return wide_lds(m, q, true); }

template <class T>
void launch_grp_cons_visit_linear_wide(const ConsVisitParams<T>& p, hipStream_t s) {
    if (p.q <= 64 || p.q > XD || p.m < 1 || p.m > XM)
        throw std::runtime_error("adelie_hip: the wide linear constraint visit takes groups of 65 to 128 coefficients with 1 to 64 rows.");
    if (!p.V) throw std::runtime_error("adelie_hip: the wide linear constraint visit needs the group's eigenbasis.");
    if (!p.lA || !p.llo || !p.lup || !p.lvars || !p.lorder || !p.lnorder)
        throw std::runtime_error("adelie_hip: device visit of a linear constraint without its description.");
    static const bool raised = [] { raise_lds(grp_cons_linear_wide_visit_kernel<T>, "grp_cons_linear_wide_visit_kernel", wide_lds(XM, XD, true)); return true; }();
    (void)raised;
    (void)hipGetLastError();
    hipLaunchKernelGGL((grp_cons_linear_wide_visit_kernel<T>), dim3(1), dim3(XT), wide_lds(p.m, p.q, true), s, p);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        throw std::runtime_error(std::string("adelie_hip: grp_cons_linear_wide_visit_kernel launch refused: ") + hipGetErrorString(e));
}

template <class T>
void launch_cons_linear_wide_abs_grad(const int32_t* list, int count, const int32_t* native, const int64_t* groups, const int64_t* gsizes,
                                      const int32_t* slot, const T* grad, const T* beta, const T* penalty, T regul_scale,
                                      const ConsLinearStore<T>& ls, T* abs_grad, hipStream_t s) {
    if (count <= 0) return;
    static const bool raised = [] { raise_lds(cons_linear_wide_abs_grad_kernel<T>, "cons_linear_wide_abs_grad_kernel", wide_lds(XM, XD, false)); return true; }();
    (void)raised;
    (void)hipGetLastError();
    // (one size for every group of the list: the largest the gate admits, with no Hessian behind it)
    hipLaunchKernelGGL((cons_linear_wide_abs_grad_kernel<T>), dim3(unsigned(count)), dim3(XT), wide_lds(XM, XD, false), s, list, native,
                       groups, gsizes, slot, grad, beta, penalty, regul_scale, ls, abs_grad);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        throw std::runtime_error(std::string("adelie_hip: cons_linear_wide_abs_grad_kernel launch refused: ") + hipGetErrorString(e));
}

#define INST(T)                                                                                                                      \
    template void launch_grp_cons_visit_linear_wide<T>(const ConsVisitParams<T>&, hipStream_t);                                     \
    template void launch_cons_linear_wide_abs_grad<T>(const int32_t*, int, const int32_t*, const int64_t*, const int64_t*, const int32_t*, \
                                                      const T*, const T*, const T*, T, const ConsLinearStore<T>&, T*, hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
