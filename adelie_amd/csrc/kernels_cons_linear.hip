// kernels_cons_linear.hip — `linear` constraint objects  lower <= A x <= upper  (A: m x d, m <= 64 rows on a group of d <= 64
// coefficients), solved on the device.
//
// The reference visits such a group through ConstraintLinear::solve (constraint_linear.ipp:232-497): the dual proximal-Newton
// driver of constraint/utils.hpp:24-243 on the m multipliers mu, the dense pinball coordinate descent as its Newton step
// (optimization/pinball_full.hpp:84-118) and a sign-bounded least squares fit of A'mu (solver_bvls.hpp through
// optimization/nnls.hpp) for the multipliers of a group whose primal is zero.  The bounded least squares is warm-started from
// the non-zero multipliers IN THE ORDER THEY BECAME NON-ZERO; that order decides which multipliers a group at x = 0 ends up
// with, so it is state: an int32 list of m entries and a count per group, kept in device memory next to mu.
//
// What is built here: ONE WAVEFRONT runs one whole visit.
//
//   eigen-coordinates   the visit receives the group's eigenbasis V (orthogonal to rounding) and works in the coordinates x of
//             the group update throughout.  B = A V (m x d) is formed once per visit with v_mfma_f64_16x16x4f64: all (up to
//             4 x 4) 16 x 16 tiles are accumulated at once in registers, so A and V are each read through L2 exactly once, and B
//             goes to LDS column by column with an odd leading dimension (conflict-free along rows and along columns).
//             Everything the driver reads is then a function of B: resid = v - B'mu, a bounded-least-squares row gradient
//             B[k] . resid, the Newton-step gradient B x, the inner products of the backtracking and convergence rules (inner
//             products of B'dmu), and the dual Hessian H = |x| B diag(b2) B' + (l1 kappa |x|) (B a)(B a)'.  Neither V (as
//             doubles) nor the d x d primal Hessian is ever stored.  The one quantity that is not a function of B, V'x in the
//             variance scale of the pinball stopping rule, reads V through L2 once per Newton iteration.
//   H         rebuilt once per Newton iteration as an MFMA product of two LDS operands (B and B diag(b2)): the tiles of the
//             lower triangle accumulate in registers, the rank-one term is added on the way out and every element is written
//             together with its mirror image, so H is exactly symmetric.  B and H take 2 x 33 KB of LDS at m = d = 64.
//   vectors   lane i carries component i of every d-vector and of every m-vector; a sum is wave_sum64 (fixed order), a scalar
//             of a coordinate is a readlane.  Every decision of the driver, of the pinball descent and of the bounded least
//             squares is wave-uniform, so a visit is bit-reproducible.
//   lists     the order / screen / active lists of the bounded least squares live in registers too: lane t carries entry t,
//             membership is a 64-bit mask, appending and filtering are wave-uniform loops over readlanes.
//   one wave  the two tile builds are 16 x 16 MFMAs of depth <= 64 (4 microseconds at the most); everything else is strictly
//             sequential.  Further waves would add workgroup barriers to every step of the descents and gain nothing measurable.
//
// The same file holds the `linear` part of abs_grad (solver_base.hpp:62-93): |grad - regul beta - A'mu| for a screened group,
// solve_zero (constraint_linear.ipp:520-603) for the others — the same bounded least squares in design coordinates (A staged in
// LDS in place of B, no early stop), which leaves the multipliers and their order as the object would hold them.
//
// Arithmetic is double precision for either value type.  Every loop is bounded by a configuration value or by m.
#include <stdexcept>
#include <string>
#include "kernels.hpp"
#include "wavered.hpp"
#include "cons_common.hpp"

namespace ahip {

namespace {

constexpr int LW = 64;               // lanes = largest group = most rows
constexpr int LNT = LW / 16;         // tiles per side at the most
constexpr double kMaxSolver = 1e100; // configs.hpp:13 max_solver_value
constexpr double kEps = 1e-16;       // constraint_linear.hpp:40: a multiplier at or below it counts as zero

typedef double ld4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double wsum(double x) { return wave_sum64(x); }
__device__ __forceinline__ double rl(double x, int l) { return prdl(x, l); }
__device__ __forceinline__ int rli(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ bool bit(uint64_t m, int k) { return (m >> k) & 1ull; }

struct LinCtx {
    int m, d, lane, LDB, LDH;
    double* B;   // [d][LDB]: B[k + j LDB], rows k < m, columns j < d
    double* H;   // [m][LDH] dual Hessian
    double* vs;  // [LW] broadcast slot
    double* vs2; // [LW] second broadcast slot
};

// a list of distinct indices below 64 in the order they were added: lane t carries entry t
struct OList {
    int v = 0, n = 0;
    uint64_t mask = 0;
};
__device__ __forceinline__ void ol_push(OList& o, int k, int lane) {
    if (k < 0 || k >= LW || bit(o.mask, k)) return;
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
__device__ __forceinline__ OList active_order(const LinCtx& c, const OList& o, double mu) {
    const uint64_t nz = __ballot(c.lane < c.m && fabs(mu) > kEps);
    OList r = ol_filter(o, nz, c.lane);
    for (uint64_t rem = nz & ~o.mask; rem; rem &= rem - 1) ol_push(r, __builtin_ctzll(rem), c.lane);
    return r;
}

// lane j < d: sum_k B[k][j] mu_k
__device__ __forceinline__ double bt_mul(const LinCtx& c, double mu) {
    __syncthreads();
    c.vs[c.lane] = c.lane < c.m ? mu : 0.0;
    __syncthreads();
    double acc = 0;
    if (c.lane < c.d)
        for (int k = 0; k < c.m; ++k) acc += c.B[k + c.lane * c.LDB] * c.vs[k];
    return acc;
}
// lane k < m: sum_j B[k][j] x_j
__device__ __forceinline__ double b_mul(const LinCtx& c, double x) {
    __syncthreads();
    c.vs[c.lane] = c.lane < c.d ? x : 0.0;
    __syncthreads();
    double acc = 0;
    if (c.lane < c.m)
        for (int j = 0; j < c.d; ++j) acc += c.B[c.lane + j * c.LDB] * c.vs[j];
    return acc;
}

// B = A V with v_mfma_f64_16x16x4f64 (A: m x d row-major doubles, V: d x d column-major of T, or nullptr for the identity of a
// group of one coefficient): fragment a = A[16 R + fr][i0 + fk], b = V[i0 + fk][16 C + fr]; acc e is row 16 R + fk + 4 e, column
// 16 C + fr.  All tiles at once: one pass over A and over V.
template <class T>
__device__ __forceinline__ void build_B(const LinCtx& c, const double* __restrict__ A, const T* __restrict__ V) {
    const int m = c.m, d = c.d, fr = c.lane & 15, fk = c.lane >> 4;
    const int mt = (m + 15) >> 4, dt = (d + 15) >> 4;
    ld4_t acc[LNT][LNT];
#pragma unroll
    for (int R = 0; R < LNT; ++R)
#pragma unroll
        for (int C = 0; C < LNT; ++C) acc[R][C] = ld4_t{0, 0, 0, 0};
    for (int i0 = 0; i0 < d; i0 += 4) {
        const int i = i0 + fk;
        const bool iok = i < d;
        double a[LNT], b[LNT];
#pragma unroll
        for (int R = 0; R < LNT; ++R) {
            const int r = R * 16 + fr;
            a[R] = (iok && r < m) ? A[size_t(r) * d + i] : 0.0;
            b[R] = (iok && r < d) ? (V ? double(V[size_t(i) + size_t(r) * d]) : 1.0) : 0.0;
        }
#pragma unroll
        for (int R = 0; R < LNT; ++R)
#pragma unroll
            for (int C = 0; C < LNT; ++C)
                if (R < mt && C < dt) acc[R][C] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[R], b[C], acc[R][C], 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int R = 0; R < LNT; ++R)
#pragma unroll
        for (int C = 0; C < LNT; ++C)
            if (R < mt && C < dt) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = R * 16 + fk + 4 * e, col = C * 16 + fr;
                    if (row < m && col < d) c.B[row + col * c.LDB] = acc[R][C][e];
                }
            }
    __syncthreads();
}

// H = x_norm B diag(b2) B' + l1kn (B a)(B a)', exactly symmetric.  b2 (zero beyond d) is in vs, B a (rows < m) in vs2.
__device__ __forceinline__ void build_H(const LinCtx& c, double x_norm, double l1kn) {
    const int m = c.m, d = c.d, fr = c.lane & 15, fk = c.lane >> 4, LDB = c.LDB;
    const int mt = (m + 15) >> 4;
    ld4_t acc[LNT][LNT];
#pragma unroll
    for (int R = 0; R < LNT; ++R)
#pragma unroll
        for (int C = 0; C < LNT; ++C) acc[R][C] = ld4_t{0, 0, 0, 0};
    for (int j0 = 0; j0 < d; j0 += 4) {
        const int j = j0 + fk;
        const bool jok = j < d;
        const double wj = jok ? c.vs[j] : 0.0;
        double a[LNT], b[LNT];
#pragma unroll
        for (int R = 0; R < LNT; ++R) {
            const int r = R * 16 + fr;
            a[R] = (jok && r < m) ? c.B[r + j * LDB] : 0.0;
            b[R] = a[R] * wj;
        }
#pragma unroll
        for (int R = 0; R < LNT; ++R)
#pragma unroll
            for (int C = 0; C < LNT; ++C)
                if (R < mt && C <= R) acc[R][C] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[R], b[C], acc[R][C], 0, 0, 0);
    }
    __syncthreads(); // (the descent's reads of the previous H are over)
#pragma unroll
    for (int R = 0; R < LNT; ++R)
#pragma unroll
        for (int C = 0; C < LNT; ++C)
            if (R < mt && C <= R) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = R * 16 + fk + 4 * e, col = C * 16 + fr;
                    if (row < m && col <= row) {
                        const double val = x_norm * acc[R][C][e] + l1kn * (c.vs2[row] * c.vs2[col]);
                        c.H[row + col * c.LDH] = val;
                        c.H[col + row * c.LDH] = val;
                    }
                }
            }
    __syncthreads();
}

// The pinball-penalised quadratic model by coordinate descent (pinball_full.hpp:84-118): g = its gradient at mu (kept current),
// lo_pen = -lower, up_pen = upper, var * tol the stopping threshold.
__device__ __forceinline__ int lin_pinball(const LinCtx& c, double& mu, double g, double lo_pen, double up_pen, double var, double tol,
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
            if (c.lane < m) g -= dl * c.H[c.lane + i * c.LDH];
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
// set (solver_bvls.hpp): `target` and the residual per lane j < d, beta (in: the warm start; out: the fit, zero off the kept
// set), the bounds and the row variances per lane k < m; `order` in: the warm start's list, out: the kept multipliers in the
// order they entered.  can_stop: the early stop at 2 loss <= l1sq (the fit inside solve); without it the descent runs to the end.
__device__ __forceinline__ int lin_bvls(const LinCtx& c, double target, double& beta, OList& order, double va, double slo, double shi,
                                        double y_var, bool can_stop, double l1sq, const BvlsCfg& cfg, double& loss_out) {
    const int m = c.m, d = c.d, lane = c.lane;
    const bool in_d = lane < d, in_m = lane < m;
    const double btb = bt_mul(c, beta); // (every lane takes part in the product)
    double resid = in_d ? target - btb : 0.0;
    double loss = 0.5 * wsum(resid * resid);
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
            const double bk = in_d ? c.B[k + lane * c.LDB] : 0.0;
            const double gk = wsum(bk * resid);
            const double nw = fmin(fmax(old + (vk <= 0 ? 0.0 : gk / vk), rl(slo, k)), rl(shi, k));
            if (nw == old) continue;
            if (lane == k) beta = nw;
            const double dl = nw - old, sds = vk * dl * dl;
            worst = fmax(worst, sds);
            loss -= dl * gk - 0.5 * sds;
            resid -= dl * bk;
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

// constraint/utils.hpp:24-243 with the hooks of ConstraintLinear, in eigen-coordinates.  Lane j < d: x (in/out), quad, v (the
// linear term); lane k < m: lo_pen = -lower, up_pen = upper, the row variances and mu (in/out).  `ord`: the multipliers' order.
template <class T>
__device__ __forceinline__ int lin_solve(const LinCtx& c, const T* __restrict__ V, double& x, double quad, double v, double l1, double l2,
                                         double lo_pen, double up_pen, double avars, double& mu, OList& ord, const LinCfg& cfg) {
    const int d = c.d, m = c.m, lane = c.lane;
    const bool in_d = lane < d, in_m = lane < m;
    const double vv = wsum(in_d ? v * v : 0.0), l1sq = l1 * l1;
    if (sqrt(vv) <= l1) { x = 0; mu = 0; ord = OList(); return CRC_OK; }
    // a negative multiplier needs an active lower bound at 0, a positive one an active upper bound (constraint_linear.ipp:286-293)
    const double slo = (-lo_pen >= 0) ? -kMaxSolver : 0.0, shi = (up_pen <= 0) ? kMaxSolver : 0.0;
    // multipliers that best explain v while the primal stays zero (:283-349); keeps the old ones when even those do not
    auto nearest_at_zero = [&](bool may_restore, double& gap) -> int {
        ord = active_order(c, ord, mu);
        double btm = bt_mul(c, mu); // (every lane takes part in the product)
        double e = in_d ? v - btm : 0.0;
        gap = wsum(e * e);
        if (gap <= l1sq) return CRC_OK; // :281-283
        double cand = mu, loss = 0;
        OList oc = ord;
        if (const int rc = lin_bvls(c, v, cand, oc, avars, slo, shi, vv, true, l1sq, cfg.nnls, loss); rc != CRC_OK) return rc;
        btm = bt_mul(c, cand);
        e = in_d ? v - btm : 0.0;
        gap = wsum(e * e);
        if (may_restore && gap > l1sq) return CRC_OK;
        mu = cand;
        ord = oc;
        return CRC_OK;
    };
    const bool x_zero_start = __ballot(in_d && x != 0) == 0ull;
    bool have_prev = false, zero_checked = false;
    double btmu_prev = 0, x_prev = 0, mu_prev = 0, rn_prev = -1, b1 = 0, b2 = 0, gap = 0;
    OList ord_prev;
    if (x_zero_start) {
        zero_checked = true;
        if (const int rc = nearest_at_zero(true, gap); rc != CRC_OK) return rc;
        if (gap <= l1sq) { x = 0; return CRC_OK; }
    }
    for (int it = 1; it <= cfg.max_iters; ++it) {
        const double btmu = bt_mul(c, mu);
        const double resid = in_d ? v - btmu : 0.0;
        const double rn = sqrt(wsum(resid * resid));
        bool inside = rn <= l1;
        double xn = -1;
        if (!inside) {
            group_prox(c, quad, resid, l1, l2, x, b1, b2);
            xn = sqrt(wsum(in_d ? x * x : 0.0));
            inside = xn <= 0;
            if (l1 <= 0) { b1 = quad + l2; b2 = in_d ? 1.0 / (b1 * xn + l1) : 0.0; } // (newton.hpp:72-75 leaves its buffers unset)
        }
        if (inside) {
            if (it == 1 && x_zero_start) { x = 0; return CRC_OK; }
            if (have_prev && fabs(wsum(in_d ? (btmu - btmu_prev) * x_prev : 0.0) / double(d)) <= cfg.tol) { x = 0; return CRC_OK; }
            if (!zero_checked) {
                zero_checked = true;
                const bool had_prev = have_prev;
                if (!had_prev) {
                    rn_prev = rn; have_prev = true;
                    mu_prev = mu; btmu_prev = btmu; x_prev = 0;
                    ord_prev = ord;
                }
                if (const int rc = nearest_at_zero(had_prev, gap); rc != CRC_OK) return rc;
                if (gap <= l1sq) { x = 0; return CRC_OK; }
                if (!had_prev) continue;
            }
            if (!have_prev || rn_prev <= l1 * 0.9999 || rn > l1 * 1.0001) return CRC_UNEXPECTED;
            // back towards the ellipse |v - B'mu| = l1 along mu_prev -> mu (constraint_linear.ipp:351-382)
            const double target = (1 - cfg.slack) * l1 + cfg.slack * rn_prev;
            const double dbt = in_d ? btmu - btmu_prev : 0.0;
            const double a = wsum(dbt * dbt), b = wsum(resid * dbt), cc = rn * rn - target * target;
            const double t_star = (-b + sqrt(fmax(b * b - a * cc, 0.0))) / a;
            mu = mu_prev + fmin(fmax(1 - t_star, 0.0), 1.0) * (mu - mu_prev);
            for (int t = 0; t < ord_prev.n; ++t) ol_push(ord, rli(ord_prev.v, t), lane); // the current multipliers first, then the previous ones
            continue;
        }
        if (have_prev && fabs(wsum(in_d ? (btmu - btmu_prev) * (x_prev - x) : 0.0) / double(d)) <= cfg.tol) return CRC_OK;
        rn_prev = rn; have_prev = true;
        mu_prev = mu; btmu_prev = btmu; x_prev = x;
        ord_prev = ord;
        // the dual Hessian and the variance scale of the descent's stopping rule (Woodbury), constraint/utils.hpp:208-237
        const double a_t = in_d ? x * b2 / xn : 0.0;
        const double kappa = 1.0 / wsum(in_d ? x * b1 * a_t : 0.0);
        const double ba = b_mul(c, a_t);
        __syncthreads();
        c.vs[lane] = in_d ? b2 : 0.0;
        c.vs2[lane] = in_m ? ba : 0.0;
        __syncthreads();
        build_H(c, xn, l1 * kappa * xn);
        c.vs[lane] = in_d ? x : 0.0; // V'x, the one product B does not give
        __syncthreads();
        double xq = 0;
        if (in_d) {
            if (V) for (int i = 0; i < d; ++i) xq += double(V[size_t(i) + size_t(lane) * d]) * c.vs[i];
            else xq = x;
        }
        const double xy = wsum(in_d ? x * xq : 0.0), s1 = wsum(in_d ? xq * xq / b2 : 0.0), s2 = wsum(in_d ? x * x * b2 : 0.0);
        const double var = fmax((s1 - (xy * xy) / ((xn * xn) / (l1 * kappa) + s2)) / xn, 0.0);
        const double g = b_mul(c, x);
        ord = active_order(c, ord, mu);
        if (const int rc = lin_pinball(c, mu, g, lo_pen, up_pen, var, cfg.qp_tol, cfg.qp_max_iters); rc != CRC_OK) return rc;
        ord = active_order(c, ord, mu);
    }
    return CRC_PN;
}

__device__ __forceinline__ LinCtx lin_ctx(char* smem, int m, int d, int lane) {
    LinCtx c;
    c.m = m; c.d = d; c.lane = lane; c.LDB = m | 1; c.LDH = m | 1;
    c.B = reinterpret_cast<double*>(smem);
    c.H = c.B + size_t(d) * c.LDB;
    c.vs = c.H + size_t(m) * c.LDH;
    c.vs2 = c.vs + LW;
    return c;
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
__global__ __launch_bounds__(LW) void grp_cons_linear_visit_kernel(ConsVisitParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int lane = threadIdx.x, d = p.q, m = p.m;
    const LinCtx c = lin_ctx(smem_raw, m, d, lane);
    const bool in = lane < d, in_m = lane < m;
    const T* V = d > 1 ? p.V : nullptr;
    build_B<T>(c, p.lA, V);
    const double gk = in ? double(p.gsrc[lane]) : 0.0, ak = in ? double(p.beta[lane]) : 0.0, quad = in ? double(p.vars[lane]) : 0.0;
    // the class keeps the bounds clamped to +-max_solver_value
    const double lo_pen = in_m ? -fmax(p.llo[lane], -kMaxSolver) : 0.0, up_pen = in_m ? fmin(p.lup[lane], kMaxSolver) : 0.0;
    const double avars = in_m ? p.lvars[lane] : 0.0;
    double mu = in_m ? double(p.mu[lane]) : 0.0;
    OList ord = load_order(p.lorder, p.lnorder[0], m, lane);
    CdBlkState<T> bs = *p.st;
    if (p.first_of_pass) bs.cm = T(0);
    // into the eigenbasis: g V, beta V  (pin_naive:123-135)
    c.vs[lane] = gk;
    c.vs2[lane] = ak;
    __syncthreads();
    double gt = gk, a_old_t = ak;
    if (in && V) {
        gt = 0; a_old_t = 0;
        for (int i = 0; i < d; ++i) {
            const double q = double(V[size_t(i) + size_t(lane) * d]);
            gt += c.vs[i] * q;
            a_old_t += c.vs2[i] * q;
        }
    }
    double x = in ? a_old_t : 0.0;
    const double lin = gt + quad * a_old_t;
    LinCfg cfg;
    cfg.max_iters = int(p.cfg[0]); cfg.tol = p.cfg[1]; cfg.qp_max_iters = int64_t(p.cfg[2]); cfg.qp_tol = p.cfg[3]; cfg.slack = p.cfg[4];
    cfg.nnls.max_iters = int64_t(p.lcfg[0]); cfg.nnls.tol = p.lcfg[1];
    const int rc = lin_solve<T>(c, V, x, quad, lin, p.l1, p.l2, lo_pen, up_pen, avars, mu, ord, cfg);
    if (!in) x = 0;
    const T mu_t = T(mu); // what the object holds, and the order brought up to date with it (ConstraintLinear::solve's last step)
    ord = active_order(c, ord, double(mu_t));
    if (in_m) p.mu[lane] = mu_t;
    store_order(ord, p.lorder, p.lnorder, m, lane);
    int status = bs.status;
    if (rc == CRC_PN) status = CD_CONS_PN;
    else if (rc == CRC_QP) status = CD_CONS_QP_BOX;
    else if (rc == CRC_BVLS) status = CD_CONS_BVLS;
    else if (rc == CRC_UNEXPECTED) status = CD_CONS_UNEXPECTED;
    int nz = 0;
    if (rc == CRC_OK) {
        const double dl = in ? x - a_old_t : 0.0;
        const double dn = wsum(dl * dl);
        if (!(sqrt(dn) <= p.dbeta_tol * sqrt(double(d)))) { // :144: the group changed
            const double cmv = wsum(quad * dl * dl), rs = wsum(dl * (2 * gt - dl * quad));
            const T cmn = T(cmv / double(d));
            bs.cm = cmn > bs.cm ? cmn : bs.cm;     // pin_base:100-110
            bs.rsq += T(rs);                        // pin_base:124-134
            __syncthreads();
            c.vs[lane] = x;
            __syncthreads();
            double a_new_d = x; // back: beta = x V^T  (:156-157)
            if (in && V) {
                a_new_d = 0;
                for (int j = 0; j < d; ++j) a_new_d += double(V[size_t(lane) + size_t(j) * d]) * c.vs[j];
            }
            const T a_new = T(a_new_d), ak_t = in ? p.beta[lane] : T(0);
            const T dlt = in ? a_new - ak_t : T(0);
            double rsum_l = 0;
            if (in) {
                p.beta[lane] = a_new;
                p.dcol[lane] = p.gram ? int32_t(p.b + lane) : int32_t(p.col0 + lane);
                p.dlt[lane] = dlt;
                if (!p.gram && p.sxm) rsum_l = double(p.sxm[lane]) * double(ak_t - a_new);
            }
            bs.resid_sum += T(wsum(rsum_l));
            bs.n_updates += 1;
            nz = d;
            if (p.mark && !p.is_active[p.ss]) { // add_active_set, pin_naive:294-304
                if (bs.active_size >= p.max_active_size) {
                    status = CD_MAX_ACTIVE;
                } else if (lane == 0) {
                    p.is_active[p.ss] = 1;
                    p.active_set[bs.active_size] = p.ss;
                }
                if (status != CD_MAX_ACTIVE) bs.active_size += 1;
            }
        }
    }
    bs.nz = nz;
    bs.status = status;
    if (lane == 0) {
        *p.st = bs;
        if (p.n_visits) p.n_visits[0] += 1;
        if (p.host_st && p.report_seq) {
            *p.host_st = bs;
            __threadfence_system();
            __hip_atomic_store(p.host_seq, p.report_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// abs_grad of the groups with linear objects, one wavefront per such group (solver_base.hpp:62-93)
template <class T>
__global__ __launch_bounds__(LW) void cons_linear_abs_grad_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ native,
                                                                  const int64_t* __restrict__ groups, const int64_t* __restrict__ gsizes,
                                                                  const int32_t* __restrict__ slot, const T* __restrict__ grad,
                                                                  const T* __restrict__ beta, const T* __restrict__ penalty, T regul_scale,
                                                                  ConsLinearStore<T> ls, T* __restrict__ abs_grad) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int g = list[blockIdx.x];
    if (native[g] != ADELIE_HIP_NATIVE_LINEAR) return;
    const int lane = threadIdx.x, d = int(gsizes[g]), m = ls.m[g];
    const int64_t k0 = groups[g], o = ls.doff[g];
    const double* A = ls.A + ls.aoff[g];
    const bool in = lane < d, in_m = lane < m;
    double mu = in_m ? double(ls.mu[o + lane]) : 0.0;
    const int b = slot[g]; // the group's first screen value, -1 outside the screen set
    if (b >= 0) {          // :69-75: the group's gradient minus the penalty's and the constraint's terms
        double atmu = 0;
        for (int k = 0; k < m; ++k) atmu += (in ? A[size_t(k) * d + lane] : 0.0) * rl(mu, k);
        const double e = in ? double(grad[k0 + lane]) - double(regul_scale) * double(penalty[g]) * double(beta[b + lane]) - atmu : 0.0;
        const double acc = wsum(e * e);
        if (lane == 0) abs_grad[g] = T(sqrt(acc));
        return;
    }
    // :88-93 solve_zero (constraint_linear.ipp:520-603): warm-started from the multipliers held, run to the end
    const LinCtx c = lin_ctx(smem_raw, m, d, lane);
    for (int e = lane; e < m * d; e += LW) c.B[(e / d) + (e % d) * c.LDB] = A[e];
    __syncthreads();
    const double v = in ? double(grad[k0 + lane]) : 0.0;
    const double lower = in_m ? fmax(ls.lower[o + lane], -kMaxSolver) : 0.0, upper = in_m ? fmin(ls.upper[o + lane], kMaxSolver) : 0.0;
    const double slo = (lower >= 0) ? -kMaxSolver : 0.0, shi = (upper <= 0) ? kMaxSolver : 0.0;
    OList ord = active_order(c, load_order(ls.order + o, ls.norder[g], m, lane), mu);
    BvlsCfg cfg;
    cfg.max_iters = int64_t(ls.cfg[2 * size_t(g)]); cfg.tol = ls.cfg[2 * size_t(g) + 1];
    double loss = 0;
    const int rc = lin_bvls(c, v, mu, ord, in_m ? ls.vars[o + lane] : 0.0, slo, shi, wsum(v * v), false, 0.0, cfg, loss);
    if (rc != CRC_OK) {
        if (lane == 0) ls.err[0] = CD_CONS_BVLS;
        return;
    }
    if (in_m) ls.mu[o + lane] = T(mu);
    store_order(ord, ls.order + o, ls.norder + g, m, lane);
    if (lane == 0) abs_grad[g] = T(sqrt(fmax(2 * loss, 0.0)));
}

size_t linear_lds(int m, int d) { return (size_t(d) * size_t(m | 1) + size_t(m) * size_t(m | 1) + 2 * LW) * sizeof(double); }

template <class K>
void raise_lds(K kernel) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(linear_lds(LW, LW)));
}

} // namespace

size_t cons_visit_linear_lds(int m, int q) { return q > LW ? cons_visit_linear_wide_lds(m, q) : linear_lds(m, q); }

template <class T>
void launch_grp_cons_visit_linear(const ConsVisitParams<T>& p, hipStream_t s) {
    if (p.q > LW && p.q <= 128 && p.m >= 1 && p.m <= LW) return launch_grp_cons_visit_linear_wide<T>(p, s); // kernels_cons_linear_wide.hip
    if (p.q < 1 || p.q > LW || p.m < 1 || p.m > LW)
        throw std::runtime_error("adelie_hip: device visit of a linear constraint beyond 128 coefficients or 64 rows.");
    if (!p.lA || !p.llo || !p.lup || !p.lvars || !p.lorder || !p.lnorder)
        throw std::runtime_error("adelie_hip: device visit of a linear constraint without its description.");
    static const bool raised = [] { raise_lds(grp_cons_linear_visit_kernel<T>); return true; }();
    (void)raised;
    (void)hipGetLastError();
    hipLaunchKernelGGL((grp_cons_linear_visit_kernel<T>), dim3(1), dim3(LW), linear_lds(p.m, p.q), s, p);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        throw std::runtime_error(std::string("adelie_hip: grp_cons_linear_visit_kernel launch refused: ") + hipGetErrorString(e));
}

template <class T>
void launch_cons_linear_abs_grad(const int32_t* list, int count, const int32_t* native, const int64_t* groups, const int64_t* gsizes,
                                 const int32_t* slot, const T* grad, const T* beta, const T* penalty, T regul_scale,
                                 const ConsLinearStore<T>& ls, T* abs_grad, hipStream_t s) {
    if (count <= 0) return;
    static const bool raised = [] { raise_lds(cons_linear_abs_grad_kernel<T>); return true; }();
    (void)raised;
    (void)hipGetLastError();
    // (one size for every group of the list: the largest the gate admits, with no Hessian behind it)
    hipLaunchKernelGGL((cons_linear_abs_grad_kernel<T>), dim3(unsigned(count)), dim3(LW), linear_lds(LW, LW), s, list, native, groups,
                       gsizes, slot, grad, beta, penalty, regul_scale, ls, abs_grad);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        throw std::runtime_error(std::string("adelie_hip: cons_linear_abs_grad_kernel launch refused: ") + hipGetErrorString(e));
}

#define INST(T)                                                                                                                 \
    template void launch_grp_cons_visit_linear<T>(const ConsVisitParams<T>&, hipStream_t);                                     \
    template void launch_cons_linear_abs_grad<T>(const int32_t*, int, const int32_t*, const int64_t*, const int64_t*, const int32_t*, \
                                                 const T*, const T*, const T*, T, const ConsLinearStore<T>&, T*, hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
