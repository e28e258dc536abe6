// kernels_bvls.hip — bounded-variable least squares on a resident dense design (adelie.solver.bvls: solver_bvls.hpp,
// state_bvls.ipp).  Kernels, the solver's part of the host driver and the C-ABI entry points of adelie_hip_bvls_solve.
//
// The reference visits one coordinate at a time and pays two n-length passes per visit (cmul for the gradient, ctmul for the
// residual).  Here the gradient g_a = x_a^T W r of EVERY screen coordinate is kept current through the resident Gram matrix
// G = X_S^T W X_S (ns x ns, uncentred, both triangles): a visit that changes beta_k by `del` does g_a -= G[a, k] * del for all
// a (one contiguous Gram column), and a visit that changes nothing touches no memory but a few broadcast reads.  One workgroup
// runs a whole fit() — screen passes, active-set passes, prune — without leaving the compute unit; the residual is caught up
// once per fit from the compact list of changes (launch_axpy_cols), and the Gram-updated gradients are thrown away at every KKT
// round: the screen members' g is re-read from the fresh full gradient X^T (w * r).
//
// Visiting order, predicates (`<=`, `==`), counters and exits are the reference's.  Two things are fixed where the reference
// leaves them open or does them differently without a visible effect:
//   * kkt_screen sorts the violations with std::sort, which leaves the order of equal violations unspecified (and carries the
//     previous round's order into the next sort).  Here the indices are sorted with std::stable_sort from 0..p-1 every round,
//     so ties go to the lower index.
//   * add_active appends a coordinate at the visit that changes it; here a screen pass raises a flag at that visit and the
//     flagged non-members are appended, in screen order, at the end of the pass.  A screen pass visits in screen order, so the
//     list is the same; it is complete before the pass's max-iterations exit is taken.
//
// Synchronisation inside the fit kernel, which this solver shares with the pinball one: cd_fit_body.hpp.  The host driver
// around it, shared as well: cd_screen_driver.hpp.
#include "cd_screen_driver.hpp"

namespace ahip {

double g_bvls_gram_limit_mb = 16384.0; // adelie_hip_set_config("bvls_gram_limit_mb", x)
int64_t g_bvls_lds_max_ns = 0;         // adelie_hip_set_config("bvls_lds_max_ns", x): 0 = automatic

namespace {


// the fit kernel (cd_fit_body.hpp) with the box rule: coordinate_descent's update (solver_bvls.hpp:44-60) and prune's predicate
template <class T>
struct BvlsRule {
    static __device__ __forceinline__ T update(T vk, T lk, T uk, T gk, T bk) {
#pragma clang fp contract(off)
        const T step = (vk <= T(0)) ? T(0) : (gk / vk);
        const T cand = bk + step;
        const T hi = (cand < lk) ? lk : cand; // std::max(cand, lk)
        return (uk < hi) ? uk : hi;           // std::min(hi, uk)
    }
    static __device__ __forceinline__ bool drop(T b, T lk, T uk) { return b <= lk || b >= uk; }
};


// viols_j = max(grad_j, 0) [beta_j < upper_j] - min(grad_j, 0) [beta_j > lower_j]   (solver_bvls.hpp:266-271); grad is kept
template <class T>
__global__ __launch_bounds__(256) void bvls_viols_kernel(const T* __restrict__ grad, const T* __restrict__ beta,
                                                         const T* __restrict__ lower, const T* __restrict__ upper, int64_t p,
                                                         T* __restrict__ viols) {
    const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j >= p) return;
    const T g = grad[j], b = beta[j];
    const T gp = g > T(0) ? g : T(0), gm = g < T(0) ? g : T(0);
    viols[j] = gp * T(b < upper[j] ? 1 : 0) - gm * T(b > lower[j] ? 1 : 0);
}

// screen-order copies for the fit kernel: g of every member from `src` (the full gradient: src[cols[a]], or a sweep of the screen
// columns: src[a]); bounds, variances and beta of the members from position a0 on
template <class T>
__global__ __launch_bounds__(256) void bvls_gather_kernel(const int32_t* __restrict__ cols, int32_t ns, int32_t a0,
                                                          const T* __restrict__ src, int by_col, const T* __restrict__ lower,
                                                          const T* __restrict__ upper, const T* __restrict__ vars,
                                                          const T* __restrict__ beta, T* __restrict__ g_s,
                                                          T* __restrict__ lower_s, T* __restrict__ upper_s,
                                                          T* __restrict__ vars_s, T* __restrict__ beta_s) {
    const int32_t a = int32_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a >= ns) return;
    const int64_t j = cols[a];
    g_s[a] = by_col ? src[j] : src[a];
    if (a >= a0) {
        lower_s[a] = lower[j];
        upper_s[a] = upper[j];
        vars_s[a] = vars[j];
        beta_s[a] = beta[j];
    }
}


} // namespace
} // namespace ahip

using namespace ahip;

struct adelie_hip_bvls_result : CdScreenResult {};

static_assert(ADELIE_HIP_BVLS_BETA == CDS_BETA && ADELIE_HIP_BVLS_RESID == CDS_RESID && ADELIE_HIP_BVLS_GRAD == CDS_GRAD &&
                  ADELIE_HIP_BVLS_SCREEN_SET == CDS_SCREEN_SET && ADELIE_HIP_BVLS_ACTIVE_SET == CDS_ACTIVE_SET &&
                  ADELIE_HIP_BVLS_IS_SCREEN == CDS_IS_SCREEN && ADELIE_HIP_BVLS_IS_ACTIVE == CDS_IS_ACTIVE,
              "the shared result vectors");
static_assert(ADELIE_HIP_BVLS_LOSS == CDS_LOSS && ADELIE_HIP_BVLS_ITERS == CDS_ITERS && ADELIE_HIP_BVLS_N_KKT == CDS_N_KKT &&
                  ADELIE_HIP_BVLS_SCREEN_SET_SIZE == CDS_SCREEN_SET_SIZE && ADELIE_HIP_BVLS_ACTIVE_SET_SIZE == CDS_ACTIVE_SET_SIZE &&
                  ADELIE_HIP_BVLS_TOTAL_TIME == CDS_TOTAL_TIME && ADELIE_HIP_BVLS_T_SWEEP_MS == CDS_T_SWEEP_MS &&
                  ADELIE_HIP_BVLS_T_GRAM_MS == CDS_T_GRAM_MS && ADELIE_HIP_BVLS_T_FIT_MS == CDS_T_FIT_MS &&
                  ADELIE_HIP_BVLS_N_CHANGED == CDS_N_CHANGED,
              "the shared result scalars");

namespace {

// what the shared driver (cd_screen_driver.hpp) does not know: X is (n, p), weighted, with box bounds and given variances
template <class T>
struct BvlsSolver : CdScreenDriver<T, BvlsSolver<T>, adelie_hip_bvls_args> {
    using Base = CdScreenDriver<T, BvlsSolver<T>, adelie_hip_bvls_args>;
    using Base::Base;
    using Base::a, Base::n, Base::p, Base::s, Base::Xv, Base::timer, Base::ns, Base::ld;
    using Base::d_r, Base::d_grad, Base::d_viols, Base::d_beta, Base::d_cols, Base::d_dcol, Base::d_dlt, Base::d_cnt, Base::d_g;
    using Base::d_lower_s, Base::d_upper_s, Base::d_vars_s, Base::d_beta_s, Base::d_G, Base::d_work_sweep;
    using Rule = BvlsRule<T>;
    static constexpr const char* kName = "bvls";
    static double gram_limit_mb() { return g_bvls_gram_limit_mb; }
    static int64_t lds_max_ns() { return g_bvls_lds_max_ns; }

    DevBuf<T> d_w, d_v, d_lower, d_upper, d_vars, d_work_gram;

    void upload() {
        d_w.reserve(size_t(n)), d_v.reserve(size_t(n));
        d_lower.reserve(size_t(p)), d_upper.reserve(size_t(p)), d_vars.reserve(size_t(p));
        d_w.upload(static_cast<const T*>(a->weights), size_t(n), s);
        d_r.upload(static_cast<const T*>(a->resid), size_t(n), s);
        d_beta.upload(static_cast<const T*>(a->beta), size_t(p), s);
        d_lower.upload(static_cast<const T*>(a->lower), size_t(p), s);
        d_upper.upload(static_cast<const T*>(a->upper), size_t(p), s);
        d_vars.upload(static_cast<const T*>(a->X_vars), size_t(p), s);
    }
    // out[c] = x_col(c)' (w * r)
    void sweep(const int32_t* cols, int64_t ncols, T* out) {
        timer.begin(PH_SWEEP, s);
        launch_vmul<T>(d_w.p, d_r.p, d_v.p, n, s);
        T* work = d_work_sweep.reserve(size_t(sweep_work_elems(n, ncols)));
        launch_sweep<T>(Xv, d_v.p, out, 0, ncols, cols, nullptr, nullptr, false, work, s);
        timer.end(s);
    }
    void viols() {
        hipLaunchKernelGGL((bvls_viols_kernel<T>), dim3(cd_blocks_for(p, 256)), dim3(256), 0, s, d_grad.p, d_beta.p, d_lower.p,
                           d_upper.p, p, d_viols.p);
    }
    // rows and columns [ns_old, ns_new) of G
    void extend(int64_t ns_old, int64_t ns_new) {
        const int64_t N = ns_new - ns_old;
        if (N <= 0) return;
        T* work = d_work_gram.reserve(size_t(gram_work_elems(n, ns_new, N)));
        timer.begin(PH_GRAM, s);
        launch_gram<T>(Xv, d_w.p, d_cols.p, int32_t(ns_new), 0, d_cols.p + ns_old, int32_t(N), int32_t(ns_old), nullptr, false,
                       d_G.p, ld, work, s);
        timer.end(s);
    }
    void gather(int64_t a0, const T* src, bool by_col) {
        hipLaunchKernelGGL((bvls_gather_kernel<T>), dim3(cd_blocks_for(ns, 256)), dim3(256), 0, s, d_cols.p, int32_t(ns), int32_t(a0),
                           src, by_col ? 1 : 0, d_lower.p, d_upper.p, d_vars.p, d_beta.p, d_g.p, d_lower_s.p, d_upper_s.p,
                           d_vars_s.p, d_beta_s.p);
    }
    const int32_t* dcol_src() { return d_cols.p; }
    // r -= X * delta
    void catch_up() { launch_axpy_cols<T>(Xv, d_dcol.p, d_dlt.p, d_cnt.p, 0, T(-1), d_r.p, s); }
};

} // namespace

extern "C" {

int adelie_hip_bvls_solve(adelie_hip_design* X, const adelie_hip_bvls_args* a, adelie_hip_bvls_result** out) {
    return cd_screen_solve<BvlsSolver>(X, a, out, [&] {
        if (X->is_pieces())
            throw make_core_error("bvls is not offered on a design made of pieces (concatenate(..., resident=\"pieces\")); "
                                  "resident=\"auto\" gives one design, on which everything works.");
        if (!X->is_dense() || X->cov || X->constraint || X->std_center)
            throw make_core_error("bvls: X must be a plain dense design on this route.");
        const int64_t n = X->n, p = X->p;
        // state_bvls.ipp:15-74
        if (a->n_X_vars != p) throw make_solver_error("X_vars must be (p,) where X is (n, p). ");
        if (a->n_lower != p) throw make_solver_error("lower must be (p,) where X is (n, p). ");
        if (a->n_upper != p) throw make_solver_error("upper must be (p,) where X is (n, p). ");
        if (a->n_weights != n) throw make_solver_error("weights must be (n,) where X is (n, p). ");
        if (a->kappa <= 0) throw make_solver_error("kappa must be > 0. ");
        if (a->tol < 0) throw make_solver_error("tol must be >= 0.");
        if (a->active_set_size > p) throw make_solver_error("active_set_size must be <= p where X is (n, p). ");
        if (a->n_active_set != p) throw make_solver_error("active_set must be (p,) where X is (n, p). ");
        if (a->n_is_active != p) throw make_solver_error("is_active must be (p,) where X is (n, p). ");
        if (a->n_beta != p) throw make_solver_error("beta must be (p,) where X is (p, n). ");
        if (a->n_resid != n) throw make_solver_error("resid must be (n,) where X is (n, p). ");
        if (a->n_grad != p) throw make_solver_error("grad must be (p,) where X is (n, p). ");
        if (p >= (int64_t(1) << 31)) throw make_core_error("bvls: p must be below 2^31.");
        if (n <= 0 || p <= 0) throw make_core_error("bvls: X must not be empty.");
        if ((p && (!a->X_vars || !a->lower || !a->upper || !a->beta || !a->grad)) || (n && (!a->weights || !a->resid)))
            throw make_core_error("null argument.");
        if (a->screen_set_size < 0 || a->screen_set_size > p || a->active_set_size < 0 ||
            (a->screen_set_size && !a->screen_set) || (a->active_set_size && !a->active_set))
            throw make_core_error("bvls: screen_set_size must be in [0, p].");
        if (const char* e = cd_screen_warm_start_error(a->screen_set, a->screen_set_size, a->active_set, a->active_set_size, p,
                                                       "bvls: screen_set must hold distinct indices in [0, p).",
                                                       "bvls: active_set must hold distinct members of screen_set."))
            throw make_core_error(e);
    });
}

int adelie_hip_bvls_result_destroy(adelie_hip_bvls_result* r) {
    delete r;
    return 0;
}

int64_t adelie_hip_bvls_result_size(const adelie_hip_bvls_result* r, int which) { return cd_result_size(r, which); }
int adelie_hip_bvls_result_copy(const adelie_hip_bvls_result* r, int which, void* out, int64_t cap) {
    return cd_result_copy(r, which, out, cap);
}
double adelie_hip_bvls_result_scalar(const adelie_hip_bvls_result* r, int which) { return cd_result_scalar(r, which); }
const char* adelie_hip_bvls_result_error(const adelie_hip_bvls_result* r) { return r ? r->error.c_str() : ""; }

} // extern "C"
