// kernels_pinball.hip — pinball least squares on a resident constraint matrix (adelie.solver.pinball: solver_pinball.hpp,
// state_pinball.ipp).  Kernels, the solver's part of the host driver and the C-ABI entry points of adelie_hip_pinball_solve.
//
//     minimise over beta in R^m   1/2 || S^{-1/2} v - S^{1/2} A' beta ||^2 + penalty_neg' beta_- + penalty_pos' beta_+
//
// The handle holds A (m, d) row-major, i.e. the (d, m) column-major matrix A' of a dense design: the full gradient A resid is
// launch_sweep over the m columns, a row of A is one contiguous column.  A matrix kept sparse
// (adelie_hip_design_create_constraint_csc) is the kCsc design of A' in the same sense: the full gradient is launch_sweep_csc,
// a row of A one compressed column, and the products of extend() below come from kernels_pinball_sparse.hip, term for term
// those of the dense route.  Everything after them (H, the compact AS, the fit kernel, the catch-up) is dense either way.
//
// The reference visits one coordinate at a time and pays a d-long dot per visit (rvmul for the gradient) plus a d-long update
// of the residual when the visit changes the coefficient.  Here the gradient g_a = A[a, :] . resid of EVERY screen coordinate
// is kept current through the resident matrix H = A_S S A_S' (ns x ns, both triangles computed, H[a, k] = A[a, :] . (A[k, :] S)):
// a visit that changes beta_k by `del` does g_a -= H[a, k] * del for all a (one contiguous column of H), and a visit that
// changes nothing touches no memory but a few broadcast reads.  One workgroup runs a whole fit() without leaving the compute
// unit: the kernel is the one bvls runs (cd_fit_body.hpp, which also describes its synchronisation) with the pinball update
// (solver_pinball.hpp:37-61) and prune predicate (beta == 0), and so is the host driver around it (cd_screen_driver.hpp: the
// screen-order buffers, H's growth, fit, the warm start and the KKT loop).  The residual is caught up once per fit from the compact list of
// changes (launch_axpy_cols on the compact rows A_S S, kept as a (d, capacity) column-major array in screen order), and the
// H-updated gradients are thrown away at every KKT round: the members' g is re-read from the fresh full gradient.
//
// A KKT round that admits members [ns_old, ns_new) computes AS[k, :] = A[k, :] S for them, then the new columns of H for all
// members and the new rows of H for the old ones.  Both are products P' Q of two different matrices (S and A', A' and AS), which
// the MFMA Gram kernel (one matrix on both sides, a diagonal weight between) does not take, so they go through one plain
// LDS-tiled kernel: every output element is one thread's sequential d-term dot, whatever the shape.
//
// Visiting order, predicates (`<=`, `==`), counters and exits are the reference's.  Two things are fixed where the reference
// leaves them open or does them differently without a visible effect:
//   * kkt_screen sorts the violations with std::sort, which leaves the order of equal violations unspecified (and carries the
//     previous round's order into the next sort).  Here the indices are sorted with std::stable_sort from 0..m-1 every round,
//     so ties go to the lower index.
//   * add_active: see cd_fit_body.hpp.
//
// An infinite penalty (max_solver_value is inf in float32) needs no special case: the update gives copysign(0, +-inf) = 0 on
// that side and the violation -inf, which sorts last.
#include "cd_screen_driver.hpp"

namespace ahip {

double g_pinball_gram_limit_mb = 16384.0; // adelie_hip_set_config("pinball_gram_limit_mb", x)
int64_t g_pinball_lds_max_ns = 0;         // adelie_hip_set_config("pinball_lds_max_ns", x): 0 = automatic

namespace {

// coordinate_descent's update (solver_pinball.hpp:46-53) and prune's predicate (:143); lk = penalty_neg, uk = penalty_pos
template <class T>
struct PinballRule {
    static __device__ __forceinline__ T update(T vk, T lk, T uk, T gk, T bk) {
#pragma clang fp contract(off)
        if (vk <= T(0)) return bk;
        const T gk0 = gk + vk * bk;
        const T gk0_lk = gk0 + lk;
        const T a = -gk0_lk, b = gk0 - uk;
        const T mx = (a < b) ? b : a;         // std::max(a, b)
        const T mag = (mx < T(0)) ? T(0) : mx; // std::max(mx, 0)
        return copysign(mag, gk0_lk) / vk;
    }
    static __device__ __forceinline__ bool drop(T b, T, T) { return b == T(0); }
};

constexpr int kTile = 16;

// C[r + c * ldc] = sum_{i < K} P[i + pcol(r) * ldp] * Q[i + qcol(c) * ldq]   (r < M, c < N; pcol(r) = pcols ? pcols[r] : r)
// One thread per element; the dot runs over i in ascending order in one accumulator.
template <class T>
__global__ __launch_bounds__(kTile * kTile) void ptq_kernel(const T* __restrict__ P, int64_t ldp, const int32_t* __restrict__ pcols,
                                                           int32_t M, const T* __restrict__ Q, int64_t ldq,
                                                           const int32_t* __restrict__ qcols, int32_t N, int64_t K,
                                                           T* __restrict__ C, int64_t ldc) {
    __shared__ T sP[kTile][kTile + 1];
    __shared__ T sQ[kTile][kTile + 1];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t r0 = int64_t(blockIdx.x) * kTile, c0 = int64_t(blockIdx.y) * kTile;
    // the column this thread loads for the tiles (row ty of each tile), and the element it owns
    const int64_t rl = r0 + ty, cl = c0 + ty;
    const int64_t pc = rl < M ? (pcols ? int64_t(pcols[rl]) : rl) : -1;
    const int64_t qc = cl < N ? (qcols ? int64_t(qcols[cl]) : cl) : -1;
    T acc = T(0);
    for (int64_t i0 = 0; i0 < K; i0 += kTile) {
        const int64_t i = i0 + tx;
        sP[ty][tx] = (pc >= 0 && i < K) ? P[i + pc * ldp] : T(0);
        sQ[ty][tx] = (qc >= 0 && i < K) ? Q[i + qc * ldq] : T(0);
        __syncthreads();
#pragma unroll
        for (int ii = 0; ii < kTile; ++ii) acc += sP[tx][ii] * sQ[ty][ii];
        __syncthreads();
    }
    const int64_t r = r0 + tx, c = c0 + ty;
    if (r < M && c < N) C[r + c * ldc] = acc;
}

// viols_j = max(grad_j - penalty_pos_j, -penalty_neg_j - grad_j)   (solver_pinball.hpp:240); grad is kept
template <class T>
__global__ __launch_bounds__(256) void pinball_viols_kernel(const T* __restrict__ grad, const T* __restrict__ pneg,
                                                            const T* __restrict__ ppos, int64_t m, T* __restrict__ viols) {
    const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const T g = grad[j];
    const T a = g - ppos[j], b = -pneg[j] - g;
    viols[j] = (a < b) ? b : a;
}

// screen-order copies for the fit kernel: g of every member from `src` (the full gradient: src[cols[a]], or a sweep of the screen
// rows: src[a]); penalties, max(H[a, a], 0) and beta of the members from position a0 on
template <class T>
__global__ __launch_bounds__(256) void pinball_gather_kernel(const int32_t* __restrict__ cols, int32_t ns, int32_t a0,
                                                             const T* __restrict__ src, int by_col, const T* __restrict__ pneg,
                                                             const T* __restrict__ ppos, const T* __restrict__ H, int64_t ld,
                                                             const T* __restrict__ beta, T* __restrict__ g_s,
                                                             T* __restrict__ lower_s, T* __restrict__ upper_s,
                                                             T* __restrict__ vars_s, T* __restrict__ beta_s) {
    const int32_t a = int32_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a >= ns) return;
    const int64_t j = cols[a];
    g_s[a] = by_col ? src[j] : src[a];
    if (a >= a0) {
        lower_s[a] = pneg[j];
        upper_s[a] = ppos[j];
        const T h = H[int64_t(a) + int64_t(a) * ld];
        vars_s[a] = (h < T(0)) ? T(0) : h; // std::max(h, 0)
        beta_s[a] = beta[j];
    }
}

} // namespace

template <class T>
void launch_ptq(const T* P, int64_t ldp, const int32_t* pcols, int32_t M, const T* Q, int64_t ldq, const int32_t* qcols, int32_t N,
                int64_t K, T* C, int64_t ldc, hipStream_t s) {
    if (M <= 0 || N <= 0) return;
    const unsigned gy_max = 65535;
    const unsigned gx = cd_blocks_for(M, kTile);
    // (the grid's second dimension is limited: the columns go in slabs)
    for (int64_t c0 = 0; c0 < N; c0 += int64_t(gy_max) * kTile) {
        const int32_t nc = int32_t(std::min<int64_t>(int64_t(gy_max) * kTile, N - c0));
        hipLaunchKernelGGL((ptq_kernel<T>), dim3(gx, cd_blocks_for(nc, kTile)), dim3(kTile, kTile), 0, s, P, ldp, pcols, M,
                           qcols ? Q : Q + c0 * ldq, ldq, qcols ? qcols + c0 : nullptr, nc, K, C + c0 * ldc, ldc);
    }
}
template void launch_ptq<float>(const float*, int64_t, const int32_t*, int32_t, const float*, int64_t, const int32_t*, int32_t,
                                int64_t, float*, int64_t, hipStream_t);
template void launch_ptq<double>(const double*, int64_t, const int32_t*, int32_t, const double*, int64_t, const int32_t*, int32_t,
                                 int64_t, double*, int64_t, hipStream_t);

} // namespace ahip

using namespace ahip;

struct adelie_hip_pinball_result : CdScreenResult { // n = d, p = m
    std::vector<char> asat_diag; // of dtype
    // the compact rows A_S S, (d, ns) column-major = (ns, d) row-major, left on the device until somebody asks
    void* as_dev = nullptr;
    size_t as_bytes = 0;
    ~adelie_hip_pinball_result() override {
        if (as_dev && !DevPool::give(as_dev, as_bytes)) (void)hipFree(as_dev);
    }
    int64_t extra_size(int which) const override {
        if (which == ADELIE_HIP_PINBALL_SCREEN_ASAT_DIAG) return int64_t(screen_set.size());
        if (which == ADELIE_HIP_PINBALL_SCREEN_AS) return as_dev ? int64_t(screen_set.size()) * n : 0;
        return -1;
    }
    void extra_copy(int which, void* out, size_t m, size_t es) const override {
        if (which == ADELIE_HIP_PINBALL_SCREEN_ASAT_DIAG) {
            std::memcpy(out, asat_diag.data(), m * es);
        } else {
            AHIP_CHECK(hipSetDevice(device));
            AHIP_CHECK(hipMemcpy(out, as_dev, m * es, hipMemcpyDeviceToHost));
        }
    }
};

static_assert(ADELIE_HIP_PINBALL_BETA == CDS_BETA && ADELIE_HIP_PINBALL_RESID == CDS_RESID && ADELIE_HIP_PINBALL_GRAD == CDS_GRAD &&
                  ADELIE_HIP_PINBALL_SCREEN_SET == CDS_SCREEN_SET && ADELIE_HIP_PINBALL_ACTIVE_SET == CDS_ACTIVE_SET &&
                  ADELIE_HIP_PINBALL_IS_SCREEN == CDS_IS_SCREEN && ADELIE_HIP_PINBALL_IS_ACTIVE == CDS_IS_ACTIVE &&
                  ADELIE_HIP_PINBALL_SCREEN_ASAT_DIAG > CDS_IS_ACTIVE && ADELIE_HIP_PINBALL_SCREEN_AS > CDS_IS_ACTIVE,
              "the shared result vectors");
static_assert(ADELIE_HIP_PINBALL_LOSS == CDS_LOSS && ADELIE_HIP_PINBALL_ITERS == CDS_ITERS && ADELIE_HIP_PINBALL_N_KKT == CDS_N_KKT &&
                  ADELIE_HIP_PINBALL_SCREEN_SET_SIZE == CDS_SCREEN_SET_SIZE &&
                  ADELIE_HIP_PINBALL_ACTIVE_SET_SIZE == CDS_ACTIVE_SET_SIZE && ADELIE_HIP_PINBALL_TOTAL_TIME == CDS_TOTAL_TIME &&
                  ADELIE_HIP_PINBALL_T_SWEEP_MS == CDS_T_SWEEP_MS && ADELIE_HIP_PINBALL_T_GRAM_MS == CDS_T_GRAM_MS &&
                  ADELIE_HIP_PINBALL_T_FIT_MS == CDS_T_FIT_MS && ADELIE_HIP_PINBALL_N_CHANGED == CDS_N_CHANGED,
              "the shared result scalars");

namespace {

// what the shared driver (cd_screen_driver.hpp) does not know.  A is (m, d) and the handle the (d, m) column-major A', so the
// driver's n is d and its p is m; its G is H.
template <class T>
struct PinballSolver : CdScreenDriver<T, PinballSolver<T>, adelie_hip_pinball_args> {
    using Base = CdScreenDriver<T, PinballSolver<T>, adelie_hip_pinball_args>;
    using Base::a, Base::s, Base::Xv, Base::timer, Base::ns, Base::ld;
    using Base::d_r, Base::d_grad, Base::d_viols, Base::d_beta, Base::d_cols, Base::d_dcol, Base::d_dlt, Base::d_cnt, Base::d_g;
    using Base::d_lower_s, Base::d_upper_s, Base::d_vars_s, Base::d_beta_s, Base::d_G, Base::d_work_sweep;
    using Rule = PinballRule<T>;
    static constexpr const char* kName = "pinball";
    static double gram_limit_mb() { return g_pinball_gram_limit_mb; }
    static int64_t lds_max_ns() { return g_pinball_lds_max_ns; }

    adelie_hip_pinball_result* pres;
    const int64_t d, m;
    const bool sparse; // A is kept sparse: Xv is null and stays unused
    DevBuf<T> d_S, d_ST, d_pneg, d_ppos, d_AS;

    PinballSolver(adelie_hip_design* A, const adelie_hip_pinball_args* a_, adelie_hip_pinball_result* r)
        : Base(A, a_, r), pres(r), d(A->n), m(A->p), sparse(A->is_csc()) {}

    void upload() {
        d_S.reserve(size_t(d) * size_t(d)), d_pneg.reserve(size_t(m)), d_ppos.reserve(size_t(m));
        d_S.upload(static_cast<const T*>(a->S), size_t(d) * size_t(d), s);
        d_r.upload(static_cast<const T*>(a->resid), size_t(d), s);
        d_beta.upload(static_cast<const T*>(a->beta), size_t(m), s);
        d_pneg.upload(static_cast<const T*>(a->penalty_neg), size_t(m), s);
        d_ppos.upload(static_cast<const T*>(a->penalty_pos), size_t(m), s);
        if (sparse) { // S' for the rows-times-S kernel, whose lanes run along a row of S
            d_ST.reserve(size_t(d) * size_t(d));
            launch_transpose_square<T>(d_S.p, d, d_ST.p, s);
        }
    }
    void grow_extra(size_t c, size_t keep) { d_AS.grow(c * size_t(d), keep * size_t(d), s); }
    // out[c] = A[col(c), :] . resid
    void sweep(const int32_t* cols, int64_t ncols, T* out) {
        timer.begin(PH_SWEEP, s);
        if (sparse) {
            T* work = d_work_sweep.reserve(size_t(sweep_work_elems_csc(Base::X->sp_parts(), ncols)));
            launch_sweep_csc<T>(Base::X->template csc<T>(), d_r.p, out, 0, ncols, cols, nullptr, nullptr, false, work, s);
        } else {
            T* work = d_work_sweep.reserve(size_t(sweep_work_elems(d, ncols)));
            launch_sweep<T>(Xv, d_r.p, out, 0, ncols, cols, nullptr, nullptr, false, work, s);
        }
        timer.end(s);
    }
    void viols() {
        hipLaunchKernelGGL((pinball_viols_kernel<T>), dim3(cd_blocks_for(m, 256)), dim3(256), 0, s, d_grad.p, d_pneg.p, d_ppos.p, m,
                           d_viols.p);
    }
    // the rows [ns_old, ns_new) of AS, then the columns [ns_old, ns_new) of H for all members and its rows [ns_old, ns_new)
    // for the old ones
    void extend(int64_t ns_old, int64_t ns_new) {
        const int64_t N = ns_new - ns_old;
        if (N <= 0) return;
        timer.begin(PH_GRAM, s);
        if (sparse) {
            const CscView<T> Av = Base::X->template csc<T>();
            launch_csc_rows_dense<T>(Av, d_cols.p + ns_old, N, d_ST.p, d_AS.p + ns_old * d, d, s);
            launch_csc_rows_cols<T>(Av, d_cols.p, ns_new, d_AS.p + ns_old * d, d, N, d_G.p + ns_old * ld, ld, s);
            if (ns_old > 0) launch_csc_rows_cols<T>(Av, d_cols.p + ns_old, N, d_AS.p, d, ns_old, d_G.p + ns_old, ld, s);
            timer.end(s);
            return;
        }
        launch_ptq<T>(d_S.p, d, nullptr, int32_t(d), Xv.X, Xv.ld, d_cols.p + ns_old, int32_t(N), d, d_AS.p + ns_old * d, d, s);
        launch_ptq<T>(Xv.X, Xv.ld, d_cols.p, int32_t(ns_new), d_AS.p + ns_old * d, d, nullptr, int32_t(N), d, d_G.p + ns_old * ld,
                      ld, s);
        if (ns_old > 0)
            launch_ptq<T>(Xv.X, Xv.ld, d_cols.p + ns_old, int32_t(N), d_AS.p, d, nullptr, int32_t(ns_old), d, d_G.p + ns_old, ld, s);
        timer.end(s);
    }
    void gather(int64_t a0, const T* src, bool by_col) {
        hipLaunchKernelGGL((pinball_gather_kernel<T>), dim3(cd_blocks_for(ns, 256)), dim3(256), 0, s, d_cols.p, int32_t(ns),
                           int32_t(a0), src, by_col ? 1 : 0, d_pneg.p, d_ppos.p, d_G.p, ld, d_beta.p, d_g.p, d_lower_s.p,
                           d_upper_s.p, d_vars_s.p, d_beta_s.p);
    }
    const int32_t* dcol_src() { return nullptr; } // the compact list names a member by its position: a column of the compact AS
    // resid -= sum_k del_k AS[k, :]
    void catch_up() { launch_axpy_cols<T>(DenseView<T>{d_AS.p, d, ns, d}, d_dcol.p, d_dlt.p, d_cnt.p, 0, T(-1), d_r.p, s); }

    void finish_downloads(size_t es) {
        pres->asat_diag.resize(size_t(ns) * es);
        if (ns) AHIP_CHECK(hipMemcpyAsync(pres->asat_diag.data(), d_vars_s.p, size_t(ns) * es, hipMemcpyDeviceToHost, s));
    }
    void finish_extras() {
        if (ns > 0 && d_AS.p) { // the result takes the compact AS over
            pres->as_dev = d_AS.p;
            pres->as_bytes = d_AS.cap * sizeof(T);
            d_AS.p = nullptr;
            d_AS.cap = 0;
        }
    }
};

} // namespace

extern "C" {

int adelie_hip_pinball_solve(adelie_hip_design* A, const adelie_hip_pinball_args* a, adelie_hip_pinball_result** out) {
    return cd_screen_solve<PinballSolver>(A, a, out, [&] {
        if (!A->constraint || !(A->is_dense() || A->is_csc()))
            throw make_core_error("A must be a constraint matrix (matrix.dense(method=\"constraint\")).");
        const int64_t d = A->n, m = A->p;
        // state_pinball.ipp:15-94
        if (a->S_rows != d || a->S_cols != d) throw make_solver_error("S must be (d, d) where A is (m, d). ");
        if (a->n_penalty_neg != m) throw make_solver_error("penalty_neg must be (m,) where A is (m, d). ");
        if (a->n_penalty_pos != m) throw make_solver_error("penalty_pos must be (m,) where A is (m, d). ");
        if (a->kappa <= 0) throw make_solver_error("kappa must be > 0. ");
        if (a->tol < 0) throw make_solver_error("tol must be >= 0.");
        if (a->screen_set_size > m) throw make_solver_error("screen_set_size must be <= m where A is (m, d). ");
        if (a->n_screen_set != m) throw make_solver_error("screen_set must be (m,) where A is (m, d). ");
        if (a->n_is_screen != m) throw make_solver_error("is_screen must be (m,) where A is (m, d). ");
        if (a->n_screen_ASAT_diag != m) throw make_solver_error("screen_ASAT_diag must be (m,) where A is (m, d). ");
        if (a->screen_AS_rows != m || a->screen_AS_cols != d) throw make_solver_error("screen_AS must be (m, d) where A is (m, d). ");
        if (a->active_set_size > m) throw make_solver_error("active_set_size must be <= m where A is (m, d). ");
        if (a->n_active_set != m) throw make_solver_error("active_set must be (m,) where A is (m, d). ");
        if (a->n_is_active != m) throw make_solver_error("is_active must be (m,) where A is (m, d). ");
        if (a->n_beta != m) throw make_solver_error("beta must be (m,) where A is (m, d). ");
        if (a->n_resid != d) throw make_solver_error("resid must be (d,) where A is (m, d). ");
        if (a->n_grad != m) throw make_solver_error("grad must be (m,) where A is (m, d). ");
        if (m >= (int64_t(1) << 31)) throw make_core_error("pinball: m must be below 2^31.");
        if (m <= 0 || d <= 0) throw make_core_error("pinball: A must not be empty.");
        if (!a->S || !a->penalty_neg || !a->penalty_pos || !a->beta || !a->resid || !a->grad) throw make_core_error("null argument.");
        if (a->screen_set_size < 0 || a->active_set_size < 0 || (a->screen_set_size && !a->screen_set) ||
            (a->active_set_size && !a->active_set))
            throw make_core_error("pinball: screen_set_size must be in [0, m].");
        if (const char* e = cd_screen_warm_start_error(a->screen_set, a->screen_set_size, a->active_set, a->active_set_size, m,
                                                       "pinball: screen_set must hold distinct indices in [0, m).",
                                                       "pinball: active_set must hold distinct members of screen_set."))
            throw make_core_error(e);
    });
}

int adelie_hip_pinball_result_destroy(adelie_hip_pinball_result* r) {
    if (r && r->as_dev) (void)hipSetDevice(r->device);
    delete r;
    return 0;
}

int64_t adelie_hip_pinball_result_size(const adelie_hip_pinball_result* r, int which) { return cd_result_size(r, which); }
int adelie_hip_pinball_result_copy(const adelie_hip_pinball_result* r, int which, void* out, int64_t cap) {
    return cd_result_copy(r, which, out, cap);
}
double adelie_hip_pinball_result_scalar(const adelie_hip_pinball_result* r, int which) { return cd_result_scalar(r, which); }
const char* adelie_hip_pinball_result_error(const adelie_hip_pinball_result* r) { return r ? r->error.c_str() : ""; }

} // extern "C"

