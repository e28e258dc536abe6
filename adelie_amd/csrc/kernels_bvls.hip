// kernels_bvls.hip — bounded-variable least squares on a resident dense design (adelie.solver.bvls: solver_bvls.hpp,
// state_bvls.ipp).  Kernels, the host driver and the C-ABI entry points of adelie_hip_bvls_solve.
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
// Synchronisation inside the fit kernel, which this solver shares with the pinball one: cd_fit_body.hpp.
#include <cmath>
#include <limits>
#include <numeric>

#include "common.hpp"
#include "cd_fit_body.hpp"

namespace ahip {
void set_last_error(const std::string& s); // design.hip

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
using BvlsRec = CdFitRec;
template <class T> using BvlsFitArgs = CdFitArgs<T>;
enum { BVLS_OK = CD_FIT_OK, BVLS_MAX_ITERS = CD_FIT_MAX_ITERS };


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

struct adelie_hip_bvls_result {
    int dtype = ADELIE_HIP_F64, device = 0;
    int64_t n = 0, p = 0;
    std::vector<char> beta, resid, grad; // of dtype
    std::vector<int64_t> screen_set, active_set;
    std::vector<uint8_t> is_screen, is_active;
    double loss = 0;
    int64_t iters = 0, n_kkt = 0, n_changed = 0;
    double total_time = 0, t_sweep_ms = 0, t_gram_ms = 0, t_fit_ms = 0;
    std::string error;
};

namespace {

template <class T>
struct BvlsSolver {
    adelie_hip_design* X;
    adelie_hip_bvls_result* res;
    const adelie_hip_bvls_args* a;
    int64_t n, p;
    hipStream_t s;
    DenseView<T> Xv;
    DeferredFrees deferred;
    PhaseTimer timer;

    // full vectors
    DevBuf<T> d_w, d_r, d_v, d_grad, d_viols, d_beta, d_lower, d_upper, d_vars;
    // screen order
    DevBuf<int32_t> d_cols, d_act, d_dcol, d_cnt;
    DevBuf<T> d_g, d_lower_s, d_upper_s, d_vars_s, d_beta_s, d_dlt, d_sweep_out;
    DevBuf<T> d_G, d_work_sweep, d_work_gram;
    DevBuf<char> d_scratch;
    DevBuf<BvlsRec> d_rec;
    int64_t ld = 0;
    size_t cap_s = 0; // capacity of the screen-order buffers

    std::vector<int64_t> screen_set, active_pos;
    std::vector<uint8_t> is_screen;
    std::vector<int32_t> h_cols;
    std::vector<T> h_viols;
    bool have_viols = false;
    int64_t ns = 0;
    int lds_limit = 0;
    bool attr_done = false;

    T loss;
    int64_t iters = 0, n_kkt = 0, nact = 0;

    BvlsSolver(adelie_hip_design* X_, const adelie_hip_bvls_args* a_, adelie_hip_bvls_result* r) : X(X_), res(r), a(a_) {
        n = X->n;
        p = X->p;
        s = X->stream;
        Xv = X->dense<T>();
        loss = T(a->loss);
    }

    // grow the screen-order buffers to hold `want` members, keeping the first `keep`
    void reserve_screen(int64_t want, int64_t keep) {
        if (size_t(want) <= cap_s) return;
        size_t c = std::max<size_t>(size_t(want), cap_s + cap_s / 2);
        c = std::min<size_t>(std::max<size_t>(c, 64), size_t(p));
        c = std::max<size_t>(c, size_t(want));
        d_cols.grow(c, size_t(keep), s);
        d_act.grow(c, size_t(keep), s);
        d_lower_s.grow(c, size_t(keep), s);
        d_upper_s.grow(c, size_t(keep), s);
        d_vars_s.grow(c, size_t(keep), s);
        d_beta_s.grow(c, size_t(keep), s);
        d_g.reserve(c), d_dcol.reserve(c), d_dlt.reserve(c), d_sweep_out.reserve(c);
        cap_s = c;
    }
    // the Gram matrix for ns_new members: false when it would pass the limit
    bool reserve_gram(int64_t ns_new, int64_t ns_old) {
        if (double(ns_new) * double(ns_new) * double(sizeof(T)) > g_bvls_gram_limit_mb * 1048576.0) return false;
        if (ns_new <= ld) return true;
        int64_t nl = std::max<int64_t>(std::max<int64_t>(ns_new, ld + ld / 2), 64);
        nl = std::min<int64_t>(nl, std::max<int64_t>(p, ns_new));
        if (double(nl) * double(nl) * double(sizeof(T)) > g_bvls_gram_limit_mb * 1048576.0) nl = ns_new;
        DevBuf<T> ng;
        ng.reserve(size_t(nl) * size_t(nl));
        if (ns_old > 0)
            AHIP_CHECK(hipMemcpy2DAsync(ng.p, size_t(nl) * sizeof(T), d_G.p, size_t(ld) * sizeof(T), size_t(ns_old) * sizeof(T),
                                        size_t(ns_old), hipMemcpyDeviceToDevice, s));
        std::swap(ng.p, d_G.p);
        std::swap(ng.cap, d_G.cap);
        ng.release(); // (kept until the end of the solve: DeferredFrees)
        ld = nl;
        return true;
    }
    void vmul_sweep(const int32_t* cols, int64_t ncols, T* out) {
        timer.begin(PH_SWEEP, s);
        launch_vmul<T>(d_w.p, d_r.p, d_v.p, n, s);
        T* work = d_work_sweep.reserve(size_t(sweep_work_elems(n, ncols)));
        launch_sweep<T>(Xv, d_v.p, out, 0, ncols, cols, nullptr, nullptr, false, work, s);
        timer.end(s);
    }
    // rows and columns [ns_old, ns_new) of G
    void extend_gram(int64_t ns_old, int64_t ns_new) {
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

    void fit(BvlsRec* h_rec) {
        BvlsFitArgs<T> fa;
        fa.G = d_G.p, fa.ld = ld, fa.ns = int32_t(ns), fa.cols = d_cols.p;
        fa.lower_s = d_lower_s.p, fa.upper_s = d_upper_s.p, fa.vars_s = d_vars_s.p, fa.g_s = d_g.p, fa.beta_s = d_beta_s.p;
        fa.act = d_act.p, fa.beta_full = d_beta.p, fa.dcol = d_dcol.p, fa.dlt = d_dlt.p, fa.cnt_dev = d_cnt.p, fa.rec = d_rec.p;
        fa.max_iters = a->max_iters;
        fa.dcol_src = d_cols.p;
        fa.tol_yvar = T(a->tol) * T(a->y_var);
        h_rec->loss = double(loss), h_rec->iters = iters, h_rec->n_visits_changed = 0, h_rec->status = 0;
        h_rec->n_active = int32_t(nact), h_rec->n_changed = 0, h_rec->pad = 0;
        AHIP_CHECK(hipMemcpyAsync(d_rec.p, h_rec, sizeof(BvlsRec), hipMemcpyHostToDevice, s));
        timer.begin(PH_FIT, s);
        launch_cd_fit<T, BvlsRule<T>>(fa, lds_limit, g_bvls_lds_max_ns, d_scratch, attr_done, s);
        timer.end(s);
        // r -= X * delta
        launch_axpy_cols<T>(Xv, d_dcol.p, d_dlt.p, d_cnt.p, 0, T(-1), d_r.p, s);
        AHIP_CHECK(hipMemcpyAsync(h_rec, d_rec.p, sizeof(BvlsRec), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
        AHIP_CHECK(hipGetLastError());
        timer.collect();
        loss = T(h_rec->loss);
        iters = h_rec->iters;
        nact = h_rec->n_active;
        res->n_changed += h_rec->n_visits_changed;
    }

    void finish() {
        AHIP_CHECK(hipStreamSynchronize(s));
        timer.collect();
        const size_t es = sizeof(T);
        res->beta.resize(size_t(p) * es), res->resid.resize(size_t(n) * es), res->grad.resize(size_t(p) * es);
        if (p) AHIP_CHECK(hipMemcpyAsync(res->beta.data(), d_beta.p, size_t(p) * es, hipMemcpyDeviceToHost, s));
        if (n) AHIP_CHECK(hipMemcpyAsync(res->resid.data(), d_r.p, size_t(n) * es, hipMemcpyDeviceToHost, s));
        std::vector<int32_t> hact(static_cast<size_t>(nact));
        if (nact) AHIP_CHECK(hipMemcpyAsync(hact.data(), d_act.p, size_t(nact) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
        AHIP_CHECK(hipGetLastError());
        if (have_viols) std::memcpy(res->grad.data(), h_viols.data(), size_t(p) * es);
        else if (p) std::memcpy(res->grad.data(), a->grad, size_t(p) * es);
        res->screen_set = screen_set;
        res->is_screen = is_screen;
        res->active_set.resize(size_t(nact));
        res->is_active.assign(size_t(p), 0);
        for (int64_t i = 0; i < nact; ++i) {
            const int64_t j = screen_set[size_t(hact[size_t(i)])];
            res->active_set[size_t(i)] = j;
            res->is_active[size_t(j)] = 1;
        }
        res->loss = double(loss);
        res->iters = iters;
        res->n_kkt = n_kkt;
        res->t_sweep_ms = timer.ms[PH_SWEEP], res->t_gram_ms = timer.ms[PH_GRAM], res->t_fit_ms = timer.ms[PH_FIT];
    }

    void run() {
        DeferredFrees::Scope scope(&deferred);
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, X->device) != hipSuccess || v <= 0) {
            (void)hipGetLastError();
            v = 65536;
        }
        lds_limit = v;
        d_w.reserve(size_t(n)), d_r.reserve(size_t(n)), d_v.reserve(size_t(n));
        d_grad.reserve(size_t(p)), d_viols.reserve(size_t(p)), d_beta.reserve(size_t(p));
        d_lower.reserve(size_t(p)), d_upper.reserve(size_t(p)), d_vars.reserve(size_t(p));
        d_cnt.reserve(4), d_rec.reserve(1);
        d_w.upload(static_cast<const T*>(a->weights), size_t(n), s);
        d_r.upload(static_cast<const T*>(a->resid), size_t(n), s);
        d_beta.upload(static_cast<const T*>(a->beta), size_t(p), s);
        d_lower.upload(static_cast<const T*>(a->lower), size_t(p), s);
        d_upper.upload(static_cast<const T*>(a->upper), size_t(p), s);
        d_vars.upload(static_cast<const T*>(a->X_vars), size_t(p), s);
        h_viols.resize(size_t(p));
        is_screen.assign(size_t(p), 0);
        Pinned pin(sizeof(BvlsRec));
        BvlsRec* h_rec = static_cast<BvlsRec*>(pin.p);

        // the caller's screen and active sets (a warm start)
        std::vector<int64_t> pos_of;
        if (a->screen_set_size > 0) pos_of.assign(size_t(p), -1);
        for (int64_t i = 0; i < a->screen_set_size; ++i) {
            const int64_t j = a->screen_set[i];
            screen_set.push_back(j);
            is_screen[size_t(j)] = 1;
            pos_of[size_t(j)] = i;
        }
        ns = int64_t(screen_set.size());
        nact = a->active_set_size;
        if (ns > 0) {
            reserve_screen(ns, 0);
            h_cols.assign(screen_set.begin(), screen_set.end());
            d_cols.upload(h_cols.data(), size_t(ns), s);
            std::vector<int32_t> hact(static_cast<size_t>(nact));
            for (int64_t i = 0; i < nact; ++i) hact[size_t(i)] = int32_t(pos_of[size_t(a->active_set[i])]);
            if (nact) d_act.upload(hact.data(), size_t(nact), s);
            AHIP_CHECK(hipStreamSynchronize(s)); // (hact / h_cols are read by the copies)
            if (!reserve_gram(ns, 0)) return gram_limit_error(ns);
            extend_gram(0, ns);
            vmul_sweep(d_cols.p, ns, d_sweep_out.p);
            gather(0, d_sweep_out.p, false);
            AHIP_CHECK(hipStreamSynchronize(s)); // (hact / h_cols are read by the copies)
        }

        while (true) { // solve(): solver_bvls.hpp:329-347
            const T loss_prev = loss;
            if (ns > 0) {
                fit(h_rec);
                if (h_rec->status == BVLS_MAX_ITERS) {
                    res->error = "adelie_core solver: bvls: max iterations reached!";
                    return finish();
                }
            } else { // an empty screen pass
                ++iters;
                if (iters >= a->max_iters) {
                    res->error = "adelie_core solver: bvls: max iterations reached!";
                    return finish();
                }
            }
            if (n_kkt > 0 && double(std::abs(loss - loss_prev)) < 1e-6 * double(std::abs(T(a->y_var)))) return finish();
            // kkt_screen(): :229-304
            ++n_kkt;
            vmul_sweep(nullptr, p, d_grad.p);
            hipLaunchKernelGGL((bvls_viols_kernel<T>), dim3(cd_blocks_for(p, 256)), dim3(256), 0, s, d_grad.p, d_beta.p, d_lower.p,
                               d_upper.p, p, d_viols.p);
            AHIP_CHECK(hipMemcpyAsync(h_viols.data(), d_viols.p, size_t(p) * sizeof(T), hipMemcpyDeviceToHost, s));
            AHIP_CHECK(hipStreamSynchronize(s));
            AHIP_CHECK(hipGetLastError());
            timer.collect();
            have_viols = true;
            std::vector<int64_t> order(static_cast<size_t>(p));
            std::iota(order.begin(), order.end(), int64_t(0));
            std::stable_sort(order.begin(), order.end(),
                             [&](int64_t i, int64_t j) { return h_viols[size_t(i)] > h_viols[size_t(j)]; });
            std::vector<int64_t> added;
            bool kkt_passed = true;
            for (int64_t t = 0; t < p; ++t) {
                const int64_t k = order[size_t(t)];
                if (is_screen[size_t(k)] || h_viols[size_t(k)] <= T(0)) continue;
                kkt_passed = false;
                if (int64_t(added.size()) >= a->kappa) break;
                added.push_back(k);
            }
            if (kkt_passed) return finish();
            const int64_t ns_old = ns, ns_new = ns + int64_t(added.size());
            if (!reserve_gram(ns_new, ns_old)) return gram_limit_error(ns_new);
            reserve_screen(ns_new, ns_old);
            for (int64_t k : added) {
                screen_set.push_back(k);
                is_screen[size_t(k)] = 1;
            }
            h_cols.assign(added.begin(), added.end());
            d_cols.upload(h_cols.data(), h_cols.size(), s, size_t(ns_old));
            ns = ns_new;
            extend_gram(ns_old, ns_new);
            gather(ns_old, d_grad.p, true);
            AHIP_CHECK(hipStreamSynchronize(s)); // (h_cols is read by the copy)
        }
    }
    void gram_limit_error(int64_t ns_want) {
        res->error = "adelie_core solver: bvls: screen set of " + std::to_string(ns_want) +
                     " coordinates exceeds the device Gram limit";
        finish();
    }
};

template <class T>
void bvls_run(adelie_hip_design* X, const adelie_hip_bvls_args* a, adelie_hip_bvls_result* res) {
    BvlsSolver<T> sv(X, a, res);
    try {
        sv.run();
    } catch (...) {
        (void)hipStreamSynchronize(X->stream); // the buffers are parked by the destructors
        throw;
    }
}

} // namespace

extern "C" {

int adelie_hip_bvls_solve(adelie_hip_design* X, const adelie_hip_bvls_args* a, adelie_hip_bvls_result** out) {
    adelie_hip_bvls_result* res = nullptr;
    try {
        if (!X || !a || !out) throw make_core_error("null argument.");
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
        {   // distinct members in range; the active set inside the screen set (what the solver itself maintains)
            std::vector<uint8_t> seen(size_t(p), 0);
            for (int64_t i = 0; i < a->screen_set_size; ++i) {
                const int64_t j = a->screen_set[i];
                if (j < 0 || j >= p || seen[size_t(j)]) throw make_core_error("bvls: screen_set must hold distinct indices in [0, p).");
                seen[size_t(j)] = 1;
            }
            for (int64_t i = 0; i < a->active_set_size; ++i) {
                const int64_t j = a->active_set[i];
                if (j < 0 || j >= p || seen[size_t(j)] != 1)
                    throw make_core_error("bvls: active_set must hold distinct members of screen_set.");
                seen[size_t(j)] = 2;
            }
        }
        AHIP_CHECK(hipSetDevice(X->device));
        res = new adelie_hip_bvls_result;
        res->dtype = X->dtype;
        res->device = X->device;
        res->n = n;
        res->p = p;
        const auto t0 = std::chrono::steady_clock::now();
        if (X->dtype == ADELIE_HIP_F64) bvls_run<double>(X, a, res);
        else bvls_run<float>(X, a, res);
        res->total_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *out = res;
    } catch (const std::exception& e) {
        delete res;
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

int adelie_hip_bvls_result_destroy(adelie_hip_bvls_result* r) {
    delete r;
    return 0;
}

int64_t adelie_hip_bvls_result_size(const adelie_hip_bvls_result* r, int which) {
    if (!r) return -1;
    switch (which) {
        case ADELIE_HIP_BVLS_BETA:
        case ADELIE_HIP_BVLS_GRAD:
        case ADELIE_HIP_BVLS_IS_SCREEN:
        case ADELIE_HIP_BVLS_IS_ACTIVE: return r->p;
        case ADELIE_HIP_BVLS_RESID: return r->n;
        case ADELIE_HIP_BVLS_SCREEN_SET: return int64_t(r->screen_set.size());
        case ADELIE_HIP_BVLS_ACTIVE_SET: return int64_t(r->active_set.size());
    }
    return -1;
}

int adelie_hip_bvls_result_copy(const adelie_hip_bvls_result* r, int which, void* out, int64_t cap) {
    try {
        const int64_t size = adelie_hip_bvls_result_size(r, which);
        if (size < 0 || !out) throw make_core_error("unknown result vector.");
        const size_t m = size_t(std::min(size, cap));
        const size_t es = r->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
        if (!m) return 0;
        switch (which) {
            case ADELIE_HIP_BVLS_BETA: std::memcpy(out, r->beta.data(), m * es); break;
            case ADELIE_HIP_BVLS_RESID: std::memcpy(out, r->resid.data(), m * es); break;
            case ADELIE_HIP_BVLS_GRAD: std::memcpy(out, r->grad.data(), m * es); break;
            case ADELIE_HIP_BVLS_SCREEN_SET: std::memcpy(out, r->screen_set.data(), m * sizeof(int64_t)); break;
            case ADELIE_HIP_BVLS_ACTIVE_SET: std::memcpy(out, r->active_set.data(), m * sizeof(int64_t)); break;
            case ADELIE_HIP_BVLS_IS_SCREEN: std::memcpy(out, r->is_screen.data(), m); break;
            case ADELIE_HIP_BVLS_IS_ACTIVE: std::memcpy(out, r->is_active.data(), m); break;
        }
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

double adelie_hip_bvls_result_scalar(const adelie_hip_bvls_result* r, int which) {
    if (!r) return 0;
    switch (which) {
        case ADELIE_HIP_BVLS_LOSS: return r->loss;
        case ADELIE_HIP_BVLS_ITERS: return double(r->iters);
        case ADELIE_HIP_BVLS_N_KKT: return double(r->n_kkt);
        case ADELIE_HIP_BVLS_SCREEN_SET_SIZE: return double(r->screen_set.size());
        case ADELIE_HIP_BVLS_ACTIVE_SET_SIZE: return double(r->active_set.size());
        case ADELIE_HIP_BVLS_TOTAL_TIME: return r->total_time;
        case ADELIE_HIP_BVLS_T_SWEEP_MS: return r->t_sweep_ms;
        case ADELIE_HIP_BVLS_T_GRAM_MS: return r->t_gram_ms;
        case ADELIE_HIP_BVLS_T_FIT_MS: return r->t_fit_ms;
        case ADELIE_HIP_BVLS_N_CHANGED: return double(r->n_changed);
    }
    return 0;
}

const char* adelie_hip_bvls_result_error(const adelie_hip_bvls_result* r) { return r ? r->error.c_str() : ""; }

} // extern "C"
