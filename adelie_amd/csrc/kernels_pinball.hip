// kernels_pinball.hip — pinball least squares on a resident constraint matrix (adelie.solver.pinball: solver_pinball.hpp,
// state_pinball.ipp).  Kernels, the host driver and the C-ABI entry points of adelie_hip_pinball_solve.
//
//     minimise over beta in R^m   1/2 || S^{-1/2} v - S^{1/2} A' beta ||^2 + penalty_neg' beta_- + penalty_pos' beta_+
//
// The handle holds A (m, d) row-major, i.e. the (d, m) column-major matrix A' of a dense design: the full gradient A resid is
// launch_sweep over the m columns, a row of A is one contiguous column.
//
// The reference visits one coordinate at a time and pays a d-long dot per visit (rvmul for the gradient) plus a d-long update
// of the residual when the visit changes the coefficient.  Here the gradient g_a = A[a, :] . resid of EVERY screen coordinate
// is kept current through the resident matrix H = A_S S A_S' (ns x ns, both triangles computed, H[a, k] = A[a, :] . (A[k, :] S)):
// a visit that changes beta_k by `del` does g_a -= H[a, k] * del for all a (one contiguous column of H), and a visit that
// changes nothing touches no memory but a few broadcast reads.  One workgroup runs a whole fit() without leaving the compute
// unit: the kernel is the one bvls runs (cd_fit_body.hpp, which also describes its synchronisation) with the pinball update
// (solver_pinball.hpp:37-61) and prune predicate (beta == 0).  The residual is caught up once per fit from the compact list of
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
#include <cmath>
#include <limits>
#include <numeric>

#include "common.hpp"
#include "cd_fit_body.hpp"

namespace ahip {
void set_last_error(const std::string& s); // design.hip

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

struct adelie_hip_pinball_result {
    int dtype = ADELIE_HIP_F64, device = 0;
    int64_t m = 0, d = 0;
    std::vector<char> beta, resid, grad, asat_diag; // of dtype
    std::vector<int64_t> screen_set, active_set;
    std::vector<uint8_t> is_screen, is_active;
    // the compact rows A_S S, (d, ns) column-major = (ns, d) row-major, left on the device until somebody asks
    void* as_dev = nullptr;
    size_t as_bytes = 0;
    double loss = 0;
    int64_t iters = 0, n_kkt = 0, n_changed = 0;
    double total_time = 0, t_sweep_ms = 0, t_gram_ms = 0, t_fit_ms = 0;
    std::string error;
    ~adelie_hip_pinball_result() {
        if (as_dev && !DevPool::give(as_dev, as_bytes)) (void)hipFree(as_dev);
    }
};

namespace {

template <class T>
struct PinballSolver {
    adelie_hip_design* X;
    adelie_hip_pinball_result* res;
    const adelie_hip_pinball_args* a;
    int64_t d, m; // A is (m, d); the handle is the (d, m) column-major A'
    hipStream_t s;
    DenseView<T> Av;
    DeferredFrees deferred;
    PhaseTimer timer;

    // full vectors
    DevBuf<T> d_S, d_r, d_grad, d_viols, d_beta, d_pneg, d_ppos;
    // screen order
    DevBuf<int32_t> d_cols, d_act, d_dcol, d_cnt;
    DevBuf<T> d_g, d_lower_s, d_upper_s, d_vars_s, d_beta_s, d_dlt, d_sweep_out;
    DevBuf<T> d_AS, d_H, d_work_sweep;
    DevBuf<char> d_scratch;
    DevBuf<CdFitRec> d_rec;
    int64_t ld = 0;
    size_t cap_s = 0; // capacity of the screen-order buffers (members)

    std::vector<int64_t> screen_set;
    std::vector<uint8_t> is_screen;
    std::vector<int32_t> h_cols;
    std::vector<T> h_viols;
    bool have_viols = false;
    int64_t ns = 0;
    int lds_limit = 0;
    bool attr_done = false;

    T loss;
    int64_t iters = 0, n_kkt = 0, nact = 0;

    PinballSolver(adelie_hip_design* X_, const adelie_hip_pinball_args* a_, adelie_hip_pinball_result* r) : X(X_), res(r), a(a_) {
        d = X->n;
        m = X->p;
        s = X->stream;
        Av = X->dense<T>();
        loss = T(a->loss);
    }

    // grow the screen-order buffers to hold `want` members, keeping the first `keep`
    void reserve_screen(int64_t want, int64_t keep) {
        if (size_t(want) <= cap_s) return;
        size_t c = std::max<size_t>(size_t(want), cap_s + cap_s / 2);
        c = std::min<size_t>(std::max<size_t>(c, 64), size_t(m));
        c = std::max<size_t>(c, size_t(want));
        d_cols.grow(c, size_t(keep), s);
        d_act.grow(c, size_t(keep), s);
        d_lower_s.grow(c, size_t(keep), s);
        d_upper_s.grow(c, size_t(keep), s);
        d_vars_s.grow(c, size_t(keep), s);
        d_beta_s.grow(c, size_t(keep), s);
        d_AS.grow(c * size_t(d), size_t(keep) * size_t(d), s);
        d_g.reserve(c), d_dcol.reserve(c), d_dlt.reserve(c), d_sweep_out.reserve(c);
        cap_s = c;
    }
    // H for ns_new members: false when it would pass the limit
    bool reserve_gram(int64_t ns_new, int64_t ns_old) {
        if (double(ns_new) * double(ns_new) * double(sizeof(T)) > g_pinball_gram_limit_mb * 1048576.0) return false;
        if (ns_new <= ld) return true;
        int64_t nl = std::max<int64_t>(std::max<int64_t>(ns_new, ld + ld / 2), 64);
        nl = std::min<int64_t>(nl, std::max<int64_t>(m, ns_new));
        if (double(nl) * double(nl) * double(sizeof(T)) > g_pinball_gram_limit_mb * 1048576.0) nl = ns_new;
        DevBuf<T> ng;
        ng.reserve(size_t(nl) * size_t(nl));
        if (ns_old > 0)
            AHIP_CHECK(hipMemcpy2DAsync(ng.p, size_t(nl) * sizeof(T), d_H.p, size_t(ld) * sizeof(T), size_t(ns_old) * sizeof(T),
                                        size_t(ns_old), hipMemcpyDeviceToDevice, s));
        std::swap(ng.p, d_H.p);
        std::swap(ng.cap, d_H.cap);
        ng.release(); // (kept until the end of the solve: DeferredFrees)
        ld = nl;
        return true;
    }
    // out[c] = A[col(c), :] . resid
    void sweep(const int32_t* cols, int64_t ncols, T* out) {
        timer.begin(PH_SWEEP, s);
        T* work = d_work_sweep.reserve(size_t(sweep_work_elems(d, ncols)));
        launch_sweep<T>(Av, d_r.p, out, 0, ncols, cols, nullptr, nullptr, false, work, s);
        timer.end(s);
    }
    // the rows [ns_old, ns_new) of AS, then the columns [ns_old, ns_new) of H for all members and its rows [ns_old, ns_new)
    // for the old ones
    void extend(int64_t ns_old, int64_t ns_new) {
        const int64_t N = ns_new - ns_old;
        if (N <= 0) return;
        timer.begin(PH_GRAM, s);
        launch_ptq<T>(d_S.p, d, nullptr, int32_t(d), Av.X, Av.ld, d_cols.p + ns_old, int32_t(N), d, d_AS.p + ns_old * d, d, s);
        launch_ptq<T>(Av.X, Av.ld, d_cols.p, int32_t(ns_new), d_AS.p + ns_old * d, d, nullptr, int32_t(N), d, d_H.p + ns_old * ld,
                      ld, s);
        if (ns_old > 0)
            launch_ptq<T>(Av.X, Av.ld, d_cols.p + ns_old, int32_t(N), d_AS.p, d, nullptr, int32_t(ns_old), d, d_H.p + ns_old, ld, s);
        timer.end(s);
    }
    void gather(int64_t a0, const T* src, bool by_col) {
        hipLaunchKernelGGL((pinball_gather_kernel<T>), dim3(cd_blocks_for(ns, 256)), dim3(256), 0, s, d_cols.p, int32_t(ns),
                           int32_t(a0), src, by_col ? 1 : 0, d_pneg.p, d_ppos.p, d_H.p, ld, d_beta.p, d_g.p, d_lower_s.p,
                           d_upper_s.p, d_vars_s.p, d_beta_s.p);
    }

    void fit(CdFitRec* h_rec) {
        CdFitArgs<T> fa;
        fa.G = d_H.p, fa.ld = ld, fa.ns = int32_t(ns), fa.cols = d_cols.p;
        fa.dcol_src = nullptr; // the compact list names a member by its position: a column of the compact AS
        fa.lower_s = d_lower_s.p, fa.upper_s = d_upper_s.p, fa.vars_s = d_vars_s.p, fa.g_s = d_g.p, fa.beta_s = d_beta_s.p;
        fa.act = d_act.p, fa.beta_full = d_beta.p, fa.dcol = d_dcol.p, fa.dlt = d_dlt.p, fa.cnt_dev = d_cnt.p, fa.rec = d_rec.p;
        fa.scratch = nullptr;
        fa.max_iters = a->max_iters;
        fa.tol_yvar = T(a->tol) * T(a->y_var);
        h_rec->loss = double(loss), h_rec->iters = iters, h_rec->n_visits_changed = 0, h_rec->status = 0;
        h_rec->n_active = int32_t(nact), h_rec->n_changed = 0, h_rec->pad = 0;
        AHIP_CHECK(hipMemcpyAsync(d_rec.p, h_rec, sizeof(CdFitRec), hipMemcpyHostToDevice, s));
        timer.begin(PH_FIT, s);
        launch_cd_fit<T, PinballRule<T>>(fa, lds_limit, g_pinball_lds_max_ns, d_scratch, attr_done, s);
        timer.end(s);
        // resid -= sum_k del_k AS[k, :]
        launch_axpy_cols<T>(DenseView<T>{d_AS.p, d, ns, d}, d_dcol.p, d_dlt.p, d_cnt.p, 0, T(-1), d_r.p, s);
        AHIP_CHECK(hipMemcpyAsync(h_rec, d_rec.p, sizeof(CdFitRec), hipMemcpyDeviceToHost, s));
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
        res->beta.resize(size_t(m) * es), res->resid.resize(size_t(d) * es), res->grad.resize(size_t(m) * es);
        res->asat_diag.resize(size_t(ns) * es);
        AHIP_CHECK(hipMemcpyAsync(res->beta.data(), d_beta.p, size_t(m) * es, hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipMemcpyAsync(res->resid.data(), d_r.p, size_t(d) * es, hipMemcpyDeviceToHost, s));
        if (ns) AHIP_CHECK(hipMemcpyAsync(res->asat_diag.data(), d_vars_s.p, size_t(ns) * es, hipMemcpyDeviceToHost, s));
        std::vector<int32_t> hact(static_cast<size_t>(nact));
        if (nact) AHIP_CHECK(hipMemcpyAsync(hact.data(), d_act.p, size_t(nact) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
        AHIP_CHECK(hipGetLastError());
        if (have_viols) std::memcpy(res->grad.data(), h_viols.data(), size_t(m) * es);
        else std::memcpy(res->grad.data(), a->grad, size_t(m) * es);
        res->screen_set = screen_set;
        res->is_screen = is_screen;
        res->active_set.resize(size_t(nact));
        res->is_active.assign(size_t(m), 0);
        for (int64_t i = 0; i < nact; ++i) {
            const int64_t j = screen_set[size_t(hact[size_t(i)])];
            res->active_set[size_t(i)] = j;
            res->is_active[size_t(j)] = 1;
        }
        if (ns > 0 && d_AS.p) { // the result takes the compact AS over
            res->as_dev = d_AS.p;
            res->as_bytes = d_AS.cap * sizeof(T);
            d_AS.p = nullptr;
            d_AS.cap = 0;
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
        d_S.reserve(size_t(d) * size_t(d)), d_r.reserve(size_t(d));
        d_grad.reserve(size_t(m)), d_viols.reserve(size_t(m)), d_beta.reserve(size_t(m));
        d_pneg.reserve(size_t(m)), d_ppos.reserve(size_t(m));
        d_cnt.reserve(4), d_rec.reserve(1);
        d_S.upload(static_cast<const T*>(a->S), size_t(d) * size_t(d), s);
        d_r.upload(static_cast<const T*>(a->resid), size_t(d), s);
        d_beta.upload(static_cast<const T*>(a->beta), size_t(m), s);
        d_pneg.upload(static_cast<const T*>(a->penalty_neg), size_t(m), s);
        d_ppos.upload(static_cast<const T*>(a->penalty_pos), size_t(m), s);
        h_viols.resize(size_t(m));
        is_screen.assign(size_t(m), 0);
        Pinned pin(sizeof(CdFitRec));
        CdFitRec* h_rec = static_cast<CdFitRec*>(pin.p);

        // the caller's screen and active sets (a warm start)
        std::vector<int64_t> pos_of;
        if (a->screen_set_size > 0) pos_of.assign(size_t(m), -1);
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
            extend(0, ns);
            sweep(d_cols.p, ns, d_sweep_out.p);
            gather(0, d_sweep_out.p, false);
            AHIP_CHECK(hipStreamSynchronize(s));
        }

        while (true) { // solve(): solver_pinball.hpp:293-308
            const T loss_prev = loss;
            if (ns > 0) {
                fit(h_rec);
                if (h_rec->status == CD_FIT_MAX_ITERS) {
                    res->error = "adelie_core solver: pinball: max iterations reached!";
                    return finish();
                }
            } else { // an empty screen pass
                ++iters;
                if (iters >= a->max_iters) {
                    res->error = "adelie_core solver: pinball: max iterations reached!";
                    return finish();
                }
            }
            if (n_kkt > 0 && double(std::abs(loss - loss_prev)) < 1e-6 * double(std::abs(T(a->y_var)))) return finish();
            // kkt_screen(): :200-276
            ++n_kkt;
            sweep(nullptr, m, d_grad.p);
            hipLaunchKernelGGL((pinball_viols_kernel<T>), dim3(cd_blocks_for(m, 256)), dim3(256), 0, s, d_grad.p, d_pneg.p, d_ppos.p,
                               m, d_viols.p);
            AHIP_CHECK(hipMemcpyAsync(h_viols.data(), d_viols.p, size_t(m) * sizeof(T), hipMemcpyDeviceToHost, s));
            AHIP_CHECK(hipStreamSynchronize(s));
            AHIP_CHECK(hipGetLastError());
            timer.collect();
            have_viols = true;
            std::vector<int64_t> order(static_cast<size_t>(m));
            std::iota(order.begin(), order.end(), int64_t(0));
            std::stable_sort(order.begin(), order.end(),
                             [&](int64_t i, int64_t j) { return h_viols[size_t(i)] > h_viols[size_t(j)]; });
            std::vector<int64_t> added;
            bool kkt_passed = true;
            for (int64_t t = 0; t < m; ++t) {
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
            extend(ns_old, ns_new);
            gather(ns_old, d_grad.p, true);
            AHIP_CHECK(hipStreamSynchronize(s)); // (h_cols is read by the copy)
        }
    }
    void gram_limit_error(int64_t ns_want) {
        res->error = "adelie_core solver: pinball: screen set of " + std::to_string(ns_want) +
                     " coordinates exceeds the device Gram limit";
        finish();
    }
};

template <class T>
void pinball_run(adelie_hip_design* X, const adelie_hip_pinball_args* a, adelie_hip_pinball_result* res) {
    PinballSolver<T> sv(X, a, res);
    try {
        sv.run();
    } catch (...) {
        (void)hipStreamSynchronize(X->stream); // the buffers are parked by the destructors
        throw;
    }
}

} // namespace

extern "C" {

int adelie_hip_pinball_solve(adelie_hip_design* A, const adelie_hip_pinball_args* a, adelie_hip_pinball_result** out) {
    adelie_hip_pinball_result* res = nullptr;
    try {
        if (!A || !a || !out) throw make_core_error("null argument.");
        if (!A->constraint || !A->is_dense())
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
        {   // distinct members in range; the active set inside the screen set (what the solver itself maintains)
            std::vector<uint8_t> seen(size_t(m), 0);
            for (int64_t i = 0; i < a->screen_set_size; ++i) {
                const int64_t j = a->screen_set[i];
                if (j < 0 || j >= m || seen[size_t(j)])
                    throw make_core_error("pinball: screen_set must hold distinct indices in [0, m).");
                seen[size_t(j)] = 1;
            }
            for (int64_t i = 0; i < a->active_set_size; ++i) {
                const int64_t j = a->active_set[i];
                if (j < 0 || j >= m || seen[size_t(j)] != 1)
                    throw make_core_error("pinball: active_set must hold distinct members of screen_set.");
                seen[size_t(j)] = 2;
            }
        }
        AHIP_CHECK(hipSetDevice(A->device));
        res = new adelie_hip_pinball_result;
        res->dtype = A->dtype;
        res->device = A->device;
        res->m = m;
        res->d = d;
        const auto t0 = std::chrono::steady_clock::now();
        if (A->dtype == ADELIE_HIP_F64) pinball_run<double>(A, a, res);
        else pinball_run<float>(A, a, res);
        res->total_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *out = res;
    } catch (const std::exception& e) {
        delete res;
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

int adelie_hip_pinball_result_destroy(adelie_hip_pinball_result* r) {
    if (r && r->as_dev) (void)hipSetDevice(r->device);
    delete r;
    return 0;
}

int64_t adelie_hip_pinball_result_size(const adelie_hip_pinball_result* r, int which) {
    if (!r) return -1;
    switch (which) {
        case ADELIE_HIP_PINBALL_BETA:
        case ADELIE_HIP_PINBALL_GRAD:
        case ADELIE_HIP_PINBALL_IS_SCREEN:
        case ADELIE_HIP_PINBALL_IS_ACTIVE: return r->m;
        case ADELIE_HIP_PINBALL_RESID: return r->d;
        case ADELIE_HIP_PINBALL_SCREEN_SET:
        case ADELIE_HIP_PINBALL_SCREEN_ASAT_DIAG: return int64_t(r->screen_set.size());
        case ADELIE_HIP_PINBALL_ACTIVE_SET: return int64_t(r->active_set.size());
        case ADELIE_HIP_PINBALL_SCREEN_AS: return r->as_dev ? int64_t(r->screen_set.size()) * r->d : 0;
    }
    return -1;
}

int adelie_hip_pinball_result_copy(const adelie_hip_pinball_result* r, int which, void* out, int64_t cap) {
    try {
        const int64_t size = adelie_hip_pinball_result_size(r, which);
        if (size < 0 || !out) throw make_core_error("unknown result vector.");
        const size_t n = size_t(std::min(size, cap));
        const size_t es = r->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
        if (!n) return 0;
        switch (which) {
            case ADELIE_HIP_PINBALL_BETA: std::memcpy(out, r->beta.data(), n * es); break;
            case ADELIE_HIP_PINBALL_RESID: std::memcpy(out, r->resid.data(), n * es); break;
            case ADELIE_HIP_PINBALL_GRAD: std::memcpy(out, r->grad.data(), n * es); break;
            case ADELIE_HIP_PINBALL_SCREEN_ASAT_DIAG: std::memcpy(out, r->asat_diag.data(), n * es); break;
            case ADELIE_HIP_PINBALL_SCREEN_SET: std::memcpy(out, r->screen_set.data(), n * sizeof(int64_t)); break;
            case ADELIE_HIP_PINBALL_ACTIVE_SET: std::memcpy(out, r->active_set.data(), n * sizeof(int64_t)); break;
            case ADELIE_HIP_PINBALL_IS_SCREEN: std::memcpy(out, r->is_screen.data(), n); break;
            case ADELIE_HIP_PINBALL_IS_ACTIVE: std::memcpy(out, r->is_active.data(), n); break;
            case ADELIE_HIP_PINBALL_SCREEN_AS:
                AHIP_CHECK(hipSetDevice(r->device));
                AHIP_CHECK(hipMemcpy(out, r->as_dev, n * es, hipMemcpyDeviceToHost));
                break;
        }
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

double adelie_hip_pinball_result_scalar(const adelie_hip_pinball_result* r, int which) {
    if (!r) return 0;
    switch (which) {
        case ADELIE_HIP_PINBALL_LOSS: return r->loss;
        case ADELIE_HIP_PINBALL_ITERS: return double(r->iters);
        case ADELIE_HIP_PINBALL_N_KKT: return double(r->n_kkt);
        case ADELIE_HIP_PINBALL_SCREEN_SET_SIZE: return double(r->screen_set.size());
        case ADELIE_HIP_PINBALL_ACTIVE_SET_SIZE: return double(r->active_set.size());
        case ADELIE_HIP_PINBALL_TOTAL_TIME: return r->total_time;
        case ADELIE_HIP_PINBALL_T_SWEEP_MS: return r->t_sweep_ms;
        case ADELIE_HIP_PINBALL_T_GRAM_MS: return r->t_gram_ms;
        case ADELIE_HIP_PINBALL_T_FIT_MS: return r->t_fit_ms;
        case ADELIE_HIP_PINBALL_N_CHANGED: return double(r->n_changed);
    }
    return 0;
}

const char* adelie_hip_pinball_result_error(const adelie_hip_pinball_result* r) { return r ? r->error.c_str() : ""; }

} // extern "C"
