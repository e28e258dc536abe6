// solver.hip — C ABI: the grpnet path driver (host side) over the device-resident state.
//
// Host logic restated from the reference (paths relative to adelie/src/include/adelie_core):
//   solve_core            solver/solver_base.hpp:435-687   (lambda_max bootstrap, path generation, BASIL loop)
//   screen / search_pivot solver/solver_base.hpp:273-403, optimization/search_pivot.hpp:7-62
//   kkt, early_exit       solver/solver_base.hpp:408-433, :241-263
//   update_screen_derived solver/solver_base.hpp:120-153, solver/solver_gaussian_naive.hpp:41-176
//   gaussian fit          solver/solver_gaussian_naive.hpp:209-349
//   glm (IRLS) fit        solver/solver_glm_naive.hpp:160-459
// These are O(G log G) scalar decisions per lambda and stay on the host; everything that touches an n- or
// p-vector or the design runs in the kernels of kernels_*.hip on the design's stream.  Per BASIL iteration the
// host receives: the CD kernel's scalar block, the screen coefficients (<= |S| values) and abs_grad (G values).
#include "common.hpp"
#include "design_ops.hpp"
#include "filter_host.hpp"
#include "screen_reads_host.hpp"
#include "cox.hpp"

#include <algorithm>
#include <cstring>
#include <exception>
#include <type_traits>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <unordered_set>

namespace ahip {
void set_last_error(const std::string& s);
double g_hessian_min = 1e-24; // configs.hpp:6-21
double g_dbeta_tol = 1e-12;

// elementwise GLM kernels (kernels_glm.hip)
template <class T>
void launch_irls_prepare(int kind, const T* y, const T* w, const T* eta, const T* resid, const T* offsets, T hessian_min,
                         int64_t n, T* hess, T* irls_resid, T* irls_y, T* sums4, hipStream_t s, int K = 1);
template <class T>
void launch_irls_weights(const T* hess, T hess_sum, const T* irls_y, T shift, int64_t n, T* wts, T* irls_resid,
                         T* sums3, hipStream_t s);
template <class T>
void launch_irls_finish(int kind, const T* y, const T* w, const T* irls_y, const T* offsets, const T* irls_resid, T shift,
                        int64_t n, T* eta, T* resid, T* sums2, hipStream_t s, int K = 1);
template <class T>
void launch_glm_gradient(int kind, const T* y, const T* w, const T* eta, int64_t n, T* resid, hipStream_t s, int K = 1);
template <class T>
void launch_glm_loss(int kind, const T* y, const T* w, const T* eta, int64_t n, T* out1, hipStream_t s, int K = 1);
template <class T>
void launch_null_step(int kind, const T* y, const T* w, const T* eta, const T* resid, const T* offsets, T hessian_min,
                      int64_t n, T* sums2, hipStream_t s, int K = 1, const T* cb_hess = nullptr, const T* cb_z = nullptr);
template <class T>
void launch_set_eta(const T* offsets, T beta0, int64_t n, T* eta, hipStream_t s);
template <class T>
void launch_dot_diff(const T* a, const T* a0, const T* b, const T* b0, int64_t n, T* out1, hipStream_t s);
template <class T>
void launch_rel_change(const T* a, T* prev, int64_t n, T* out, hipStream_t s);
template <class T>
void launch_gather(const T* src, const int32_t* idx, int64_t cnt, T* dst, hipStream_t s);
template <class T>
void launch_scatter(const T* src, const int32_t* idx, int64_t cnt, T* dst, hipStream_t s); // dst[idx[a]] = src[a]
} // namespace ahip

using namespace ahip;
using idx = int64_t;

namespace {

struct Stopwatch {
    std::chrono::steady_clock::time_point t0;
    void start() { t0 = std::chrono::steady_clock::now(); }
    double elapsed() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

core_error max_cds_error(int l) {
    return make_solver_error("max coordinate descents reached at lambda index: " + std::to_string(l) + ".");
}
core_error max_screen_set_error() { return make_solver_error("maximum screen set size reached."); }

// cyclic Jacobi eigen-decomposition of a symmetric (q,q) matrix; stands in for Eigen::SelfAdjointEigenSolver
// (solver_gaussian_naive.hpp:113).  Eigenvalues ascending, V column-major with eigenvectors in columns.
void jacobi_eigh(int q, std::vector<double>& A, std::vector<double>& V, std::vector<double>& D) {
    V.assign(size_t(q) * q, 0.0);
    for (int i = 0; i < q; ++i) V[i + size_t(i) * q] = 1.0;
    auto a = [&](int i, int j) -> double& { return A[i + size_t(j) * q]; };
    auto v = [&](int i, int j) -> double& { return V[i + size_t(j) * q]; };
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0, dg = 0;
        for (int i = 0; i < q; ++i) {
            dg += a(i, i) * a(i, i);
            for (int j = i + 1; j < q; ++j) off += a(i, j) * a(i, j);
        }
        if (off == 0 || off <= 1e-32 * (dg + off)) break;
        for (int r = 0; r < q - 1; ++r)
            for (int c = r + 1; c < q; ++c) {
                const double arc = a(r, c);
                if (arc == 0.0) continue;
                const double theta = (a(c, c) - a(r, r)) / (2.0 * arc);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < q; ++k) {
                    const double x = a(k, r), y = a(k, c);
                    a(k, r) = cs * x - sn * y;
                    a(k, c) = sn * x + cs * y;
                }
                for (int k = 0; k < q; ++k) {
                    const double x = a(r, k), y = a(c, k);
                    a(r, k) = cs * x - sn * y;
                    a(c, k) = sn * x + cs * y;
                }
                for (int k = 0; k < q; ++k) {
                    const double x = v(k, r), y = v(k, c);
                    v(k, r) = cs * x - sn * y;
                    v(k, c) = sn * x + cs * y;
                }
            }
    }
    std::vector<int> ord(q);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int i, int j) { return a(i, i) < a(j, j); });
    std::vector<double> V2(size_t(q) * q);
    D.resize(q);
    for (int k = 0; k < q; ++k) {
        D[k] = a(ord[k], ord[k]);
        for (int i = 0; i < q; ++i) V2[i + size_t(k) * q] = v(i, ord[k]);
    }
    V.swap(V2);
}

// HIP-event timing of the device phases on the design's own stream (read by bench.py for the roofline object)
// (timing events are recycled through a process-wide free list: a headline path records ~2000 pairs)
struct TimingEvents {
    static std::mutex& mu() { static std::mutex* m = new std::mutex; return *m; }
    static std::vector<hipEvent_t>& idle() { static auto* v = new std::vector<hipEvent_t>; return *v; }
    static hipEvent_t take() {
        {
            std::lock_guard<std::mutex> lk(mu());
            auto& v = idle();
            if (!v.empty()) {
                hipEvent_t e = v.back();
                v.pop_back();
                return e;
            }
        }
        hipEvent_t e;
        AHIP_CHECK(hipEventCreate(&e));
        return e;
    }
    static void give(hipEvent_t e) {
        {
            std::lock_guard<std::mutex> lk(mu());
            if (idle().size() < 16384) {
                idle().push_back(e);
                return;
            }
        }
        (void)hipEventDestroy(e);
    }
};
struct KTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    double ms = 0;
    int64_t launches = 0;
    void begin(hipStream_t st) {
        hipEvent_t a = TimingEvents::take(), b = TimingEvents::take();
        AHIP_CHECK(hipEventRecord(a, st));
        ev.emplace_back(a, b);
    }
    void end(hipStream_t st) { AHIP_CHECK(hipEventRecord(ev.back().second, st)); }
    std::vector<float> each; // per-launch milliseconds (debug / tuning)
    void collect() {
        for (auto& e : ev) {
            float t = 0;
            if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&t, e.first, e.second) == hipSuccess) {
                ms += t;
                ++launches;
                each.push_back(t);
            }
            TimingEvents::give(e.first);
            TimingEvents::give(e.second);
        }
        ev.clear();
    }
    ~KTimer() { collect(); }
};

struct Counters {
    int64_t n_basil_iters = 0, n_sweeps = 0, n_cd_visits_screen = 0, n_cd_visits_active = 0, n_updates = 0,
            n_irls_iters = 0, n_new_screen_cols = 0, n_cd_passes_screen = 0, n_cd_passes_active = 0,
            n_gram_col_reads = 0, n_resid_col_reads = 0, n_panel_blocks = 0, n_panel_grams = 0, n_panel_cols = 0,
            n_irls_screen_cols = 0, n_sweeps_shared = 0, n_update_cols = 0, n_sweeps_factor = 0;
    double gram_flops = 0;
};

template <class T>
struct FitOut {
    std::vector<idx> beta_idx;
    std::vector<T> beta_val;
    T intercept = 0, rsq = 0;
    double t_screen = 0, t_active = 0;
};

// ------------------------------------------------------------------------------------------------------------
// Sweep batching: solvers that run concurrently on one resident dense matrix (the folds of cv_grpnet, each from its own
// host thread on an alias handle) all spend most of their time in the same HBM-bound kernel, the full-gradient sweep X^T v.
// The K-wide sweep of kernels_multi.hip reads X once for K vectors, so the solvers that reach their sweep within a short
// window are answered by ONE pass over X.  A solver that arrives alone (or with batching off) takes its ordinary sweep.
// Results do not depend on who shares a batch: every vector's dot products are accumulated independently and in a fixed
// order; they differ from the ordinary sweep kernel's only by that order (last bits).
// ------------------------------------------------------------------------------------------------------------
int g_sweep_batch = 0; // adelie_hip_set_config("sweep_batch", 0/1)
std::mutex g_batcher_create_mutex;

struct SweepBatcher {
    static constexpr int KMAX = 8, NGEN = 4;
    std::mutex m;
    std::condition_variable cv;
    int registered = 0;
    struct Gen {
        int count = 0, K = 0, pending = 0; // pending: members of the launched batch that have not enqueued their pick yet
        hipEvent_t done = nullptr, in_ev[KMAX], out_ev[KMAX];
        bool out_set[KMAX], done_set = false, failed = false;
    };
    Gen gen[NGEN];
    uint64_t cur = 0, launched_upto = 0; // generation collecting arrivals; generations < launched_upto have been launched
    hipStream_t stream = nullptr;
    DevBuf<char> vbuf[NGEN], obuf[NGEN], work;
    // HIP-event timing of the shared sweeps on the batcher's stream (adelie_hip_design_batch_stats): launches, vectors
    // answered, milliseconds
    KTimer timer;
    int64_t n_vectors = 0;
    SweepBatcher() {
        AHIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (auto& g : gen) {
            AHIP_CHECK(hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
            for (int k = 0; k < KMAX; ++k) {
                AHIP_CHECK(hipEventCreateWithFlags(&g.in_ev[k], hipEventDisableTiming));
                AHIP_CHECK(hipEventCreateWithFlags(&g.out_ev[k], hipEventDisableTiming));
                g.out_set[k] = false;
            }
        }
    }
    ~SweepBatcher() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        for (auto& g : gen) {
            (void)hipEventDestroy(g.done);
            for (int k = 0; k < KMAX; ++k) {
                (void)hipEventDestroy(g.in_ev[k]);
                (void)hipEventDestroy(g.out_ev[k]);
            }
        }
    }
    void add() { std::lock_guard<std::mutex> lk(m); ++registered; }
    void remove() {
        { std::lock_guard<std::mutex> lk(m); --registered; }
        cv.notify_all();
    }
    // out[u] = X[:,u] . v - (sub_vec ? sub_scale[0] * sub_vec[u] : 0) on stream `ps`; returns false if the caller should run its
    // own sweep (it is the only solver around)
    template <class T>
    bool sweep(const DenseView<T>& X, const T* v, T* out, const T* sub_scale, const T* sub_vec, hipStream_t ps) {
        const int64_t n = X.n, p = X.p;
        std::unique_lock<std::mutex> lk(m);
        if (registered <= 1) return false;
        // join the generation that is collecting (a full one is launched by its leader before anybody can join again)
        while (gen[cur % NGEN].count >= KMAX || gen[cur % NGEN].pending > 0) cv.wait(lk);
        const uint64_t g = cur;
        Gen& G = gen[g % NGEN];
        const int slot = G.count++;
        char* vb = nullptr;
        try { // stage this solver's vector.  The mutex is held from the join above to the end of this block, so nobody has
              // joined after us yet: a failure here is undone by leaving the generation again, and nobody ever waits for us
            vb = vbuf[g % NGEN].reserve(size_t(KMAX) * size_t(n) * sizeof(T));
            if (G.done_set) AHIP_CHECK(hipStreamWaitEvent(ps, G.done, 0)); // the previous user of this buffer has been read
            AHIP_CHECK(hipMemcpyAsync(vb + size_t(slot) * size_t(n) * sizeof(T), v, size_t(n) * sizeof(T), hipMemcpyDeviceToDevice, ps));
            AHIP_CHECK(hipEventRecord(G.in_ev[slot], ps));
        } catch (...) {
            --G.count;
            lk.unlock();
            cv.notify_all();
            throw;
        }
        if (slot == 0) {
            // leader: give the others a window of about four sweep times (a sweep moves n*p values at ~7 TB/s), then launch
            // for whoever has arrived: waiting costs a lone solver at most that, sharing saves K - 1 sweeps
            // (8-fold CV, 100k x 10k: 1.05 s with a 0.25 ms window, 0.84 s with 0.8 ms, 0.70 s with 5 ms, no better beyond)
            const double sweep_us = double(n) * double(p) * double(sizeof(T)) / 7.0e6;
            const int window_us = int(std::min(5000.0, std::max(100.0, 4.0 * sweep_us)));
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(window_us);
            cv.wait_until(lk, deadline, [&] { return G.count >= std::min(registered, KMAX); });
            const int K = G.count;
            G.K = K;
            G.failed = false;
            ++cur; // later arrivals collect in the next generation
            try {
                T* ob = reinterpret_cast<T*>(obuf[g % NGEN].reserve(size_t(KMAX) * size_t(p) * sizeof(T)));
                for (int k = 0; k < K; ++k) AHIP_CHECK(hipStreamWaitEvent(stream, G.in_ev[k], 0));
                for (int k = 0; k < KMAX; ++k) // the previous readers of this output buffer are done
                    if (G.out_set[k]) { AHIP_CHECK(hipStreamWaitEvent(stream, G.out_ev[k], 0)); G.out_set[k] = false; }
                MultiView<T> mv{X.X, n, p, X.ld, nullptr, int32_t(K), 0};
                T* wk = reinterpret_cast<T*>(work.reserve(size_t(multi_sweep_work_elems<T>(MultiView<T>{X.X, n, p, X.ld, nullptr, KMAX, 0})) * sizeof(T)));
                timer.begin(stream);
                launch_multi_sweep<T>(mv, reinterpret_cast<const T*>(vb), ob, wk, stream);
                timer.end(stream);
                n_vectors += K;
                AHIP_CHECK(hipEventRecord(G.done, stream));
                G.done_set = true;
            } catch (...) {
                G.failed = true; // the members of this batch must not wait for a launch that did not happen
            }
            G.count = 0; // the slot bookkeeping of this generation index restarts when it comes round again
            G.pending = K;
            launched_upto = g + 1;
            lk.unlock();
            cv.notify_all();
            lk.lock();
        } else {
            cv.notify_all(); // the leader may be waiting for the last arrival
            cv.wait(lk, [&] { return launched_upto > g; });
        }
        // every member of a launched generation accounts for itself in `pending` exactly once, whatever happens to its pick:
        // a generation whose count of pending members never reaches zero would stall every solver once `cur` wraps to it
        const int K = G.K;
        std::exception_ptr err;
        if (G.failed) {
            err = std::make_exception_ptr(core_error("adelie_hip: the shared sweep of a batch of concurrent solves failed to launch."));
        } else {
            try {
                const T* ob = reinterpret_cast<const T*>(obuf[g % NGEN].p);
                AHIP_CHECK(hipStreamWaitEvent(ps, G.done, 0));
                launch_batch_pick<T>(ob, p, K, slot, sub_scale, sub_vec, out, ps);
                AHIP_CHECK(hipEventRecord(G.out_ev[slot], ps));
                G.out_set[slot] = true;
            } catch (...) {
                err = std::current_exception();
            }
        }
        --G.pending;
        lk.unlock();
        cv.notify_all();
        if (err) std::rethrow_exception(err);
        return true;
    }
};

SweepBatcher* batcher_of(adelie_hip_design* d) {
    adelie_hip_design* owner = d->batch_owner ? d->batch_owner : d;
    std::lock_guard<std::mutex> lk(g_batcher_create_mutex);
    if (!owner->batcher) owner->batcher = new SweepBatcher();
    return static_cast<SweepBatcher*>(owner->batcher);
}

// ------------------------------------------------------------------------------------------------------------
// Solver: host mirror of StateGaussianNaive / StateGlmNaive + the device-resident working set
// ------------------------------------------------------------------------------------------------------------
template <class T>
struct Solver {
#include "solver_builds.hpp"
#include "solver_screen.hpp"
#include "solver_panel.hpp"
#include "solver_fit.hpp"
#include "solver_path.hpp"
};

struct ResultBase {
    int device = -1; // the device the solve ran on
    virtual ~ResultBase() {}
    virtual void sync_live() = 0;
    virtual int64_t size(int which) const = 0;
    virtual int copy(int which, void* out, int64_t cap) const = 0;
    virtual double scalar(int which) const = 0;
    virtual const char* err() const = 0;
};

template <class V>
void cp_d(const V& v, double* out, int64_t cap) {
    const int64_t m = std::min<int64_t>(cap, int64_t(v.size()));
    for (int64_t i = 0; i < m; ++i) out[i] = double(v[i]);
}
template <class V>
void cp_i(const V& v, int64_t* out, int64_t cap) {
    const int64_t m = std::min<int64_t>(cap, int64_t(v.size()));
    for (int64_t i = 0; i < m; ++i) out[i] = int64_t(v[i]);
}

template <class T>
struct Result : ResultBase {
    Solver<T> s;
    void sync_live() override { s.download_invariants(); }
    int64_t size(int which) const override {
        switch (which) {
            case ADELIE_HIP_V_INTERCEPTS: return s.intercepts.size();
            case ADELIE_HIP_V_DEVS: return s.devs.size();
            case ADELIE_HIP_V_LMDAS: return s.lmdas.size();
            case ADELIE_HIP_V_LMDA_PATH: return s.lmda_path.size();
            case ADELIE_HIP_V_SCREEN_BETA: return s.screen_beta.size();
            case ADELIE_HIP_V_GRAD: return s.grad.size();
            case ADELIE_HIP_V_ABS_GRAD: return s.abs_grad.size();
            case ADELIE_HIP_V_RESID: return s.resid.size();
            case ADELIE_HIP_V_ETA: return s.eta.size();
            case ADELIE_HIP_V_SCREEN_X_MEANS: return s.screen_X_means.size();
            case ADELIE_HIP_V_SCREEN_VARS: return s.screen_vars.size();
            case ADELIE_HIP_V_SCREEN_TRANSFORMS: { int64_t t = 0; for (auto& v : s.screen_transforms) t += v.size(); return t; }
            case ADELIE_HIP_V_BENCHMARK_SCREEN: return s.benchmark_screen.size();
            case ADELIE_HIP_V_BENCHMARK_FIT_SCREEN: return s.benchmark_fit_screen.size();
            case ADELIE_HIP_V_BENCHMARK_FIT_ACTIVE: return s.benchmark_fit_active.size();
            case ADELIE_HIP_V_BENCHMARK_KKT: return s.benchmark_kkt.size();
            case ADELIE_HIP_V_BENCHMARK_INVARIANCE: return s.benchmark_invariance.size();
            case ADELIE_HIP_I_SCREEN_SET: return s.screen_set.size();
            case ADELIE_HIP_I_SCREEN_BEGINS: return s.screen_begins.size();
            case ADELIE_HIP_I_SCREEN_IS_ACTIVE: return s.screen_is_active.size();
            case ADELIE_HIP_I_ACTIVE_SET: return s.active_set.size();
            case ADELIE_HIP_I_N_VALID_SOLUTIONS: return s.n_valid_solutions.size();
            case ADELIE_HIP_I_ACTIVE_SIZES: return s.active_sizes.size();
            case ADELIE_HIP_I_SCREEN_SIZES: return s.screen_sizes.size();
            case ADELIE_HIP_I_BETAS_INDPTR: return s.betas_idx.size() + 1;
            case ADELIE_HIP_I_BETAS_INDICES:
            case ADELIE_HIP_V_BETAS_VALUES: { int64_t t = 0; for (auto& v : s.betas_idx) t += v.size(); return t; }
            case ADELIE_HIP_I_DUALS_INDPTR: return s.duals_idx.size() + 1;
            case ADELIE_HIP_I_DUALS_INDICES:
            case ADELIE_HIP_V_DUALS_VALUES: { int64_t t = 0; for (auto& v : s.duals_idx) t += v.size(); return t; }
            case ADELIE_HIP_V_CONSTRAINT_MU: return s.cons_on ? s.G : 0;
            case ADELIE_HIP_V_CONSTRAINT_VMU: return s.cons_dev ? s.p : 0;
            case ADELIE_HIP_I_CONSTRAINT_DEV_GROUPS: return s.cons_dev ? int64_t(s.devcons_list.size()) : 0;
        }
        return -1;
    }
    int copy(int which, void* out, int64_t cap) const override {
        double* d = (double*)out;
        int64_t* ii = (int64_t*)out;
        switch (which) {
            case ADELIE_HIP_V_INTERCEPTS: cp_d(s.intercepts, d, cap); return 0;
            case ADELIE_HIP_V_DEVS: cp_d(s.devs, d, cap); return 0;
            case ADELIE_HIP_V_LMDAS: cp_d(s.lmdas, d, cap); return 0;
            case ADELIE_HIP_V_LMDA_PATH: cp_d(s.lmda_path, d, cap); return 0;
            case ADELIE_HIP_V_SCREEN_BETA: cp_d(s.screen_beta, d, cap); return 0;
            case ADELIE_HIP_V_GRAD: cp_d(s.grad, d, cap); return 0;
            case ADELIE_HIP_V_ABS_GRAD: cp_d(s.abs_grad, d, cap); return 0;
            case ADELIE_HIP_V_RESID: cp_d(s.resid, d, cap); return 0;
            case ADELIE_HIP_V_ETA: cp_d(s.eta, d, cap); return 0;
            case ADELIE_HIP_V_SCREEN_X_MEANS: cp_d(s.screen_X_means, d, cap); return 0;
            case ADELIE_HIP_V_SCREEN_VARS: cp_d(s.screen_vars, d, cap); return 0;
            case ADELIE_HIP_V_SCREEN_TRANSFORMS: {
                int64_t k = 0;
                for (auto& v : s.screen_transforms)
                    for (auto x : v) { if (k < cap) d[k] = double(x); ++k; }
                return 0;
            }
            case ADELIE_HIP_V_BENCHMARK_SCREEN: cp_d(s.benchmark_screen, d, cap); return 0;
            case ADELIE_HIP_V_BENCHMARK_FIT_SCREEN: cp_d(s.benchmark_fit_screen, d, cap); return 0;
            case ADELIE_HIP_V_BENCHMARK_FIT_ACTIVE: cp_d(s.benchmark_fit_active, d, cap); return 0;
            case ADELIE_HIP_V_BENCHMARK_KKT: cp_d(s.benchmark_kkt, d, cap); return 0;
            case ADELIE_HIP_V_BENCHMARK_INVARIANCE: cp_d(s.benchmark_invariance, d, cap); return 0;
            case ADELIE_HIP_I_SCREEN_SET: cp_i(s.screen_set, ii, cap); return 0;
            case ADELIE_HIP_I_SCREEN_BEGINS: cp_i(s.screen_begins, ii, cap); return 0;
            case ADELIE_HIP_I_SCREEN_IS_ACTIVE: cp_i(s.screen_is_active, ii, cap); return 0;
            case ADELIE_HIP_I_ACTIVE_SET: cp_i(s.active_set, ii, cap); return 0;
            case ADELIE_HIP_I_N_VALID_SOLUTIONS: cp_i(s.n_valid_solutions, ii, cap); return 0;
            case ADELIE_HIP_I_ACTIVE_SIZES: cp_i(s.active_sizes, ii, cap); return 0;
            case ADELIE_HIP_I_SCREEN_SIZES: cp_i(s.screen_sizes, ii, cap); return 0;
            case ADELIE_HIP_I_BETAS_INDPTR: {
                int64_t acc = 0, k = 0;
                if (k < cap) ii[k] = 0;
                ++k;
                for (auto& v : s.betas_idx) { acc += v.size(); if (k < cap) ii[k] = acc; ++k; }
                return 0;
            }
            case ADELIE_HIP_I_BETAS_INDICES: {
                int64_t k = 0;
                for (auto& v : s.betas_idx) for (auto x : v) { if (k < cap) ii[k] = x; ++k; }
                return 0;
            }
            case ADELIE_HIP_V_BETAS_VALUES: {
                int64_t k = 0;
                for (auto& v : s.betas_val) for (auto x : v) { if (k < cap) d[k] = double(x); ++k; }
                return 0;
            }
            case ADELIE_HIP_I_DUALS_INDPTR: {
                int64_t acc = 0, k = 0;
                if (k < cap) ii[k] = 0;
                ++k;
                for (auto& v : s.duals_idx) { acc += v.size(); if (k < cap) ii[k] = acc; ++k; }
                return 0;
            }
            case ADELIE_HIP_I_DUALS_INDICES: {
                int64_t k = 0;
                for (auto& v : s.duals_idx) for (auto x : v) { if (k < cap) ii[k] = x; ++k; }
                return 0;
            }
            case ADELIE_HIP_I_CONSTRAINT_DEV_GROUPS: {
                if (!s.cons_dev) return 0;
                int64_t k = 0;
                for (int32_t g : s.devcons_list) { if (k < cap) ii[k] = g; ++k; }
                return 0;
            }
            case ADELIE_HIP_V_DUALS_VALUES: {
                int64_t k = 0;
                for (auto& v : s.duals_val) for (auto x : v) { if (k < cap) d[k] = double(x); ++k; }
                return 0;
            }
            case ADELIE_HIP_V_CONSTRAINT_MU: {
                if (!s.cons_on) return 0;
                for (idx g = 0; g < s.G && g < cap; ++g) d[g] = s.cons_kind[g] ? double(s.cons_dual_of(g)) : 0.0;
                return 0;
            }
            case ADELIE_HIP_V_CONSTRAINT_VMU: {
                if (!s.cons_dev) return 0;
                cp_d(s.cons_vmu, d, cap);
                return 0;
            }
        }
        return 1;
    }
    double scalar(int which) const override {
        switch (which) {
            case ADELIE_HIP_S_LMDA_MAX: return s.lmda_max;
            case ADELIE_HIP_S_LMDA: return s.lmda;
            case ADELIE_HIP_S_RSQ: return s.rsq;
            case ADELIE_HIP_S_RESID_SUM: return s.resid_sum;
            case ADELIE_HIP_S_ACTIVE_SET_SIZE: return double(s.active_set_size);
            case ADELIE_HIP_S_BETA0: return s.beta0;
            case ADELIE_HIP_S_LOSS_NULL: return s.loss_null;
            case ADELIE_HIP_S_LOSS_FULL: return s.loss_full;
            case ADELIE_HIP_S_TOTAL_TIME: return s.total_time;
            case ADELIE_HIP_S_N_BASIL_ITERS: return double(s.cnt.n_basil_iters);
            case ADELIE_HIP_S_N_SWEEPS: return double(s.cnt.n_sweeps);
            case ADELIE_HIP_S_N_CD_VISITS_SCREEN: return double(s.cnt.n_cd_visits_screen);
            case ADELIE_HIP_S_N_CD_VISITS_ACTIVE: return double(s.cnt.n_cd_visits_active);
            case ADELIE_HIP_S_N_UPDATES: return double(s.cnt.n_updates);
            case ADELIE_HIP_S_N_IRLS_ITERS: return double(s.cnt.n_irls_iters);
            case ADELIE_HIP_S_N_NEW_SCREEN_COLS: return double(s.cnt.n_new_screen_cols);
            case ADELIE_HIP_S_N_CD_PASSES_SCREEN: return double(s.cnt.n_cd_passes_screen);
            case ADELIE_HIP_S_N_CD_PASSES_ACTIVE: return double(s.cnt.n_cd_passes_active);
            case ADELIE_HIP_S_N_GRAM_COL_READS: return double(s.cnt.n_gram_col_reads);
            case ADELIE_HIP_S_N_RESID_COL_READS: return double(s.cnt.n_resid_col_reads);
            case ADELIE_HIP_S_GRAM_FLOPS: return s.cnt.gram_flops;
            case ADELIE_HIP_S_N_PANEL_BLOCKS: return double(s.cnt.n_panel_blocks);
            case ADELIE_HIP_S_N_PANEL_GRAMS: return double(s.cnt.n_panel_grams);
            case ADELIE_HIP_S_N_PANEL_COLS: return double(s.cnt.n_panel_cols);
            case ADELIE_HIP_S_N_IRLS_SCREEN_COLS: return double(s.cnt.n_irls_screen_cols);
            case ADELIE_HIP_S_N_SPECULATED: return double(s.n_spec);
            case ADELIE_HIP_S_N_SPEC_ROLLBACKS: return double(s.n_spec_rollback);
            case ADELIE_HIP_S_T_PANEL_STEP_MS: return s.t_step.ms;
            case ADELIE_HIP_S_N_PANEL_STEP_LAUNCHES: return double(s.t_step.launches);
            case ADELIE_HIP_S_T_SWEEP_MS: return s.t_sweep.ms;
            case ADELIE_HIP_S_T_GRAM_MS: return s.t_gram.ms;
            case ADELIE_HIP_S_T_CD_MS: return s.t_cd.ms;
            case ADELIE_HIP_S_T_AXPY_MS: return s.t_axpy.ms;
            case ADELIE_HIP_S_N_SWEEP_LAUNCHES: return double(s.t_sweep.launches);
            case ADELIE_HIP_S_N_GRAM_LAUNCHES: return double(s.t_gram.launches);
            case ADELIE_HIP_S_T_HOST_SCREEN_MS: return 1e3 * s.t_host_screen;
            case ADELIE_HIP_S_T_HOST_SCREEN_WAIT_MS: return 1e3 * s.t_host_screen_wait;
            case ADELIE_HIP_S_N_SWEEPS_SHARED: return double(s.cnt.n_sweeps_shared);
            case ADELIE_HIP_S_N_UPDATE_COLS: return double(s.cnt.n_update_cols);
            case ADELIE_HIP_S_N_DEVICE_SCREENS: return 0.0; /* (screening on the device was measured slower and removed in round 4) */
            case ADELIE_HIP_S_N_HOST_SCREENS: return double(s.n_host_screens);
            case ADELIE_HIP_S_N_HOST_CONS_VISITS: return double(s.n_host_cons_visits);
            case ADELIE_HIP_S_N_DEV_CONS_VISITS: return double(s.n_dev_cons_visits_final);
            case ADELIE_HIP_S_N_SWEEPS_FACTOR: return double(s.cnt.n_sweeps_factor);
            case ADELIE_HIP_S_N_SWEEPS_FILTERED: return double(s.n_sweeps_filtered);
            case ADELIE_HIP_S_N_SWEEPS_REFILLED: return double(s.n_sweeps_refilled);
            case ADELIE_HIP_S_N_FILTER_EXACT_COLS: return double(s.n_filter_exact_cols);
            case ADELIE_HIP_S_N_FILTER_SHADOW_COLS: return double(s.n_filter_shadow_cols);
            case ADELIE_HIP_S_T_FSWEEP_MS: return s.t_fsweep.ms;
            case ADELIE_HIP_S_N_FSWEEP_LAUNCHES: return double(s.t_fsweep.launches);
            case ADELIE_HIP_S_FSWEEP_BYTES: return s.fsweep_bytes;
            case ADELIE_HIP_S_N_SCREEN_READS: return double(s.n_screen_reads);
            case ADELIE_HIP_S_N_SCREEN_SHORT: return double(s.n_screen_short);
            case ADELIE_HIP_S_N_FILTER_OPEN_COLS: return double(s.n_filter_open_cols);
            case ADELIE_HIP_S_ENGINE_PANEL: return s.engine_panel ? 1.0 : 0.0;
            default:
                if (which >= 900 && which < 908) return double(s.cd_dbg[which - 900]);
                if (which >= 910 && which < 918) return 1e3 * s.t_host[which - 910];
        }
        return std::numeric_limits<double>::quiet_NaN();
    }
    const char* err() const override { return s.error.c_str(); }
};

template <class T>
void run(adelie_hip_design* X, const adelie_hip_grpnet_args* a, adelie_hip_result* res);

} // namespace

struct adelie_hip_result {
    ResultBase* r = nullptr;
    ~adelie_hip_result() { delete r; }
};

namespace {

template <class T>
void run(adelie_hip_design* X, const adelie_hip_grpnet_args* a, adelie_hip_result* res) {
    auto* r = new Result<T>();
    res->r = r; // owned by `res` from here on (the poll callbacks read the live state through it)
    r->device = X->device;
    r->s.live = res;
    r->s.stage.init(size_t(8) << 20, X->stream);
    Staging::Scope stage_scope(&r->s.stage);
    DeferredFrees::Scope deferred_scope(&r->s.deferred);
    Stopwatch sw_build;
    sw_build.start();
    r->s.build(X, a);
    if (r->s.hooks.trace >= 2) std::fprintf(stderr, "[build] state set-up %.2f ms\n", sw_build.elapsed() * 1e3);
    Stopwatch sw;
    sw.start();
    struct BatchGuard { // registered for sweep batching exactly while the path runs
        SweepBatcher* b = nullptr;
        ~BatchGuard() { if (b) b->remove(); }
    } guard;
    if (g_sweep_batch && X->is_dense()) {
        guard.b = batcher_of(X);
        guard.b->add();
        r->s.batcher = guard.b;
    }
    try {
        r->s.solve();
    } catch (const std::exception& e) {
        r->s.error = e.what();
    }
    r->s.batcher = nullptr;
    if (guard.b) {
        guard.b->remove();
        guard.b = nullptr;
    }
    try {
        r->s.finalize();
    } catch (const std::exception& e) {
        if (r->s.error.empty()) r->s.error = e.what();
    }
    r->s.total_time = sw.elapsed();
    if (r->s.hooks.trace >= 2) std::fprintf(stderr, "[run] solve + finalize %.2f ms\n", r->s.total_time * 1e3);
    r->s.live = nullptr;
}

} // namespace

void adelie_hip_internal_free_batcher(void* b) { delete static_cast<SweepBatcher*>(b); }
void adelie_hip_internal_batch_stats(void* b, double* out) {
    out[0] = out[1] = out[2] = 0;
    if (!b) return;
    auto* sb = static_cast<SweepBatcher*>(b);
    std::lock_guard<std::mutex> lk(sb->m);
    sb->timer.collect();
    out[0] = double(sb->timer.launches);
    out[1] = double(sb->n_vectors);
    out[2] = sb->timer.ms;
}

namespace ahip {
extern double g_bvls_gram_limit_mb; // kernels_bvls.hip
extern int64_t g_bvls_lds_max_ns;
extern double g_pinball_gram_limit_mb; // kernels_pinball.hip
extern int64_t g_pinball_lds_max_ns;
extern int64_t g_qp_full_lds_max_d; // kernels_qp_full.hip
} // namespace ahip

extern "C" {

int adelie_hip_set_config(const char* name, double value) {
    const std::string nm(name ? name : "");
    if (nm == "hessian_min") g_hessian_min = value;
    else if (nm == "dbeta_tol") g_dbeta_tol = value;
    else if (nm == "sweep_batch") g_sweep_batch = value != 0.0 ? 1 : 0;
    else if (nm == "pool_limit_mb") {
        DevPool::limit_bytes() = value > 0 ? size_t(value) << 20 : 0;
        if (value <= 0) DevPool::trim();
    } else if (nm == "pool_trim") DevPool::trim();
    else if (nm == "bvls_gram_limit_mb") ahip::g_bvls_gram_limit_mb = value > 0 ? value : 16384.0;
    else if (nm == "bvls_lds_max_ns") ahip::g_bvls_lds_max_ns = value > 0 ? int64_t(value) : 0;
    else if (nm == "pinball_gram_limit_mb") ahip::g_pinball_gram_limit_mb = value > 0 ? value : 16384.0;
    else if (nm == "pinball_lds_max_ns") ahip::g_pinball_lds_max_ns = value > 0 ? int64_t(value) : 0;
    else if (nm == "qp_full_lds_max_d") ahip::g_qp_full_lds_max_d = value > 0 ? int64_t(value) : 0;
    else {
        set_last_error("adelie_core: unknown config name.");
        return 1;
    }
    return 0;
}

int adelie_hip_glm_cox_create(int device, int dtype, int64_t n, const void* start, const void* stop, const void* status,
                              const int64_t* strata, const void* weights, int tie_method, adelie_hip_glm_cox** out) {
    try {
        if (!out) throw make_core_error("null argument.");
        *out = cox_create(device, dtype, n, start, stop, status, strata, weights, tie_method);
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}
int adelie_hip_glm_cox_destroy(adelie_hip_glm_cox* h) {
    cox_destroy(h);
    return 0;
}
int adelie_hip_glm_cox_eval(adelie_hip_glm_cox* h, const void* eta, void* grad, void* hess, double* loss) {
    try {
        cox_eval_host(h, eta, grad, hess, loss);
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

static int solve_entry(adelie_hip_design* X, const adelie_hip_grpnet_args* args, adelie_hip_result** out, bool cov);
int adelie_hip_grpnet_solve(adelie_hip_design* X, const adelie_hip_grpnet_args* args, adelie_hip_result** out) {
    return solve_entry(X, args, out, false);
}
int adelie_hip_gaussian_cov_solve(adelie_hip_design* A, const adelie_hip_grpnet_args* args, adelie_hip_result** out) {
    return solve_entry(A, args, out, true);
}
static int solve_entry(adelie_hip_design* X, const adelie_hip_grpnet_args* args, adelie_hip_result** out, bool cov) {
    try {
        if (!X || !args || !out) throw make_core_error("null argument.");
        if (cov && !X->cov) throw make_core_error("A must be a covariance matrix (matrix.dense(method=\"cov\")).");
        if (!cov && X->cov) throw make_core_error("X is a covariance matrix: use gaussian_cov for the covariance method.");
        if (X->constraint) throw make_core_error("X is a constraint matrix (matrix.dense(method=\"constraint\")): use pinball.");
        auto* res = new adelie_hip_result();
        try {
            if (X->dtype == ADELIE_HIP_F64) run<double>(X, args, res);
            else run<float>(X, args, res);
        } catch (...) {
            delete res;
            throw;
        }
        *out = res;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}
int adelie_hip_grpnet_solve_many(adelie_hip_design* const* X, const adelie_hip_grpnet_args* const* args, int32_t count,
                                 adelie_hip_result** out, adelie_hip_done_fn on_done, void* user) {
    try {
        if (count < 0 || (count > 0 && (!X || !args || !out))) throw make_core_error("null argument.");
        for (int32_t k = 0; k < count; ++k) {
            out[k] = nullptr;
            if (!X[k] || !args[k]) throw make_core_error("null argument.");
            for (int32_t m = 0; m < k; ++m)
                if (X[m] == X[k]) throw make_core_error("solve_many: a design handle appears twice (concurrent solves need a handle each: adelie_hip_design_alias).");
        }
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    std::vector<std::string> msg(static_cast<size_t>(count));
    std::vector<int> rc(static_cast<size_t>(count), 0);
    auto one = [&](int32_t k) {
        rc[size_t(k)] = solve_entry(X[k], args[k], &out[k], false);
        if (rc[size_t(k)] != 0) msg[size_t(k)] = adelie_hip_last_error(); // (thread-local: read it on the solve's own thread)
        if (on_done) on_done(k, rc[size_t(k)], user);
    };
    if (count == 1) {
        one(0);
    } else {
        std::vector<std::thread> th;
        th.reserve(static_cast<size_t>(count));
        for (int32_t k = 0; k < count; ++k) th.emplace_back(one, k);
        for (auto& t : th) t.join();
    }
    for (int32_t k = 0; k < count; ++k)
        if (rc[size_t(k)] != 0) {
            set_last_error("solve " + std::to_string(k) + ": " + msg[size_t(k)]);
            return 1;
        }
    return 0;
}
int adelie_hip_result_destroy(adelie_hip_result* r) {
    if (r && r->r && r->r->device >= 0) (void)hipSetDevice(r->r->device); // (its buffers and streams are parked per device)
    delete r;
    return 0;
}
int64_t adelie_hip_result_size(const adelie_hip_result* r, int which) { return r->r->size(which); }
int adelie_hip_result_copy(const adelie_hip_result* r, int which, void* out, int64_t cap) { return r->r->copy(which, out, cap); }
double adelie_hip_result_scalar(const adelie_hip_result* r, int which) { return r->r->scalar(which); }
const char* adelie_hip_result_error(const adelie_hip_result* r) { return r->r->err(); }
int adelie_hip_result_sync(const adelie_hip_result* live) {
    try {
        if (!live || !live->r) throw make_core_error("null argument.");
        live->r->sync_live();
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

// Times `reps` launches of the dominant kernel with HIP events on the design's own stream.
int adelie_hip_bench_sweep(adelie_hip_design* d, int64_t reps, double* ms_per_launch) {
    try {
        if (!d || !ms_per_launch || reps <= 0) throw make_core_error("bad arguments.");
        if (d->cov_csc()) throw make_core_error("bench_sweep takes a design matrix, not a covariance matrix kept sparse.");
        AHIP_CHECK(hipSetDevice(d->device));
        hipStream_t s = d->stream;
        auto body = [&](auto tag) {
            using T = decltype(tag);
            DevBuf<T> v, out, xm, work, sc;
            v.reserve(d->n); out.reserve(d->p); xm.reserve(d->p); sc.reserve(1);
            // a one-hot / interaction or convex-relu design: the route ADELIE_HIP_FACTOR_SWEEP / ADELIE_HIP_RELU_SWEEP select (read here)
            // (a design made of pieces: raw_sweep issues the full range piece by piece, as a solve's per-lambda sweep does)
            const bool structured = raw_sweep_structured(*d, 0, d->p, nullptr, false, SweepHooks::from_env());
            work.reserve(size_t(raw_sweep_work_elems(*d, d->p, structured)));
            launch_fill<T>(v.p, T(1) / T(d->n), d->n, s);
            launch_fill<T>(xm.p, T(0.5), d->p, s);
            launch_fill<T>(sc.p, T(0.25), 1, s);
            auto once = [&]() { raw_sweep<T>(*d, v.p, out.p, 0, d->p, nullptr, sc.p, xm.p, false, structured, work.p, s); };
            once();
            AHIP_CHECK(hipStreamSynchronize(s));
            hipEvent_t e0, e1;
            AHIP_CHECK(hipEventCreate(&e0));
            AHIP_CHECK(hipEventCreate(&e1));
            AHIP_CHECK(hipEventRecord(e0, s));
            for (int64_t i = 0; i < reps; ++i) once();
            AHIP_CHECK(hipEventRecord(e1, s));
            AHIP_CHECK(hipEventSynchronize(e1));
            float ms = 0;
            AHIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            *ms_per_launch = double(ms) / double(reps);
        };
        if (d->dtype == ADELIE_HIP_F64) body(double{});
        else body(float{});
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

// One filtered invariance sweep on a dense f64 design, as a solve at one lambda enqueues it: v = w o r, the shadow sweep, the
// classification against tstar, the exact sweeps of the screen groups' columns, of the groups without a penalty and of the
// groups listed.  grad (p), exact (p: 1 where the value is the full sweep's), info: [0] columns listed, [1] flags (1: more
// than the cap of max(1024, p/4) were wanted, 2: a column swept both ways left its bound), [2] 1 if the route ran, 0 if
// the plain full sweep answered (hook off, no shadow), [3] columns wanted.
int adelie_hip_filter_sweep_test(adelie_hip_design* d, const double* w, const double* r, double sub_scale, const double* sub_vec,
                                 const int64_t* screen_groups, int64_t n_screen, const int64_t* groups, const int64_t* group_sizes,
                                 int64_t G, const double* penalty, double tstar, double* grad, uint8_t* exact, int64_t* info) {
    try {
        if (!d || !w || !r || !groups || !group_sizes || !penalty || !grad || !exact || !info || G < 1 || n_screen < 0)
            throw make_core_error("bad arguments.");
        if (!d->is_dense() || d->dtype != ADELIE_HIP_F64 || d->cov || d->constraint || d->std_center) throw make_core_error("a dense f64 design is required.");
        AHIP_CHECK(hipSetDevice(d->device));
        hipStream_t s = d->stream;
        const int64_t n = d->n, p = d->p;
        if (groups[G - 1] + group_sizes[G - 1] != p) throw make_core_error("groups do not cover the columns.");
        std::vector<int32_t> slot(size_t(G), -1), scols, pen0;
        for (int64_t k = 0; k < n_screen; ++k) {
            const int64_t g = screen_groups[k];
            if (g < 0 || g >= G) throw make_core_error("screen group out of range.");
            slot[size_t(g)] = int32_t(scols.size());
            for (int64_t t = 0; t < group_sizes[g]; ++t) scols.push_back(int32_t(groups[g] + t));
        }
        for (int64_t g = 0; g < G; ++g)
            if (!(penalty[g] > 0))
                for (int64_t t = 0; t < group_sizes[g]; ++t) pen0.push_back(int32_t(groups[g] + t));
        ShadowView sh{};
        const bool route = filter_sweep_on(Hooks::filter_sweep_env()) && adelie_hip_internal_shadow_acquire(d, &sh);
        const int64_t cap = filter_list_cap(p);
        DevBuf<double> dw, dr, dv, dgrad, dxm, dsc, dpen, dpart, dmetad, work;
        DevBuf<int64_t> dgroups, dgs;
        DevBuf<int32_t> dslot, dscols, dpen0, dlist, dmeta;
        dw.reserve(n); dr.reserve(n); dv.reserve(n); dgrad.reserve(p); dsc.reserve(1); dpen.reserve(G); dgroups.reserve(G);
        dgs.reserve(G); dslot.reserve(G); dlist.reserve(cap); dmeta.reserve(4); dmetad.reserve(2);
        const int n_part = filter_norm_parts(n);
        dpart.reserve(n_part);
        work.reserve(size_t(std::max(filtered_sweep_work_elems(n, p, int64_t(scols.size() + pen0.size()), cap), sweep_work_elems(n, p))));
        dw.upload(w, n, s); dr.upload(r, n, s); dsc.upload(&sub_scale, 1, s); dpen.upload(penalty, G, s);
        dgroups.upload(groups, G, s); dgs.upload(group_sizes, G, s); dslot.upload(slot.data(), G, s);
        if (sub_vec) { dxm.reserve(p); dxm.upload(sub_vec, p, s); }
        if (!scols.empty()) { dscols.reserve(scols.size()); dscols.upload(scols.data(), scols.size(), s); }
        if (!pen0.empty()) { dpen0.reserve(pen0.size()); dpen0.upload(pen0.data(), pen0.size(), s); }
        const double* xm = sub_vec ? dxm.p : nullptr;
        const DenseView<double> X = d->dense<double>();
        int32_t meta[4] = {0, 0, 0, 0};
        std::vector<int32_t> list;
        if (!route) {
            launch_vmul<double>(dw.p, dr.p, dv.p, n, s);
            launch_sweep<double>(X, dv.p, dgrad.p, 0, p, nullptr, dsc.p, xm, false, work.p, s);
            std::fill(exact, exact + p, uint8_t(1));
        } else {
            FilteredSweep a{};
            a.w = dw.p; a.r = dr.p; a.v = dv.p; a.grad = dgrad.p; a.sub_scale = dsc.p; a.sub_vec = xm;
            a.screen_cols = scols.empty() ? nullptr : dscols.p; a.n_screen_cols = int64_t(scols.size());
            a.pen0_cols = pen0.empty() ? nullptr : dpen0.p; a.n_pen0_cols = int64_t(pen0.size());
            a.groups = dgroups.p; a.group_sizes = dgs.p; a.G = G; a.slot = dslot.p; a.penalty = dpen.p; a.tstar = tstar;
            a.sq_part = dpart.p; a.list = dlist.p; a.cap = cap; a.meta_i = dmeta.p; a.meta_d = dmetad.p; a.work = work.p;
            enqueue_filtered_sweep(X, sh, a, s);
            AHIP_CHECK(hipMemcpyAsync(meta, dmeta.p, sizeof(meta), hipMemcpyDeviceToHost, s));
            AHIP_CHECK(hipStreamSynchronize(s));
            list.resize(size_t(meta[0]));
            if (meta[0] > 0) AHIP_CHECK(hipMemcpyAsync(list.data(), dlist.p, size_t(meta[0]) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            std::fill(exact, exact + p, uint8_t(0));
        }
        AHIP_CHECK(hipMemcpyAsync(grad, dgrad.p, size_t(p) * sizeof(double), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
        if (route) {
            for (int32_t c : scols) exact[c] = 1;
            for (int32_t c : pen0) exact[c] = 1;
            for (int32_t c : list) exact[c] = 1;
            if (meta[1] & 2) adelie_hip_internal_shadow_mark_stale(d);
        }
        info[0] = meta[0]; info[1] = meta[1]; info[2] = route ? 1 : 0; info[3] = meta[2];
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

// One block build on caller-supplied inputs, through the launcher the solver calls (tests; include/adelie_hip.h has the layout of
// `table` and `info`).  Everything the kernels index by is checked here against the buffers' sizes before anything is launched.
int adelie_hip_block_build_test(adelie_hip_design* d, int mode, int64_t row_off, const void* w, const int32_t* cols, int64_t n_cols,
                                const int64_t* table, int64_t count, const void* xm, int center, int64_t ldc, int strip_plain,
                                void* out0, int64_t out0_elems, void* out1, int64_t out1_elems, int64_t* info) {
    bool lds_changed = false;
    try {
        if (!d || !w || !cols || !table || !out0 || !info || n_cols < 1 || count < 1) throw make_core_error("bad arguments.");
        if (d->cov || d->constraint || d->std_center || d->is_multi()) throw make_core_error("a plain dense, 2-bit or compressed-column design is required.");
        no_pieces(*d, "adelie_hip_block_build_test"); // (the block builds below take a dense, a 2-bit or a compressed view)
        if (!d->is_dense() && !d->is_snp() && !d->is_csc()) throw make_core_error("a plain dense, 2-bit or compressed-column design is required.");
        if (center && !xm) throw make_core_error("center needs xm.");
        if (row_off < 0 || row_off >= d->n || (row_off > 0 && !d->is_dense())) throw make_core_error("row_off: a dense design and 0 <= row_off < n are required.");
        if (ldc < 1 || out0_elems < 1 || (out1 && out1_elems < 1)) throw make_core_error("bad output shape.");
        const int64_t n = d->n - row_off, p = d->p;
        for (int64_t i = 0; i < n_cols; ++i)
            if (cols[i] < 0 || cols[i] >= p) throw make_core_error("column out of range.");
        auto in_list = [&](int64_t off, int64_t cnt) { return off >= 0 && cnt >= 0 && off + cnt <= n_cols; };
        // a block of rows x cs entries at `dst` (leading dimension ldc) lies inside a buffer of `elems` elements
        auto fits = [&](int64_t dst, int64_t rows, int64_t cs, int64_t elems) {
            return dst >= 0 && rows >= 1 && cs >= 1 && rows <= ldc && dst + (rows - 1) + (cs - 1) * ldc < elems;
        };
        enum { M_SYRK = 0, M_SYRK_BATCH = 1, M_GRAM = 2, M_GRAM_BATCH = 3, M_STRIP = 4 };
        const int64_t* t = table;
        SyrkBatch sb{};
        GramBatch gb{};
        StripBatch stb{};
        int mx = 0;
        if (mode == M_SYRK || mode == M_SYRK_BATCH) {
            if (count > SyrkBatch::MAX || (mode == M_SYRK && count != 1)) throw make_core_error("bad block count.");
            for (int64_t y = 0; y < count; ++y, t += 10) {
                if (t[1] < 1 || t[1] > 128 || !in_list(t[0], t[1]) || !fits(t[2], t[1], t[1], out0_elems)) throw make_core_error("bad diagonal block.");
                sb.off[y] = int32_t(t[0]); sb.nb[y] = int32_t(t[1]); sb.dst[y] = t[2];
                mx = std::max(mx, int(t[1]));
            }
            sb.count = int32_t(count);
        } else if (mode == M_GRAM) {
            if (count != 1) throw make_core_error("bad block count.");
            const int64_t M = t[1], m_pos0 = t[2], N = t[4], n_pos0 = t[5];
            if (M < 1 || N < 1 || M > (1 << 20) || N > (1 << 20) || m_pos0 < 0 || n_pos0 < 0 || m_pos0 > (1 << 20) || n_pos0 > (1 << 20) ||
                !in_list(t[0], M) || !in_list(t[3], N))
                throw make_core_error("bad Gram panel.");
            // the panel and its mirror image
            const int64_t side = std::max(m_pos0 + M, n_pos0 + N);
            if (side > ldc || (side - 1) * (ldc + 1) >= out0_elems) throw make_core_error("bad Gram panel.");
        } else if (mode == M_GRAM_BATCH) {
            if (count > GramBatch::MAX) throw make_core_error("bad block count.");
            if (d->is_csc()) throw make_core_error("no batch of cross blocks on a compressed-column design.");
            for (int64_t y = 0; y < count; ++y, t += 10) {
                if (t[1] < 1 || t[1] > 128 || t[3] < 1 || t[3] > 128 || !in_list(t[0], t[1]) || !in_list(t[2], t[3]) ||
                    !fits(t[4], t[1], t[3], out0_elems))
                    throw make_core_error("bad cross block.");
                gb.moff[y] = int32_t(t[0]); gb.m[y] = int32_t(t[1]); gb.noff[y] = int32_t(t[2]); gb.nn[y] = int32_t(t[3]); gb.dst[y] = t[4];
            }
            gb.count = int32_t(count);
        } else if (mode == M_STRIP) {
            if (count > StripBatch::MAX) throw make_core_error("bad block count.");
            if (!d->is_dense()) throw make_core_error("strips are built on dense designs only.");
            for (int64_t y = 0; y < count; ++y, t += 10) {
                const int64_t m = t[1], c0n = t[3], c1n = t[5], row0 = t[6];
                if (m < 1 || m > 64 || c0n < 0 || c0n > 128 || c1n < 1 || c1n > 128 || row0 < 0 || row0 + m != c1n || !in_list(t[0], m) ||
                    !in_list(t[2], c0n) || !in_list(t[4], c1n) || !fits(t[8], c1n, c1n, out0_elems))
                    throw make_core_error("bad strip.");
                if (c0n > 0 && (!out1 || !fits(t[7], c1n, c0n, out1_elems))) throw make_core_error("bad strip (cross block).");
                stb.voff[y] = int32_t(t[0]); stb.m[y] = int32_t(m); stb.c0off[y] = int32_t(t[2]); stb.c0n[y] = int32_t(c0n);
                stb.c1off[y] = int32_t(t[4]); stb.c1n[y] = int32_t(c1n); stb.row0[y] = int32_t(row0); stb.dstX[y] = t[7]; stb.dstD[y] = t[8];
                mx = std::max(mx, int(m));
            }
            stb.count = int32_t(count);
        } else {
            throw make_core_error("unknown mode.");
        }
        AHIP_CHECK(hipSetDevice(d->device));
        hipStream_t s = d->stream;
        last_build_launch() = BuildLaunchInfo{};
        auto body = [&](auto tag) {
            using T = decltype(tag);
            DevBuf<T> dw, dxm, dC, dX, work;
            DevBuf<int32_t> dcols;
            dw.reserve(size_t(n)); dw.upload(static_cast<const T*>(w), size_t(n), s);
            dcols.reserve(size_t(n_cols)); dcols.upload(cols, size_t(n_cols), s);
            if (xm) { dxm.reserve(size_t(p)); dxm.upload(static_cast<const T*>(xm), size_t(p), s); }
            dC.reserve(size_t(out0_elems)); dC.upload(static_cast<const T*>(out0), size_t(out0_elems), s);
            if (out1) { dX.reserve(size_t(out1_elems)); dX.upload(static_cast<const T*>(out1), size_t(out1_elems), s); }
            const T* xmp = xm ? dxm.p : nullptr;
            const bool ctr = center != 0;
            DenseView<T> Xd{};
            if (d->is_dense()) {
                Xd = d->dense<T>();
                Xd.X += row_off;
                Xd.n = n;
            }
            if (mode == M_SYRK) {
                const int32_t* c = dcols.p + sb.off[0];
                T* C = dC.p + sb.dst[0];
                if (d->is_csc()) {
                    SyrkBatch one = sb;
                    one.off[0] = 0; one.dst[0] = 0;
                    launch_block_gram_csc<T>(d->csc<T>(), dw.p, c, one, xmp, ctr, C, int(ldc), s);
                } else {
                    T* wk = work.reserve(size_t(syrk_work_elems(n, sb.nb[0])));
                    if (d->is_dense()) launch_syrk<T>(Xd, dw.p, c, sb.nb[0], xmp, ctr, C, ldc, wk, s);
                    else launch_syrk_snp<T>(d->snp(), snp_impute<T>(*d), dw.p, c, sb.nb[0], xmp, ctr, C, ldc, wk, s);
                }
            } else if (mode == M_SYRK_BATCH) {
                if (d->is_csc()) {
                    launch_block_gram_csc<T>(d->csc<T>(), dw.p, dcols.p, sb, xmp, ctr, dC.p, int(ldc), s);
                } else {
                    T* wk = work.reserve(size_t(syrk_batch_work_elems(n, sb.count)));
                    if (d->is_dense()) launch_syrk_batch<T>(Xd, dw.p, dcols.p, sb, xmp, ctr, dC.p, ldc, wk, s);
                    else launch_syrk_batch_snp<T>(d->snp(), snp_impute<T>(*d), dw.p, dcols.p, sb, xmp, ctr, dC.p, ldc, wk, s);
                }
            } else if (mode == M_GRAM) {
                const int32_t M = int32_t(table[1]), N = int32_t(table[4]);
                T* wk = work.reserve(size_t(std::max<int64_t>(raw_gram_work_elems(*d, n, M, N), 1)));
                if (d->is_dense() && row_off > 0)
                    launch_gram<T>(Xd, dw.p, dcols.p + table[0], M, int32_t(table[2]), dcols.p + table[3], N, int32_t(table[5]), xmp, ctr, dC.p, ldc, wk, s);
                else
                    raw_gram<T>(*d, dw.p, dcols.p + table[0], M, int32_t(table[2]), dcols.p + table[3], N, int32_t(table[5]), xmp, ctr, dC.p, ldc, wk, s);
            } else if (mode == M_GRAM_BATCH) {
                T* wk = work.reserve(size_t(gram_batch_work_elems(n, gb.count)));
                if (d->is_dense()) launch_gram_batch<T>(Xd, dw.p, dcols.p, gb, xmp, ctr, dC.p, ldc, wk, s);
                else launch_gram_batch_snp<T>(d->snp(), snp_impute<T>(*d), dw.p, dcols.p, gb, xmp, ctr, dC.p, ldc, wk, s);
            } else {
                T* wk = work.reserve(size_t(strip_work_elems(n, stb.count, mx)));
                if (strip_plain) { set_strip_lds(false); lds_changed = true; }
                launch_strip_batch<T>(Xd, dw.p, dcols.p, stb, xmp, ctr, dC.p, out1 ? dX.p : dC.p, ldc, wk, s);
                if (lds_changed) { set_strip_lds(true); lds_changed = false; }
            }
            AHIP_CHECK(hipGetLastError());
            AHIP_CHECK(hipMemcpyAsync(out0, dC.p, size_t(out0_elems) * sizeof(T), hipMemcpyDeviceToHost, s));
            if (out1) AHIP_CHECK(hipMemcpyAsync(out1, dX.p, size_t(out1_elems) * sizeof(T), hipMemcpyDeviceToHost, s));
            AHIP_CHECK(hipStreamSynchronize(s));
        };
        if (d->dtype == ADELIE_HIP_F64) body(double{});
        else body(float{});
        const BuildLaunchInfo& r = last_build_launch();
        info[0] = r.kind; info[1] = r.nsplit; info[2] = r.kchunk; info[3] = r.tile; info[4] = r.n128; info[5] = r.n64;
        info[6] = r.vec16; info[7] = r.strip_lt; info[8] = r.symmetric;
        info[9] = d->is_csc() ? d->sp_nb : 0;
    } catch (const std::exception& e) {
        if (lds_changed) set_strip_lds(true);
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

// One device piece of the group engine on caller-supplied inputs, through the launcher the solver calls (tests; include/adelie_hip.h
// has the modes and the arrays).  Everything the kernels index by is checked here against the buffers' sizes before anything is
// launched; the outputs are written only after the last download.
int adelie_hip_group_piece_test(const adelie_hip_group_piece* a, int64_t* info) {
    try {
        if (!a || !info) throw make_core_error("bad arguments.");
        if (a->dtype != ADELIE_HIP_F64 && a->dtype != ADELIE_HIP_F32) throw make_core_error("bad dtype.");
        constexpr int64_t G = 128, SLOT = G * G;
        const int mode = int(a->mode);
        const bool solve = mode == ADELIE_HIP_GROUP_PANEL_SOLVE || mode == ADELIE_HIP_GROUP_GRAM_PASS;
        // a (q, q) eigenbasis at `off` lies inside V
        auto v_fits = [&](int64_t off, int64_t q) { return off >= 0 && off <= a->V_elems && q * q <= a->V_elems - off; };
        std::vector<EigDesc> edesc;
        GrpRotArgs rot{};
        bool rot_wide = false;
        int64_t n_pos = 0; // list positions the pass covers
        if (mode == ADELIE_HIP_GROUP_EIG) {
            if (a->count < 1 || a->count > 4096 || a->max_q < 1 || a->max_q > kEigMaxQ || !a->eig || !a->src || a->src_elems < 1 ||
                !a->vars || a->vars_elems < 1 || !a->V || a->V_elems < 1)
                throw make_core_error("EIG: bad arguments.");
            for (int64_t y = 0; y < a->count; ++y) {
                const int64_t* t = a->eig + 5 * y;
                const int64_t src = t[0], vp = t[1], vo = t[2], ld = t[3], q = t[4];
                if (q < 1 || q > a->max_q) throw make_core_error("EIG: group size outside 1 .. max_q <= " + std::to_string(kEigMaxQ) + ".");
                if (ld < 1 || ld > (int64_t(1) << 30) || src < 0 || src >= a->src_elems || (q - 1) * (ld + 1) >= a->src_elems - src)
                    throw make_core_error("EIG: block outside the source.");
                if (vp < 0 || vp > a->vars_elems || q > a->vars_elems - vp) throw make_core_error("EIG: variances outside vars.");
                if (q > 1 && !v_fits(vo, q)) throw make_core_error("EIG: eigenbasis outside V.");
                edesc.push_back(EigDesc{src, vp, vo, int32_t(ld), int32_t(q)});
            }
        } else if (mode == ADELIE_HIP_GROUP_ROTATE) {
            if (a->ng < 1 || a->ng > G || !a->goff || !a->rvoff || !a->D || !a->V || a->V_elems < 1) throw make_core_error("ROTATE: bad arguments.");
            if (a->goff[0] != 0) throw make_core_error("ROTATE: goff[0] must be 0.");
            rot.ng = int32_t(a->ng);
            for (int64_t k = 0; k < a->ng; ++k) {
                const int64_t q = int64_t(a->goff[k + 1]) - a->goff[k];
                if (q < 1 || a->goff[k + 1] > G) throw make_core_error("ROTATE: groups must be non-empty and hold at most 128 values together.");
                if (q > 1 && !v_fits(a->rvoff[k], q)) throw make_core_error("ROTATE: eigenbasis outside V.");
                rot.goff[k] = a->goff[k];
                rot.voff[k] = q > 1 ? a->rvoff[k] : 0;
                rot_wide = rot_wide || q > 16;
            }
            for (int64_t k = a->ng; k <= G; ++k) rot.goff[k] = a->goff[a->ng];
        } else if (mode == ADELIE_HIP_GROUP_LAYOUT || solve) {
            if (a->ns < 1 || a->ns > (1 << 20) || a->nv < 1 || a->nv > (1 << 20) || a->nblk < 1 || a->nblk > 4096 || !a->sbegin || !a->ssize ||
                !a->voff || !a->blk_g0 || !a->desc || (a->list && a->n_list < 1))
                throw make_core_error("bad arguments.");
            for (int64_t ss = 0; ss < a->ns; ++ss) {
                const int64_t b = a->sbegin[ss], q = a->ssize[ss];
                if (q < 1 || b < 0 || b > a->nv || q > a->nv - b) throw make_core_error("a screen group lies outside the screen values.");
                if (q > 1 && solve && !v_fits(a->voff[ss], q)) throw make_core_error("eigenbasis outside V.");
                if (q > 1 && (a->voff[ss] < 0 || a->voff[ss] > INT32_MAX)) throw make_core_error("voff out of range.");
            }
            n_pos = a->list ? a->n_list : a->ns;
            std::vector<char> seen(size_t(a->ns), 0);
            if (a->list)
                for (int64_t i = 0; i < a->n_list; ++i) {
                    if (a->list[i] < 0 || a->list[i] >= a->ns) throw make_core_error("list index out of range.");
                    if (seen[size_t(a->list[i])]++) throw make_core_error("list names a group twice.");
                }
            if (a->blk_g0[0] < 0) throw make_core_error("blk_g0 must start at >= 0.");
            for (int64_t j = 0; j < a->nblk; ++j) {
                const int64_t g0 = a->blk_g0[j], g1 = a->blk_g0[j + 1];
                if (g1 <= g0 || g1 - g0 > G || g1 > n_pos) throw make_core_error("blk_g0 must increase, by at most 128, inside the list.");
                int64_t nval = 0;
                for (int64_t g = g0; g < g1; ++g) nval += a->ssize[a->list ? a->list[g] : g];
                if (nval > G) throw make_core_error("a block holds more than 128 values.");
            }
            if (solve) {
                if (!a->vars || a->vars_elems < a->nv || !a->V || a->V_elems < 1 || !a->xmean || !a->spen || !a->vcol || !a->beta || !a->is_active ||
                    !a->active_set || !a->st_f || !a->st_i)
                    throw make_core_error("solve: bad arguments.");
                if (a->max_active_size < 0 || a->max_active_size > INT32_MAX) throw make_core_error("max_active_size must be >= 0.");
                if (a->active_size < 0 || a->active_size > a->ns) throw make_core_error("active_size outside 0 .. ns.");
                if (a->newton_max_iters < 0 || a->newton_max_iters > INT32_MAX || !(a->newton_tol >= 0) || !(a->dbeta_tol >= 0))
                    throw make_core_error("bad Newton / change tolerances.");
                for (int64_t i = 0; i < a->nv; ++i)
                    if (a->vcol[i] < 0) throw make_core_error("vcol out of range.");
                if (mode == ADELIE_HIP_GROUP_PANEL_SOLVE && (!a->Dblk || !a->gblk || !a->dcol || !a->dlt || !a->dd))
                    throw make_core_error("PANEL_SOLVE: bad arguments.");
                if (mode == ADELIE_HIP_GROUP_GRAM_PASS && (!a->C || !a->g || a->ldc < a->nv || a->ldc > (1 << 20)))
                    throw make_core_error("GRAM_PASS: bad arguments.");
            }
        } else {
            throw make_core_error("unknown mode.");
        }
        AHIP_CHECK(hipSetDevice(0));
        hipStream_t s = nullptr;
        int64_t launches = 0;
        auto body = [&](auto tag) {
            using T = decltype(tag);
            auto up = [&](auto& buf, const auto* h, int64_t n) { buf.reserve(size_t(n)); buf.upload(h, size_t(n), s); };
            auto down = [&](void* h, const void* dev, size_t bytes) { AHIP_CHECK(hipMemcpyAsync(h, dev, bytes, hipMemcpyDeviceToHost, s)); };
            if (mode == ADELIE_HIP_GROUP_EIG) {
                DevBuf<T> dsrc, dvars, dV;
                DevBuf<EigDesc> dd;
                up(dsrc, static_cast<const T*>(a->src), a->src_elems);
                up(dvars, static_cast<const T*>(a->vars), a->vars_elems);
                up(dV, static_cast<const T*>(a->V), a->V_elems);
                up(dd, edesc.data(), int64_t(edesc.size()));
                launch_grp_eig<T>(dsrc.p, dd.p, int(a->count), int(a->max_q), dvars.p, dV.p, s);
                ++launches;
                AHIP_CHECK(hipGetLastError());
                std::vector<T> hvars(size_t(a->vars_elems)), hV(size_t(a->V_elems));
                down(hvars.data(), dvars.p, hvars.size() * sizeof(T));
                down(hV.data(), dV.p, hV.size() * sizeof(T));
                AHIP_CHECK(hipStreamSynchronize(s));
                std::memcpy(a->vars, hvars.data(), hvars.size() * sizeof(T));
                std::memcpy(a->V, hV.data(), hV.size() * sizeof(T));
                return;
            }
            if (mode == ADELIE_HIP_GROUP_ROTATE) {
                DevBuf<T> dD, dS, dV, scratch;
                up(dD, static_cast<const T*>(a->D), SLOT);
                if (a->Dsrc) up(dS, static_cast<const T*>(a->Dsrc), SLOT);
                up(dV, static_cast<const T*>(a->V), a->V_elems);
                scratch.reserve(size_t(SLOT));
                launch_grp_block_rotate<T>(dD.p, a->Dsrc ? dS.p : dD.p, dV.p, rot, scratch.p, s);
                ++launches;
                AHIP_CHECK(hipGetLastError());
                std::vector<T> hD(static_cast<size_t>(SLOT));
                down(hD.data(), dD.p, hD.size() * sizeof(T));
                AHIP_CHECK(hipStreamSynchronize(s));
                std::memcpy(a->D, hD.data(), hD.size() * sizeof(T));
                return;
            }
            const int64_t nblk = a->nblk, ns = a->ns, nv = a->nv;
            DevBuf<int32_t> dsb, dsz, dg0, dlist, ddesc, dvcol, dact, ddcol, ddidx;
            DevBuf<int64_t> dvoff;
            DevBuf<int8_t> disact;
            DevBuf<T> dvars, dV, dxm, dspen, dbeta, dg, dC, dDb, dgb, ddlt, ddd, dDbuf;
            DevBuf<CdBlkState<T>> dst;
            up(dsb, a->sbegin, ns); up(dsz, a->ssize, ns); up(dvoff, a->voff, ns); up(dg0, a->blk_g0, nblk + 1);
            if (a->list) up(dlist, a->list, a->n_list);
            ddesc.reserve(size_t(nblk * GDESC_STRIDE));
            AHIP_CHECK(hipMemsetAsync(ddesc.p, 0, size_t(nblk * GDESC_STRIDE) * sizeof(int32_t), s)); // (the unnamed gaps)
            CdGrpBlkParams<T> p{};
            p.nv = int32_t(nv);
            p.sbegin = dsb.p; p.ssize = dsz.p; p.voff = dvoff.p; p.blk_g0 = dg0.p; p.list = a->list ? dlist.p : nullptr;
            p.nblk = int32_t(nblk);
            launch_grp_layout<T>(p, int(nblk), ddesc.p, s);
            ++launches;
            AHIP_CHECK(hipGetLastError());
            std::vector<int32_t> hdesc(size_t(nblk * GDESC_STRIDE));
            down(hdesc.data(), ddesc.p, hdesc.size() * sizeof(int32_t));
            if (!solve) {
                AHIP_CHECK(hipStreamSynchronize(s));
                std::memcpy(a->desc, hdesc.data(), hdesc.size() * sizeof(int32_t));
                return;
            }
            const bool panel = mode == ADELIE_HIP_GROUP_PANEL_SOLVE;
            up(dvars, static_cast<const T*>(a->vars), nv); up(dV, static_cast<const T*>(a->V), a->V_elems);
            up(dxm, static_cast<const T*>(a->xmean), nv); up(dspen, static_cast<const T*>(a->spen), ns);
            up(dbeta, static_cast<const T*>(a->beta), nv); up(dvcol, a->vcol, nv); up(disact, a->is_active, ns);
            dact.reserve(size_t(2 * ns + 1)); // a group is marked at most once: active_size <= ns on entry, at most ns more
            dact.upload(a->active_set, size_t(ns), s);
            CdBlkState<T> st0{};
            st0.rsq = T(a->rsq); st0.resid_sum = T(a->resid_sum); st0.n_updates = a->n_updates; st0.active_size = int32_t(a->active_size);
            up(dst, &st0, 1);
            p.vars = dvars.p; p.xmean = dxm.p; p.beta = dbeta.p; p.is_active = disact.p; p.active_set = dact.p;
            p.l1 = T(a->l1); p.l2 = T(a->l2); p.newton_tol = T(a->newton_tol); p.dbeta_tol = T(a->dbeta_tol);
            p.newton_max_iters = int32_t(a->newton_max_iters); p.max_active_size = int32_t(a->max_active_size); p.mark = a->mark ? 1 : 0;
            p.V = dV.p; p.spen = dspen.p; p.st = dst.p; p.vcol = dvcol.p;
            std::vector<CdBlkState<T>> hst(size_t(panel ? nblk : 1));
            std::vector<T> hdlt, hdd, hbeta(static_cast<size_t>(nv)), hg;
            std::vector<int32_t> hdcol, hact(static_cast<size_t>(ns));
            std::vector<int8_t> hisact(static_cast<size_t>(ns));
            if (panel) {
                up(dDb, static_cast<const T*>(a->Dblk), nblk * SLOT); up(dgb, static_cast<const T*>(a->gblk), nblk * G);
                up(ddlt, static_cast<const T*>(a->dlt), nblk * G); up(ddd, static_cast<const T*>(a->dd), nblk * G); up(ddcol, a->dcol, nblk * G);
                p.rot = 1; p.desc = ddesc.p;
                for (int64_t j = 0; j < nblk; ++j) {
                    p.Dptr = dDb.p + j * SLOT; p.gblk = dgb.p + j * G;
                    p.dlt = ddlt.p + j * G; p.dd = ddd.p + j * G; p.dcol = ddcol.p + j * G;
                    launch_cd_group_panel_solve<T>(p, int(j), s);
                    ++launches;
                    down(&hst[size_t(j)], dst.p, sizeof(CdBlkState<T>));
                }
                AHIP_CHECK(hipGetLastError());
                hdlt.resize(size_t(nblk * G)); hdd.resize(size_t(nblk * G)); hdcol.resize(size_t(nblk * G));
                down(hdlt.data(), ddlt.p, hdlt.size() * sizeof(T)); down(hdd.data(), ddd.p, hdd.size() * sizeof(T));
                down(hdcol.data(), ddcol.p, hdcol.size() * sizeof(int32_t));
            } else {
                dC.reserve(size_t(a->ldc * nv)); dC.upload(static_cast<const T*>(a->C), size_t(a->ldc * nv), s);
                up(dg, static_cast<const T*>(a->g), nv);
                dDbuf.reserve(size_t(2 * SLOT)); ddlt.reserve(size_t(G)); ddidx.reserve(size_t(G));
                p.C = dC.p; p.ldc = a->ldc; p.g = dg.p; p.Dbuf = dDbuf.p; p.dlt = ddlt.p; p.didx = ddidx.p; p.rot = 0;
                launch_cd_group_block_pass<T>(p, s);
                launches += 1 + 2 * nblk;
                AHIP_CHECK(hipGetLastError());
                down(&hst[0], dst.p, sizeof(CdBlkState<T>));
                hg.resize(size_t(nv));
                down(hg.data(), dg.p, hg.size() * sizeof(T));
            }
            down(hbeta.data(), dbeta.p, hbeta.size() * sizeof(T));
            down(hact.data(), dact.p, hact.size() * sizeof(int32_t));
            down(hisact.data(), disact.p, hisact.size());
            AHIP_CHECK(hipStreamSynchronize(s));
            std::memcpy(a->desc, hdesc.data(), hdesc.size() * sizeof(int32_t));
            std::memcpy(a->beta, hbeta.data(), hbeta.size() * sizeof(T));
            std::memcpy(a->active_set, hact.data(), hact.size() * sizeof(int32_t));
            std::memcpy(a->is_active, hisact.data(), hisact.size());
            if (panel) {
                std::memcpy(a->dlt, hdlt.data(), hdlt.size() * sizeof(T));
                std::memcpy(a->dd, hdd.data(), hdd.size() * sizeof(T));
                std::memcpy(a->dcol, hdcol.data(), hdcol.size() * sizeof(int32_t));
            } else {
                std::memcpy(a->g, hg.data(), hg.size() * sizeof(T));
            }
            for (size_t j = 0; j < hst.size(); ++j) {
                a->st_f[3 * j] = double(hst[j].rsq); a->st_f[3 * j + 1] = double(hst[j].resid_sum); a->st_f[3 * j + 2] = double(hst[j].cm);
                a->st_i[4 * j] = hst[j].n_updates; a->st_i[4 * j + 1] = hst[j].active_size; a->st_i[4 * j + 2] = hst[j].status;
                a->st_i[4 * j + 3] = hst[j].nz;
            }
        };
        if (a->dtype == ADELIE_HIP_F64) body(double{});
        else body(float{});
        info[0] = launches;
        info[1] = rot_wide ? 1 : 0;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

// One launcher of kernels_multi.hip on caller-supplied inputs (tests; include/adelie_hip.h has the modes and the arrays).  Everything
// the kernels index by is checked here against the buffers' sizes before anything is launched; the outputs are written only after
// the last download.
int adelie_hip_multi_piece_test(const adelie_hip_multi_piece* a, int64_t* info) {
    try {
        if (!a || !info) throw make_core_error("bad arguments.");
        if (a->dtype != ADELIE_HIP_F64 && a->dtype != ADELIE_HIP_F32) throw make_core_error("bad dtype.");
        constexpr int64_t G = 128, SLOT = G * G, BIG = int64_t(1) << 24;
        const int mode = int(a->mode);
        if (a->mode < ADELIE_HIP_MULTI_SWEEP || a->mode > ADELIE_HIP_MULTI_BATCH_PICK) throw make_core_error("unknown mode.");
        const bool step = mode == ADELIE_HIP_MULTI_STEP || mode == ADELIE_HIP_MULTI_FUSED_STEP;
        const bool view = mode == ADELIE_HIP_MULTI_SWEEP || step || mode == ADELIE_HIP_MULTI_AXPY;
        const int64_t nb = a->nb, pb = a->pb, K = a->K, icpt = a->icpt;
        const int64_t ncol = (pb + icpt) * K; // view columns
        auto in_cols = [&](const int32_t* list, int64_t n, const char* what) {
            if (n > 0 && !list) throw make_core_error(std::string(what) + ": null list.");
            for (int64_t m = 0; m < n; ++m)
                if (list[m] < 0 || list[m] >= ncol) throw make_core_error(std::string(what) + ": column index outside [0, (pb + icpt) K).");
        };
        if (view) {
            if (nb < 1 || nb > BIG || pb < 1 || pb > (1 << 20) || K < 1 || K > 64 || (icpt != 0 && icpt != 1) || ncol > BIG)
                throw make_core_error("view: 1 <= nb, pb, 1 <= K <= 64 and icpt in {0, 1} are required.");
            if (a->bits) {
                if (a->ldb < (nb + 3) / 4 || a->ldb > BIG || a->bits_elems < 1 || a->bits_elems > (int64_t(1) << 28) || pb * a->ldb > a->bits_elems || !a->impute)
                    throw make_core_error("view: the 2-bit base needs ldb >= (nb + 3) / 4, pb ldb <= bits_elems and impute.");
            } else {
                if (!a->X || a->ld < nb || a->ld > BIG || a->X_elems < 1 || a->X_elems > (int64_t(1) << 28) || pb * a->ld > a->X_elems || a->x_off < 0 || a->x_off > 64)
                    throw make_core_error("view: the dense base needs ld >= nb, pb ld <= X_elems and 0 <= x_off <= 64.");
            }
        }
        int64_t n_used = 0; // entries of dcol / dlt the kernel may read
        if (mode == ADELIE_HIP_MULTI_SWEEP) {
            if (!a->v || !a->out || a->v_off < 0 || a->v_off > 64) throw make_core_error("SWEEP: v, out and 0 <= v_off <= 64 are required.");
        } else if (step) {
            const int64_t max_cols = mode == ADELIE_HIP_MULTI_STEP ? 2 * G : G;
            if (!a->w || !a->r || !a->part || a->nz < 0 || a->nz > INT32_MAX || a->n_dcol < 0 || a->n_dcol > G || a->nb_cols < 0 ||
                a->nb_cols > max_cols || a->part_elems < 1 || a->part_elems > (int64_t(1) << 28))
                throw make_core_error("STEP: w, r, part, n_dcol <= 128 and nb_cols <= 256 (128 in the fused step) are required.");
            n_used = std::min<int64_t>(a->nz, G);
            if (n_used > a->n_dcol || (n_used > 0 && !a->dlt)) throw make_core_error("STEP: dcol / dlt hold fewer than min(nz, 128) entries.");
            in_cols(a->dcol, a->n_dcol, "STEP dcol");
            in_cols(a->cols, a->nb_cols, "STEP cols");
        } else if (mode == ADELIE_HIP_MULTI_AXPY) {
            if (!a->r || a->n_dcol < 0 || a->n_dcol > 4096 || a->nz < 0 || a->nz > a->n_dcol || (a->nz > 0 && !a->dlt))
                throw make_core_error("AXPY: r and 0 <= nz <= n_dcol <= 4096 are required.");
            n_used = a->nz;
            in_cols(a->dcol, a->n_dcol, "AXPY dcol");
        } else if (mode == ADELIE_HIP_MULTI_BLOCK_LISTS) {
            if (a->nv < 1 || a->nv > G || K < 1 || K > (1 << 20) || !a->cols || !a->ulist || !a->slot || !a->resp)
                throw make_core_error("BLOCK_LISTS: 1 <= nv <= 128, K >= 1, cols, ulist, slot and resp are required.");
            for (int64_t m = 0; m < a->nv; ++m)
                if (a->cols[m] < 0) throw make_core_error("BLOCK_LISTS: negative column index.");
        } else if (mode == ADELIE_HIP_MULTI_EXPAND || mode == ADELIE_HIP_MULTI_EXPAND_CROSS) {
            const bool cross = mode == ADELIE_HIP_MULTI_EXPAND_CROSS;
            const int64_t nr = a->nv, ncc = cross ? a->nc : a->nv;
            if (nr < 1 || nr > G || ncc < 1 || ncc > G || !a->slot || !a->resp || !a->C || !a->D || a->ldc < 1 || a->ldc > BIG ||
                a->C_elems < 1 || a->C_elems > (int64_t(1) << 28) || a->ldd < nr || a->ldd > BIG || a->D_elems > (int64_t(1) << 28) ||
                (ncc - 1) * a->ldd + nr > a->D_elems || (cross && (!a->slot_c || !a->resp_c)))
                throw make_core_error("EXPAND: 1 <= nv, nc <= 128, slot, resp, C, D with ldd >= nv and (nc - 1) ldd + nv <= D_elems are required.");
            const int32_t* sc = cross ? a->slot_c : a->slot;
            int64_t mr = 0, mc = 0;
            for (int64_t m = 0; m < nr; ++m) {
                if (a->slot[m] < 0) throw make_core_error("EXPAND: negative slot.");
                mr = std::max<int64_t>(mr, a->slot[m]);
            }
            for (int64_t m = 0; m < ncc; ++m) {
                if (sc[m] < 0) throw make_core_error("EXPAND: negative slot.");
                mc = std::max<int64_t>(mc, sc[m]);
            }
            if (mr >= a->ldc || mr + mc * a->ldc >= a->C_elems) throw make_core_error("EXPAND: a slot lies outside C.");
            if (!cross) {
                if (a->n_lsel < 1 || a->n_lsel > 64 || !a->lsel_list) throw make_core_error("EXPAND: 1 <= n_lsel <= 64 and lsel_list are required.");
                for (int64_t q = 0; q < a->n_lsel; ++q)
                    if (a->lsel_list[q] < -1 || a->lsel_list[q] > (1 << 20)) throw make_core_error("EXPAND: lsel out of range.");
            }
        } else if (mode == ADELIE_HIP_MULTI_TO_MAJOR || mode == ADELIE_HIP_MULTI_FROM_MAJOR) {
            if (nb < 1 || K < 1 || nb > BIG || K > BIG || nb * K > (int64_t(1) << 26) || !a->v || !a->out)
                throw make_core_error("TO_MAJOR / FROM_MAJOR: nb, K >= 1, v and out are required.");
        } else { // BATCH_PICK
            if (pb < 1 || K < 1 || pb > BIG || K > BIG || pb * K > (int64_t(1) << 26) || a->lsel < 0 || a->lsel >= K || !a->v || !a->out)
                throw make_core_error("BATCH_PICK: pb, K >= 1, 0 <= lsel < K, v and out are required.");
        }
        AHIP_CHECK(hipSetDevice(0));
        hipStream_t s = nullptr;
        for (int q = 0; q < 8; ++q) info[q] = 0;
        auto body = [&](auto tag) {
            using T = decltype(tag);
            auto up = [&](auto& buf, const auto* h, int64_t n) { buf.reserve(size_t(n)); buf.upload(h, size_t(n), s); };
            auto down = [&](void* h, const void* dev, size_t bytes) { AHIP_CHECK(hipMemcpyAsync(h, dev, bytes, hipMemcpyDeviceToHost, s)); };
            auto finish = [&](void* dst, std::vector<T>& h, const T* dev) { // download, synchronise, then write the caller's array
                AHIP_CHECK(hipGetLastError());
                down(h.data(), dev, h.size() * sizeof(T));
                AHIP_CHECK(hipStreamSynchronize(s));
                std::memcpy(dst, h.data(), h.size() * sizeof(T));
            };
            DevBuf<T> dX, dimp, dv, dout, dw, dr, ddlt, dpart, dwork;
            DevBuf<uint8_t> dbits;
            DevBuf<int32_t> ddcol, dcols, dnz;
            DevArr<void> ones;
            MultiView<T> mv{};
            if (view) {
                alloc_multi_ones<T>(ones, nb, s);
                mv.nb = nb; mv.pb = pb; mv.K = int32_t(K); mv.icpt = int32_t(icpt);
                mv.ones = static_cast<const T*>(ones.get());
                if (a->bits) {
                    up(dbits, a->bits, a->bits_elems);
                    up(dimp, static_cast<const T*>(a->impute), pb);
                    mv.bits = dbits.p; mv.ldb = a->ldb; mv.impute = dimp.p;
                } else {
                    dX.reserve(size_t(a->X_elems + a->x_off + 64));
                    dX.upload(static_cast<const T*>(a->X), size_t(a->X_elems), s, size_t(a->x_off));
                    mv.X = dX.p + a->x_off; mv.ld = a->ld;
                }
            }
            if (mode == ADELIE_HIP_MULTI_SWEEP) {
                dv.reserve(size_t(nb * K + a->v_off + 64));
                dv.upload(static_cast<const T*>(a->v), size_t(nb * K), s, size_t(a->v_off));
                up(dout, static_cast<const T*>(a->out), ncol);
                dwork.reserve(size_t(multi_sweep_work_elems<T>(mv)));
                const T* v = dv.p + a->v_off;
                const MSweepPlan pl = multi_sweep_plan<T>(mv, v);
                if (int64_t(pl.nsplit) * ncol > multi_sweep_work_elems<T>(mv)) throw make_core_error("SWEEP: the work size does not cover the plan.");
                launch_multi_sweep<T>(mv, v, dout.p, dwork.p, s);
                info[0] = pl.variant; info[1] = pl.vec; info[2] = pl.kt; info[3] = pl.feats; info[4] = pl.blocks_c; info[5] = pl.nsplit;
                info[6] = pl.rows_per_split; info[7] = pl.kchunks;
                std::vector<T> h(static_cast<size_t>(ncol));
                finish(a->out, h, dout.p);
                return;
            }
            if (step || mode == ADELIE_HIP_MULTI_AXPY) {
                up(dr, static_cast<const T*>(a->r), nb * K);
                ddcol.reserve(size_t(G)); ddlt.reserve(size_t(G));
                if (a->n_dcol > 0) up(ddcol, a->dcol, a->n_dcol);
                if (n_used > 0) up(ddlt, static_cast<const T*>(a->dlt), a->n_dcol);
                const int32_t nz32 = int32_t(a->nz);
                up(dnz, &nz32, 1);
            }
            if (mode == ADELIE_HIP_MULTI_AXPY) {
                launch_multi_axpy_cols<T>(mv, ddcol.p, ddlt.p, dnz.p, T(a->sign), dr.p, s);
                std::vector<T> h(static_cast<size_t>(nb * K));
                finish(a->r, h, dr.p);
                return;
            }
            if (step) {
                const bool fused = mode == ADELIE_HIP_MULTI_FUSED_STEP;
                const int vec = multi_step_vec<T>(mv);
                const int64_t ld = fused ? mfused_part_ld(nb, vec) : mstep_slices(nb, vec);
                if (a->nb_cols * ld > a->part_elems) throw make_core_error("STEP: part holds fewer than nb_cols * slices elements.");
                up(dw, static_cast<const T*>(a->w), nb * K);
                up(dpart, static_cast<const T*>(a->part), a->part_elems);
                dcols.reserve(size_t(2 * G));
                if (a->nb_cols > 0) up(dcols, a->cols, a->nb_cols);
                int got = 0;
                // the solve half of the fused launch: one singleton group, zero gradient, a penalty above it (set up as the
                // PANEL_SOLVE mode of adelie_hip_group_piece_test sets up its block): it changes nothing
                DevBuf<int32_t> dsb, dsz, dg0, ddesc, dvcol, dact, dsdcol;
                DevBuf<int64_t> dvoff;
                DevBuf<int8_t> disact;
                DevBuf<T> dvars, dV, dxm, dspen, dbeta, dDb, dgb, dsdlt, dsdd;
                DevBuf<CdBlkState<T>> dst;
                if (fused) {
                    const int32_t zero32 = 0, one32 = 1, g0[2] = {0, 1};
                    const int64_t zero64 = 0;
                    const int8_t zero8 = 0;
                    const T one = T(1), zero = T(0);
                    up(dsb, &zero32, 1); up(dsz, &one32, 1); up(dvoff, &zero64, 1); up(dg0, g0, 2);
                    ddesc.reserve(size_t(GDESC_STRIDE));
                    AHIP_CHECK(hipMemsetAsync(ddesc.p, 0, size_t(GDESC_STRIDE) * sizeof(int32_t), s));
                    CdGrpBlkParams<T> p{};
                    p.nv = 1;
                    p.sbegin = dsb.p; p.ssize = dsz.p; p.voff = dvoff.p; p.blk_g0 = dg0.p; p.list = nullptr;
                    p.nblk = 1;
                    launch_grp_layout<T>(p, 1, ddesc.p, s);
                    up(dvars, &one, 1); up(dV, &one, 1); up(dxm, &zero, 1); up(dspen, &one, 1); up(dbeta, &zero, 1);
                    up(dvcol, &zero32, 1); up(disact, &zero8, 1);
                    dact.reserve(3);
                    AHIP_CHECK(hipMemsetAsync(dact.p, 0, 3 * sizeof(int32_t), s));
                    CdBlkState<T> st0{};
                    up(dst, &st0, 1);
                    dDb.reserve(size_t(SLOT)); dgb.reserve(size_t(G)); dsdlt.reserve(size_t(G)); dsdd.reserve(size_t(G)); dsdcol.reserve(size_t(G));
                    AHIP_CHECK(hipMemsetAsync(dDb.p, 0, size_t(SLOT) * sizeof(T), s));
                    AHIP_CHECK(hipMemsetAsync(dgb.p, 0, size_t(G) * sizeof(T), s));
                    AHIP_CHECK(hipMemsetAsync(dsdlt.p, 0, size_t(G) * sizeof(T), s));
                    AHIP_CHECK(hipMemsetAsync(dsdd.p, 0, size_t(G) * sizeof(T), s));
                    AHIP_CHECK(hipMemsetAsync(dsdcol.p, 0, size_t(G) * sizeof(int32_t), s));
                    p.vars = dvars.p; p.xmean = dxm.p; p.beta = dbeta.p; p.is_active = disact.p; p.active_set = dact.p;
                    p.l1 = T(1); p.l2 = T(0); p.newton_tol = T(1e-6); p.dbeta_tol = T(0);
                    p.newton_max_iters = 10; p.max_active_size = 1; p.mark = 0;
                    p.V = dV.p; p.spen = dspen.p; p.st = dst.p; p.vcol = dvcol.p;
                    p.rot = 1; p.desc = ddesc.p;
                    p.Dptr = dDb.p; p.gblk = dgb.p; p.dlt = dsdlt.p; p.dd = dsdd.p; p.dcol = dsdcol.p;
                    got = launch_multi_panel_fused<T>(p, 0, mv, dw.p, dr.p, ddcol.p, ddlt.p, dnz.p, dcols.p, int(a->nb_cols), dpart.p, s);
                } else {
                    got = launch_multi_panel_step<T>(mv, dw.p, dr.p, ddcol.p, ddlt.p, dnz.p, dcols.p, int(a->nb_cols), dpart.p, s);
                }
                AHIP_CHECK(hipGetLastError());
                info[0] = got; info[1] = vec;
                std::vector<T> hr(static_cast<size_t>(nb * K)), hp(static_cast<size_t>(a->part_elems));
                down(hr.data(), dr.p, hr.size() * sizeof(T));
                down(hp.data(), dpart.p, hp.size() * sizeof(T));
                AHIP_CHECK(hipStreamSynchronize(s));
                if (got != ld) throw make_core_error("STEP: the launcher's leading dimension differs from the one part was sized for.");
                std::memcpy(a->r, hr.data(), hr.size() * sizeof(T));
                std::memcpy(a->part, hp.data(), hp.size() * sizeof(T));
                return;
            }
            if (mode == ADELIE_HIP_MULTI_BLOCK_LISTS) {
                DevBuf<int32_t> du, dsl, drs;
                up(dcols, a->cols, a->nv); up(du, a->ulist, a->nv); up(dsl, a->slot, a->nv); up(drs, a->resp, a->nv);
                launch_multi_block_lists(dcols.p, int(a->nv), int(K), du.p, dsl.p, drs.p, s);
                AHIP_CHECK(hipGetLastError());
                std::vector<int32_t> h(size_t(3 * a->nv));
                down(h.data(), du.p, size_t(a->nv) * 4); down(h.data() + a->nv, dsl.p, size_t(a->nv) * 4); down(h.data() + 2 * a->nv, drs.p, size_t(a->nv) * 4);
                AHIP_CHECK(hipStreamSynchronize(s));
                std::memcpy(a->ulist, h.data(), size_t(a->nv) * 4);
                std::memcpy(a->slot, h.data() + a->nv, size_t(a->nv) * 4);
                std::memcpy(a->resp, h.data() + 2 * a->nv, size_t(a->nv) * 4);
                return;
            }
            if (mode == ADELIE_HIP_MULTI_EXPAND || mode == ADELIE_HIP_MULTI_EXPAND_CROSS) {
                DevBuf<int32_t> dsl, drs, dslc, drsc;
                DevBuf<T> dC, dD;
                up(dsl, a->slot, a->nv); up(drs, a->resp, a->nv);
                up(dC, static_cast<const T*>(a->C), a->C_elems); up(dD, static_cast<const T*>(a->D), a->D_elems);
                if (mode == ADELIE_HIP_MULTI_EXPAND) {
                    for (int64_t q = 0; q < a->n_lsel; ++q)
                        launch_multi_expand<T>(dC.p, a->ldc, dsl.p, drs.p, int(a->nv), int(a->lsel_list[q]), dD.p, a->ldd, s);
                } else {
                    up(dslc, a->slot_c, a->nc); up(drsc, a->resp_c, a->nc);
                    launch_multi_expand_cross<T>(dC.p, a->ldc, dsl.p, drs.p, int(a->nv), dslc.p, drsc.p, int(a->nc), dD.p, a->ldd, s);
                }
                std::vector<T> h(static_cast<size_t>(a->D_elems));
                finish(a->D, h, dD.p);
                return;
            }
            if (mode == ADELIE_HIP_MULTI_TO_MAJOR || mode == ADELIE_HIP_MULTI_FROM_MAJOR) {
                up(dv, static_cast<const T*>(a->v), nb * K); up(dout, static_cast<const T*>(a->out), nb * K);
                if (mode == ADELIE_HIP_MULTI_TO_MAJOR) launch_multi_to_major<T>(dv.p, nb, int(K), dout.p, s);
                else launch_multi_from_major<T>(dv.p, nb, int(K), dout.p, s);
                std::vector<T> h(static_cast<size_t>(nb * K));
                finish(a->out, h, dout.p);
                return;
            }
            // BATCH_PICK
            up(dv, static_cast<const T*>(a->v), pb * K); up(dout, static_cast<const T*>(a->out), pb);
            const T scale = T(a->sign);
            up(dr, &scale, 1);
            if (a->w) up(dw, static_cast<const T*>(a->w), pb);
            launch_batch_pick<T>(dv.p, pb, int(K), int(a->lsel), dr.p, a->w ? dw.p : nullptr, dout.p, s);
            std::vector<T> h(static_cast<size_t>(pb));
            finish(a->out, h, dout.p);
        };
        if (a->dtype == ADELIE_HIP_F64) body(double{});
        else body(float{});
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

// One of the two places where the path solver touches the covariance matrix A, through the dispatcher the solver calls
// (design_ops.hpp: raw_cov_gather / raw_cov_grad), on either storage (tests; include/adelie_hip.h has the arguments).  Everything
// the kernels index by is checked here before anything is launched.
int adelie_hip_cov_piece_test(adelie_hip_design* A, int what, const int32_t* vcol, int64_t nv, int64_t pos0, int64_t N, int64_t ldc,
                              double sentinel, const void* v, const int32_t* cols, const void* coef, int64_t count, void* out) {
    try {
        if (!A || !out) throw make_core_error("bad arguments.");
        if (!A->cov) throw make_core_error("A must be a covariance matrix (matrix.dense(method=\"cov\")).");
        const int64_t p = A->p;
        const bool gather = what == ADELIE_HIP_COV_PIECE_GATHER;
        if (!gather && what != ADELIE_HIP_COV_PIECE_GRAD) throw make_core_error("unknown piece.");
        const int32_t* list = gather ? vcol : cols;
        const int64_t n_list = gather ? nv : count;
        if (gather && (!vcol || nv < 1 || nv > p || pos0 < 0 || N < 1 || pos0 + N != nv || ldc < nv || ldc > (int64_t(1) << 20)))
            throw make_core_error("GATHER: vcol (nv), 1 <= nv <= p, pos0 + N == nv and nv <= ldc are required.");
        if (!gather && (!v || count < 0 || count > p || (count > 0 && (!cols || !coef))))
            throw make_core_error("GRAD: v (p), cols and coef (count), 0 <= count <= p are required.");
        std::vector<uint8_t> seen(size_t(p), 0);
        for (int64_t k = 0; k < n_list; ++k) {
            if (list[k] < 0 || list[k] >= p || seen[size_t(list[k])]) throw make_core_error("the columns must be distinct and in [0, p).");
            seen[size_t(list[k])] = 1;
        }
        AHIP_CHECK(hipSetDevice(A->device));
        hipStream_t s = A->stream;
        auto body = [&](auto tag) {
            using T = decltype(tag);
            DevBuf<int32_t> dlist, dpos, dcnt;
            dlist.reserve(size_t(n_list) + 1);
            if (n_list) AHIP_CHECK(hipMemcpyAsync(dlist.p, list, size_t(n_list) * sizeof(int32_t), hipMemcpyHostToDevice, s));
            if (gather) {
                DevBuf<T> dC;
                std::vector<T> hC(size_t(ldc) * size_t(nv), T(sentinel));
                dC.reserve(hC.size());
                dpos.reserve(size_t(p));
                AHIP_CHECK(hipMemcpyAsync(dC.p, hC.data(), hC.size() * sizeof(T), hipMemcpyHostToDevice, s));
                if (pos0 > 0) raw_cov_gather<T>(*A, dlist.p, int32_t(pos0), 0, int32_t(pos0), dC.p, ldc, dpos.p, s);
                raw_cov_gather<T>(*A, dlist.p, int32_t(nv), int32_t(pos0), int32_t(N), dC.p, ldc, dpos.p, s);
                AHIP_CHECK(hipGetLastError());
                AHIP_CHECK(hipMemcpyAsync(out, dC.p, hC.size() * sizeof(T), hipMemcpyDeviceToHost, s));
                AHIP_CHECK(hipStreamSynchronize(s));
            } else {
                DevBuf<T> dv, dcoef, dgrad, dw;
                dv.reserve(size_t(p)); dcoef.reserve(size_t(count) + 1); dgrad.reserve(size_t(p)); dw.reserve(size_t(p)); dcnt.reserve(1);
                const int32_t c32 = int32_t(count);
                AHIP_CHECK(hipMemcpyAsync(dv.p, v, size_t(p) * sizeof(T), hipMemcpyHostToDevice, s));
                if (count) AHIP_CHECK(hipMemcpyAsync(dcoef.p, coef, size_t(count) * sizeof(T), hipMemcpyHostToDevice, s));
                AHIP_CHECK(hipMemcpyAsync(dcnt.p, &c32, sizeof(int32_t), hipMemcpyHostToDevice, s));
                raw_cov_grad<T>(*A, dv.p, dlist.p, dcoef.p, dcnt.p, count, dgrad.p, dw.p, s);
                AHIP_CHECK(hipGetLastError());
                AHIP_CHECK(hipMemcpyAsync(out, dgrad.p, size_t(p) * sizeof(T), hipMemcpyDeviceToHost, s));
                AHIP_CHECK(hipStreamSynchronize(s));
            }
        };
        if (A->dtype == ADELIE_HIP_F64) body(double{});
        else body(float{});
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

} // extern "C"
