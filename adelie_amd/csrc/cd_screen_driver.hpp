// cd_screen_driver.hpp — the host driver shared by the coordinate descents over a growing screen set (kernels_bvls.hip,
// kernels_pinball.hip): the screen-order buffers, the resident ns x ns matrix, fit() around the shared kernel
// (cd_fit_body.hpp), the warm start, the KKT loop of solve() and the result the C accessors read.
//
// A solver derives from CdScreenDriver<T, Self, Args> and supplies what truly differs:
//     kName, Rule, gram_limit_mb(), lds_max_ns()         its name in messages, its fit rule, its two config globals
//     upload()                                           its full vectors onto the device (d_r and d_beta among them)
//     sweep(cols, ncols, out)                            the gradient of the listed coordinates (all of them when cols is null)
//     viols()                                            d_viols from d_grad
//     extend(ns_old, ns_new)                             rows and columns [ns_old, ns_new) of G
//     gather(a0, src, by_col)                            the screen-order copies for the fit kernel
//     dcol_src(), catch_up()                             what the compact list names a member by; resid -= (design) * delta
//     grow_extra(c, keep), finish_downloads(es), finish_extras()   optional: its own screen-order storage and results
// Everything enqueued on the stream, and every synchronisation, is in the order the two solvers had on their own.
#pragma once
#include <cmath>
#include <string>

#include "common.hpp"
#include "cd_fit_body.hpp"
#include "cd_screen_host.hpp"

namespace ahip {

// what a solve leaves behind; `n` rows and `p` coordinates (bvls: X is (n, p); pinball: A is (p, n) = (m, d))
struct CdScreenResult {
    int dtype = ADELIE_HIP_F64, device = 0;
    int64_t n = 0, p = 0;
    std::vector<char> beta, resid, grad; // of dtype
    std::vector<int64_t> screen_set, active_set;
    std::vector<uint8_t> is_screen, is_active;
    double loss = 0;
    int64_t iters = 0, n_kkt = 0, n_changed = 0;
    double total_time = 0, t_sweep_ms = 0, t_gram_ms = 0, t_fit_ms = 0;
    std::string error;
    virtual ~CdScreenResult() = default;
    // a solver's own vectors: the length (-1: not one of them) and the copy of the first m elements
    virtual int64_t extra_size(int) const { return -1; }
    virtual void extra_copy(int, void*, size_t, size_t) const {}
};
// the vectors and scalars both solvers have, by the values of their enums in adelie_hip.h (static_asserts in the two files)
enum { CDS_BETA = 0, CDS_RESID, CDS_GRAD, CDS_SCREEN_SET, CDS_ACTIVE_SET, CDS_IS_SCREEN, CDS_IS_ACTIVE };
enum { CDS_LOSS = 0, CDS_ITERS, CDS_N_KKT, CDS_SCREEN_SET_SIZE, CDS_ACTIVE_SET_SIZE, CDS_TOTAL_TIME, CDS_T_SWEEP_MS, CDS_T_GRAM_MS,
       CDS_T_FIT_MS, CDS_N_CHANGED };

// the bodies of the C accessors
inline int64_t cd_result_size(const CdScreenResult* r, int which) {
    if (!r) return -1;
    switch (which) {
        case CDS_BETA:
        case CDS_GRAD:
        case CDS_IS_SCREEN:
        case CDS_IS_ACTIVE: return r->p;
        case CDS_RESID: return r->n;
        case CDS_SCREEN_SET: return int64_t(r->screen_set.size());
        case CDS_ACTIVE_SET: return int64_t(r->active_set.size());
    }
    return r->extra_size(which);
}
inline int cd_result_copy(const CdScreenResult* r, int which, void* out, int64_t cap) {
    ABI_TRY
    const int64_t size = cd_result_size(r, which);
    if (size < 0 || !out) throw make_core_error("unknown result vector.");
    const size_t m = size_t(std::min(size, cap));
    const size_t es = r->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
    if (!m) return 0;
    switch (which) {
        case CDS_BETA: std::memcpy(out, r->beta.data(), m * es); break;
        case CDS_RESID: std::memcpy(out, r->resid.data(), m * es); break;
        case CDS_GRAD: std::memcpy(out, r->grad.data(), m * es); break;
        case CDS_SCREEN_SET: std::memcpy(out, r->screen_set.data(), m * sizeof(int64_t)); break;
        case CDS_ACTIVE_SET: std::memcpy(out, r->active_set.data(), m * sizeof(int64_t)); break;
        case CDS_IS_SCREEN: std::memcpy(out, r->is_screen.data(), m); break;
        case CDS_IS_ACTIVE: std::memcpy(out, r->is_active.data(), m); break;
        default: r->extra_copy(which, out, m, es);
    }
    ABI_CATCH
}
inline double cd_result_scalar(const CdScreenResult* r, int which) {
    if (!r) return 0;
    switch (which) {
        case CDS_LOSS: return r->loss;
        case CDS_ITERS: return double(r->iters);
        case CDS_N_KKT: return double(r->n_kkt);
        case CDS_SCREEN_SET_SIZE: return double(r->screen_set.size());
        case CDS_ACTIVE_SET_SIZE: return double(r->active_set.size());
        case CDS_TOTAL_TIME: return r->total_time;
        case CDS_T_SWEEP_MS: return r->t_sweep_ms;
        case CDS_T_GRAM_MS: return r->t_gram_ms;
        case CDS_T_FIT_MS: return r->t_fit_ms;
        case CDS_N_CHANGED: return double(r->n_changed);
    }
    return 0;
}

namespace {

struct Pinned {
    void* p = nullptr;
    size_t bytes = 0;
    explicit Pinned(size_t n) : bytes((n + 4095) / 4096 * 4096) {
        p = HostPool::take(bytes, hipHostMallocDefault);
        if (!p) throw core_error("adelie_hip: hipHostMalloc failed");
    }
    ~Pinned() { HostPool::give(p, bytes, hipHostMallocDefault); }
};

// HIP-event time of the three device phases; collected after a stream synchronisation
struct PhaseTimer {
    struct Span { hipEvent_t a, b; int cat; };
    std::vector<Span> open;
    std::vector<hipEvent_t> idle;
    double ms[3] = {0, 0, 0};
    hipEvent_t get() {
        if (!idle.empty()) {
            hipEvent_t e = idle.back();
            idle.pop_back();
            return e;
        }
        hipEvent_t e;
        AHIP_CHECK(hipEventCreate(&e));
        return e;
    }
    void begin(int cat, hipStream_t s) {
        Span sp{get(), get(), cat};
        AHIP_CHECK(hipEventRecord(sp.a, s));
        open.push_back(sp);
    }
    void end(hipStream_t s) { AHIP_CHECK(hipEventRecord(open.back().b, s)); }
    void collect() { // (the stream is idle)
        for (const Span& sp : open) {
            float t = 0;
            if (hipEventElapsedTime(&t, sp.a, sp.b) == hipSuccess) ms[sp.cat] += double(t);
            else (void)hipGetLastError();
            idle.push_back(sp.a);
            idle.push_back(sp.b);
        }
        open.clear();
    }
    ~PhaseTimer() {
        for (const Span& sp : open) idle.push_back(sp.a), idle.push_back(sp.b);
        for (hipEvent_t e : idle) (void)hipEventDestroy(e);
    }
};
enum { PH_SWEEP = 0, PH_GRAM = 1, PH_FIT = 2 };

inline unsigned cd_blocks_for(int64_t n, int per) { return unsigned((n + per - 1) / per); }

template <class T, class Self, class Args>
struct CdScreenDriver {
    adelie_hip_design* X;
    CdScreenResult* res;
    const Args* a;
    int64_t n, p; // rows and coordinates of the handle
    hipStream_t s;
    DenseView<T> Xv;
    DeferredFrees deferred;
    PhaseTimer timer;

    // full vectors
    DevBuf<T> d_r, d_grad, d_viols, d_beta;
    // screen order
    DevBuf<int32_t> d_cols, d_act, d_dcol, d_cnt;
    DevBuf<T> d_g, d_lower_s, d_upper_s, d_vars_s, d_beta_s, d_dlt, d_sweep_out;
    DevBuf<T> d_G, d_work_sweep;
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

    CdScreenDriver(adelie_hip_design* X_, const Args* a_, CdScreenResult* r) : X(X_), res(r), a(a_) {
        n = X->n;
        p = X->p;
        s = X->stream;
        Xv = X->dense<T>();
        loss = T(a->loss);
    }
    Self& self() { return static_cast<Self&>(*this); }
    void grow_extra(size_t, size_t) {}
    void finish_downloads(size_t) {}
    void finish_extras() {}

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
        self().grow_extra(c, size_t(keep));
        d_g.reserve(c), d_dcol.reserve(c), d_dlt.reserve(c), d_sweep_out.reserve(c);
        cap_s = c;
    }
    // G for ns_new members: false when it would pass the limit
    bool reserve_gram(int64_t ns_new, int64_t ns_old) {
        const double limit = Self::gram_limit_mb() * 1048576.0;
        if (double(ns_new) * double(ns_new) * double(sizeof(T)) > limit) return false;
        if (ns_new <= ld) return true;
        int64_t nl = std::max<int64_t>(std::max<int64_t>(ns_new, ld + ld / 2), 64);
        nl = std::min<int64_t>(nl, std::max<int64_t>(p, ns_new));
        if (double(nl) * double(nl) * double(sizeof(T)) > limit) nl = ns_new;
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

    void fit(CdFitRec* h_rec) {
        CdFitArgs<T> fa;
        fa.G = d_G.p, fa.ld = ld, fa.ns = int32_t(ns), fa.cols = d_cols.p;
        fa.dcol_src = self().dcol_src();
        fa.lower_s = d_lower_s.p, fa.upper_s = d_upper_s.p, fa.vars_s = d_vars_s.p, fa.g_s = d_g.p, fa.beta_s = d_beta_s.p;
        fa.act = d_act.p, fa.beta_full = d_beta.p, fa.dcol = d_dcol.p, fa.dlt = d_dlt.p, fa.cnt_dev = d_cnt.p, fa.rec = d_rec.p;
        fa.scratch = nullptr;
        fa.max_iters = a->max_iters;
        fa.tol_yvar = T(a->tol) * T(a->y_var);
        h_rec->loss = double(loss), h_rec->iters = iters, h_rec->n_visits_changed = 0, h_rec->status = 0;
        h_rec->n_active = int32_t(nact), h_rec->n_changed = 0, h_rec->pad = 0;
        AHIP_CHECK(hipMemcpyAsync(d_rec.p, h_rec, sizeof(CdFitRec), hipMemcpyHostToDevice, s));
        timer.begin(PH_FIT, s);
        launch_cd_fit<T, typename Self::Rule>(fa, lds_limit, Self::lds_max_ns(), d_scratch, attr_done, s);
        timer.end(s);
        self().catch_up();
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
        res->beta.resize(size_t(p) * es), res->resid.resize(size_t(n) * es), res->grad.resize(size_t(p) * es);
        if (p) AHIP_CHECK(hipMemcpyAsync(res->beta.data(), d_beta.p, size_t(p) * es, hipMemcpyDeviceToHost, s));
        if (n) AHIP_CHECK(hipMemcpyAsync(res->resid.data(), d_r.p, size_t(n) * es, hipMemcpyDeviceToHost, s));
        self().finish_downloads(es);
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
        self().finish_extras();
        res->loss = double(loss);
        res->iters = iters;
        res->n_kkt = n_kkt;
        res->t_sweep_ms = timer.ms[PH_SWEEP], res->t_gram_ms = timer.ms[PH_GRAM], res->t_fit_ms = timer.ms[PH_FIT];
    }
    void error_exit(const std::string& what) {
        res->error = std::string("adelie_core solver: ") + Self::kName + ": " + what;
        finish();
    }
    void gram_limit_error(int64_t ns_want) {
        error_exit("screen set of " + std::to_string(ns_want) + " coordinates exceeds the device Gram limit");
    }

    void run() {
        DeferredFrees::Scope scope(&deferred);
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, X->device) != hipSuccess || v <= 0) {
            (void)hipGetLastError();
            v = 65536;
        }
        lds_limit = v;
        d_r.reserve(size_t(n)), d_grad.reserve(size_t(p)), d_viols.reserve(size_t(p)), d_beta.reserve(size_t(p));
        d_cnt.reserve(4), d_rec.reserve(1);
        self().upload();
        h_viols.resize(size_t(p));
        is_screen.assign(size_t(p), 0);
        Pinned pin(sizeof(CdFitRec));
        CdFitRec* h_rec = static_cast<CdFitRec*>(pin.p);

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
            self().extend(0, ns);
            self().sweep(d_cols.p, ns, d_sweep_out.p);
            self().gather(0, d_sweep_out.p, false);
            AHIP_CHECK(hipStreamSynchronize(s));
        }

        while (true) { // the reference's solve()
            const T loss_prev = loss;
            if (ns > 0) {
                fit(h_rec);
                if (h_rec->status == CD_FIT_MAX_ITERS) return error_exit("max iterations reached!");
            } else { // an empty screen pass
                ++iters;
                if (iters >= a->max_iters) return error_exit("max iterations reached!");
            }
            if (n_kkt > 0 && double(std::abs(loss - loss_prev)) < 1e-6 * double(std::abs(T(a->y_var)))) return finish();
            // kkt_screen()
            ++n_kkt;
            self().sweep(nullptr, p, d_grad.p);
            self().viols();
            AHIP_CHECK(hipMemcpyAsync(h_viols.data(), d_viols.p, size_t(p) * sizeof(T), hipMemcpyDeviceToHost, s));
            AHIP_CHECK(hipStreamSynchronize(s));
            AHIP_CHECK(hipGetLastError());
            timer.collect();
            have_viols = true;
            std::vector<int64_t> added;
            if (cd_screen_admit(h_viols.data(), p, is_screen.data(), a->kappa, added)) return finish();
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
            self().extend(ns_old, ns_new);
            self().gather(ns_old, d_grad.p, true);
            AHIP_CHECK(hipStreamSynchronize(s)); // (h_cols is read by the copy)
        }
    }
};

// the C entry point's body: `checks` holds the solver's own argument checks (they throw), the warm-start validation included
template <template <class> class Solver, class Result, class Args, class Checks>
int cd_screen_solve(adelie_hip_design* X, const Args* a, Result** out, Checks checks) {
    Result* res = nullptr;
    try {
        if (!X || !a || !out) throw make_core_error("null argument.");
        checks();
        AHIP_CHECK(hipSetDevice(X->device));
        res = new Result;
        res->dtype = X->dtype;
        res->device = X->device;
        res->n = X->n;
        res->p = X->p;
        const auto t0 = std::chrono::steady_clock::now();
        auto run = [&](auto&& sv) {
            try {
                sv.run();
            } catch (...) {
                (void)hipStreamSynchronize(X->stream); // the buffers are parked by the destructors
                throw;
            }
        };
        DTYPE_DISPATCH(X, run(Solver<T>(X, a, res)))
        res->total_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *out = res;
    } catch (const std::exception& e) {
        delete res;
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

} // namespace
} // namespace ahip
