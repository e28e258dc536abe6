// cd_fit_body.hpp — the one-workgroup fit() shared by the box-constrained (kernels_bvls.hip) and the pinball
// (kernels_pinball.hip) coordinate descents, and its launch.  The host driver around it: cd_screen_driver.hpp.
//
// Both solvers of the reference (solver_bvls.hpp, solver_pinball.hpp) have the same fit(): screen-set passes that add the
// changed coordinates to the active set, active-set passes until convergence, a prune, the max-iterations exit and the
// counters.  They differ in the scalar update of a visit and in which active members a prune drops.  Those two come in as
// a `Rule`:
//     static T    Rule::update(vk, lk, uk, gk, bk)   the new coefficient (bit-equal to bk: the visit changes nothing)
//     static bool Rule::drop(b, lk, uk)              prune's predicate
// `lk` / `uk` are the coordinate's two per-coordinate constants (bounds for bvls, the penalties for pinball).
//
// The gradient g_a of EVERY screen coordinate is kept current through a resident matrix G (ns x ns, both triangles): a visit
// that changes beta_k by `del` does g_a -= G[a, k] * del for all a (one contiguous column), and a visit that changes nothing
// touches no memory but a few broadcast reads.
//
// Synchronisation.  Every thread evaluates the scalar update of a visit redundantly from broadcast reads, so no shuffle or
// reduction sits on the visit chain and all control flow is uniform.  g and beta are double-buffered: a changed visit reads
// buffer `cur`, writes ALL of g and beta to the other buffer and ends with the one barrier of the visit — a slow wavefront
// still reading g[k] / beta[k] of buffer `cur` cannot see the fast ones' stores.  Unchanged visits have no barrier and no
// store.  No atomics anywhere: reruns are bit-identical, and the LDS and the global-memory storage of the per-coordinate
// arrays run the same code and give the same bits.
//
// add_active: the reference appends a coordinate at the visit that changes it; here a screen pass raises a flag at that visit
// and the flagged non-members are appended, in screen order, at the end of the pass.  A screen pass visits in screen order, so
// the list is the same; it is complete before the pass's max-iterations exit is taken.
#pragma once
#include "common.hpp"

namespace ahip {
namespace {

constexpr int kCdFitThreads = 1024;
enum { CD_FIT_OK = 0, CD_FIT_MAX_ITERS = 1 };

// what a fit and the host exchange; `loss`, `iters` and `n_active` are read on entry and written on exit
struct CdFitRec {
    double loss;
    int64_t iters;
    int64_t n_visits_changed; // visits that changed a coefficient (this fit)
    int32_t status;
    int32_t n_active;
    int32_t n_changed;        // coordinates whose beta differs from its value at entry (= length of the compact list)
    int32_t pad;
};

// bytes of per-coordinate state: g x 2, beta x 2, lower, upper, vars; active list, membership flag, touched flag
template <class T>
constexpr size_t cd_fit_state_bytes(int64_t ns) {
    return size_t(ns) * (7 * sizeof(T) + 3 * sizeof(int32_t)) + 64;
}

template <class T>
struct CdFitArgs {
    const T* G;          // (ns, ns) column-major, leading dimension ld
    int64_t ld;
    int32_t ns;
    const int32_t* cols; // screen members' coordinates, screen order
    const int32_t* dcol_src; // what the compact list names a member by: dcol_src[k], or the position k itself when null
    const T* lower_s;    // screen order
    const T* upper_s;
    const T* vars_s;
    const T* g_s;        // gradient at entry
    T* beta_s;           // in: beta at entry; out: beta at exit
    int32_t* act;        // in / out: active set as positions in the screen set
    T* beta_full;        // out: beta_full[cols[a]] = beta at exit
    int32_t* dcol;       // out: compact list for launch_axpy_cols
    T* dlt;
    int32_t* cnt_dev;
    CdFitRec* rec;
    char* scratch;       // global storage of the per-coordinate state (the non-LDS form)
    int64_t max_iters;
    T tol_yvar;          // tol * y_var
};

// Appends to a list the positions k = src(i), i in [0, count_in) ascending, for which keep(i, k) holds, through emit(slot, k);
// returns the number appended (the same value in every thread).  The slots are handed out in ascending i: per trip a ballot
// gives the rank inside a wavefront and the wavefronts' counts go through `wcnt` (LDS, 16 ints).
template <class Src, class Keep, class Emit>
__device__ __forceinline__ int cd_compact(int count_in, int* wcnt, Src src, Keep keep, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (blockDim.x + 63) >> 6;
    int total = 0;
    for (int base = 0; base < count_in; base += blockDim.x) {
        const int i = base + tid;
        int k = 0;
        bool f = false;
        if (i < count_in) {
            k = src(i);
            f = keep(i, k);
        }
        const unsigned long long m = __ballot(f);
        const int within = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < nw; ++w) {
            const int c = wcnt[w];
            off += w < wave ? c : 0;
            tot += c;
        }
        if (f) emit(total + off + within, k);
        total += tot;
        __syncthreads();
    }
    return total;
}

template <class T, bool LDS, class Rule>
__global__ __launch_bounds__(kCdFitThreads) void cd_fit_kernel(CdFitArgs<T> A) {
    extern __shared__ __attribute__((aligned(16))) char cd_fit_sm[];
    __shared__ int wcnt[kCdFitThreads / 64];
    const int tid = threadIdx.x, bd = blockDim.x, ns = A.ns;
    // no __restrict__ on the state: the same arrays are read and written across barriers
    char* base = LDS ? cd_fit_sm : A.scratch;
    T* g0 = reinterpret_cast<T*>(base);
    T* g1 = g0 + ns;
    T* b0 = g1 + ns;
    T* b1 = b0 + ns;
    T* lo = b1 + ns;
    T* up = lo + ns;
    T* var = up + ns;
    int32_t* act = reinterpret_cast<int32_t*>(var + ns);
    int32_t* isact = act + ns;
    int32_t* touched = isact + ns;

    int nact = A.rec->n_active;
    for (int a = tid; a < ns; a += bd) {
        g0[a] = A.g_s[a];
        b0[a] = A.beta_s[a];
        lo[a] = A.lower_s[a];
        up[a] = A.upper_s[a];
        var[a] = A.vars_s[a];
        isact[a] = 0;
        touched[a] = 0;
    }
    __syncthreads();
    for (int i = tid; i < nact; i += bd) {
        const int k = A.act[i];
        act[i] = k;
        isact[k] = 1;
    }
    __syncthreads();

    T loss = T(A.rec->loss);
    int64_t iters = A.rec->iters;
    int64_t nvis = 0;
    const int64_t max_iters = A.max_iters;
    const T tol_yvar = A.tol_yvar;
    int cur = 0, status = CD_FIT_OK;
    T convg = T(0);

    // coordinate_descent's body for position k; SCREEN: raise the touched flag (add_active)
    auto visit = [&](int k, bool screen) {
#pragma clang fp contract(off)
        const T* gc = cur ? g1 : g0;
        const T* bc = cur ? b1 : b0;
        const T vk = var[k], lk = lo[k], uk = up[k], gk = gc[k], bk = bc[k];
        const T bn = Rule::update(vk, lk, uk, gk, bk);
        if (bn == bk) return;
        const T del = bn - bk;
        const T sds = vk * del * del;
        convg = (convg < sds) ? sds : convg;
        loss -= del * gk - T(0.5) * sds;
        T* gn = cur ? g0 : g1;
        T* bx = cur ? b0 : b1;
        const T* Gk = A.G + int64_t(k) * A.ld;
        for (int a = tid; a < ns; a += bd) {
            gn[a] = gc[a] - Gk[a] * del;
            bx[a] = a == k ? bn : bc[a];
        }
        if (screen && tid == 0) touched[k] = 1;
        ++nvis;
        cur ^= 1;
        __syncthreads();
    };
    auto prune = [&]() { // in place: a kept member moves to a slot at or before its own
        const T* bc = cur ? b1 : b0;
        nact = cd_compact(
            nact, wcnt, [&](int i) { return act[i]; },
            [&](int, int k) {
                const bool drop = Rule::drop(bc[k], lo[k], up[k]);
                if (drop) isact[k] = 0;
                return !drop;
            },
            [&](int slot, int k) { act[slot] = k; });
    };

    while (true) { // fit()
        ++iters;
        convg = T(0);
        for (int k = 0; k < ns; ++k) visit(k, true);
        {   // the pass's add_active calls, in screen order
            const int base_n = nact;
            nact += cd_compact(
                ns, wcnt, [&](int i) { return i; }, [&](int, int k) { return touched[k] != 0 && isact[k] == 0; },
                [&](int slot, int k) { act[base_n + slot] = k; });
            for (int a = tid; a < ns; a += bd) {
                if (touched[a]) isact[a] = 1;
                touched[a] = 0;
            }
            __syncthreads();
        }
        if (iters >= max_iters) {
            status = CD_FIT_MAX_ITERS;
            break;
        }
        if (convg <= tol_yvar) {
            prune();
            break;
        }
        bool stop = false;
        while (true) { // solve_active()
            ++iters;
            convg = T(0);
            for (int i = 0; i < nact; ++i) visit(act[i], false);
            if (iters >= max_iters) {
                status = CD_FIT_MAX_ITERS;
                stop = true;
                break;
            }
            if (convg <= tol_yvar) break;
        }
        if (stop) break;
        prune();
    }

    // exit: the compact (member, change) list, beta, the active set, the report
    const T* bc = cur ? b1 : b0;
    const int nchg = cd_compact(
        ns, wcnt, [&](int i) { return i; }, [&](int, int k) { return bc[k] != A.beta_s[k]; },
        [&](int slot, int k) {
            A.dcol[slot] = A.dcol_src ? A.dcol_src[k] : k;
            A.dlt[slot] = bc[k] - A.beta_s[k];
        });
    // (cd_compact ends with a barrier: every read of beta at entry is done)
    for (int a = tid; a < ns; a += bd) {
        const T b = bc[a];
        A.beta_s[a] = b;
        A.beta_full[A.cols[a]] = b;
    }
    for (int i = tid; i < nact; i += bd) A.act[i] = act[i];
    if (tid == 0) {
        A.rec->loss = double(loss);
        A.rec->iters = iters;
        A.rec->n_visits_changed = nvis;
        A.rec->status = status;
        A.rec->n_active = nact;
        A.rec->n_changed = nchg;
        A.cnt_dev[0] = nchg;
    }
}

// launches one fit on `s`: the state in dynamic LDS when it fits there (and `lds_max_ns` allows it), else in `scratch`
template <class T, class Rule>
void launch_cd_fit(CdFitArgs<T> fa, int lds_limit, int64_t lds_max_ns, DevBuf<char>& scratch, bool& attr_done, hipStream_t s) {
    const int64_t ns = fa.ns;
    const size_t bytes = cd_fit_state_bytes<T>(ns);
    // the static LDS of the kernel (the wavefront counts) comes out of the same budget
    const bool lds = bytes + 256 <= size_t(lds_limit) && (lds_max_ns <= 0 || ns <= lds_max_ns);
    fa.scratch = lds ? nullptr : scratch.reserve(bytes);
    const unsigned threads = unsigned(std::min<int64_t>(kCdFitThreads, std::max<int64_t>(64, (ns + 63) / 64 * 64)));
    if (lds) {
        if (!attr_done) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_fit_kernel<T, true, Rule>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds_limit);
            (void)hipGetLastError();
            attr_done = true;
        }
        hipLaunchKernelGGL((cd_fit_kernel<T, true, Rule>), dim3(1), dim3(threads), bytes, s, fa);
    } else {
        hipLaunchKernelGGL((cd_fit_kernel<T, false, Rule>), dim3(1), dim3(threads), 0, s, fa);
    }
}

} // namespace
} // namespace ahip
