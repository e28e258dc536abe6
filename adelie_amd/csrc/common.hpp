// common.hpp — host-side helpers shared by the C-ABI translation units.
#pragma once
#include <cstdlib>
#include <algorithm>
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/adelie_hip.h"
#include "kernels.hpp"
#include "dev_array_host.hpp"

namespace ahip {

// ---- every environment hook of libadelie_hip.so, in one place ------------------------------------------------------------------
// Fifteen variables.  They are read when a solve starts (Hooks::from_env, one call per solve): the tests force the multi-CU engines
// at sizes the CPU checker finishes in seconds and compare variants between two solves of ONE process, so reading them once at
// library load would freeze the first test's setting.  None changes results beyond rounding.  (Python side: ADELIE_HIP_LIB picks
// another build of this library, ADELIE_HIP_SWEEP_BATCH=0 keeps concurrent CV folds from sharing their sweeps.)
//   ADELIE_HIP_CD_BLOCK_MIN_NV=n  screen sets of at least n coefficients use the panel engine (default 128)       [test hook]
//   ADELIE_HIP_PANEL_BSZ=32|64|128  visits per lasso panel block (default 128, 64 under IRLS)                      [test hook]
//   ADELIE_HIP_LOOKAHEAD=0        Gaussian passes in the sequential form (step -> reduce -> solve) that IRLS and
//                                 constrained problems always use                                                   [test hook]
//   ADELIE_HIP_SPECULATE=0        no speculative first active-set pass behind the invariance sweep                  [A/B, bit-identity test]
//   ADELIE_HIP_IRLS_REUSE=theta   IRLS diagonal-block / Gram reuse threshold (default 0.1, 0 = rebuild per iteration) [documented deviation]
//   ADELIE_HIP_CONS_HOST=1        box / one-sided constraint objects visited on the host instead of kernels_cons.hip  [A/B, tests]
//   ADELIE_HIP_SPARSE_PANEL=0     IRLS on a design kept sparse on the full-Gram engines instead of the panel engine    [A/B, tests]
//   ADELIE_HIP_STD_PANEL=0        standardized dense / 2-bit views on their full-Gram engines instead of the panel engines [A/B, tests]
//   ADELIE_HIP_FACTOR_SWEEP=0|1   full sweeps of a one-hot / interaction design read off Z (kernels_factor.hip) or off the
//                                 expanded matrix like any dense design (default: kFactorSweepDefault below; the matrix
//                                 operations read it at the call)                                                     [A/B, tests]
//   ADELIE_HIP_RELU_SWEEP=0|1     full sweeps of a convex-relu design as the matrix product Z^T (mask o v) (kernels_relu.hip) or off
//                                 the expanded matrix like any dense design (default: kReluSweepDefault below; the matrix
//                                 operations read it at the call); on a convex-relu design kept sparse, off Z's compressed
//                                 columns and the packed mask (kernels_relu_sparse.hip) or off the expansion's compressed
//                                 columns (default: kReluSparseSweepDefault)                                          [A/B, tests]
//   ADELIE_HIP_FILTER_SWEEP=0|1   the invariance sweep of an eligible Gaussian lambda through the float32 shadow of the design
//                                 (kernels_filter.hip) or as the full f64 sweep; same results bit for bit             [A/B, tests]
//   ADELIE_HIP_FILTER_DEPTH=0|1   the pivot rule's threshold of a filtered sweep at the depth screen() is predicted to read
//                                 (screen_reads_host.hpp) or at twice the worst case `need`; same results bit for bit [A/B, tests]
//   ADELIE_HIP_FILTER_DEPTH_MARGIN=m  the margin of that depth over the prediction; 0 leaves none, so that threshold passes
//                                 fall short and take the full sweep after all                                        [test hook]
//   ADELIE_HIP_SHADOW_KIND=f32|q15|auto  the encoding of that shadow copy, read when a design's copy is made: float32, int16
//                                 with one scale per column, or (default) the rule of shadow_kind_host.hpp           [A/B, tests]
//   ADELIE_HIP_SHADOW_MIN_BYTES=b `auto` considers q15 when the float32 copy would hold at least b bytes (default 2^30)  [test hook]
//   ADELIE_HIP_TIME_PANEL=1       per-launch HIP events around the panel step (bench.py's roofline leg)
//   ADELIE_HIP_TRACE=1|2          1: per-pass trace on stderr; 2: + enqueue / allocation / build timings
struct Hooks {
    long long cd_block_min_nv = -1; // -1: unset
    int panel_bsz = 0;
    int sparse_panel = -1;   // ADELIE_HIP_SPARSE_PANEL=0: IRLS on a design kept sparse stays on the full-Gram engines
    int std_panel = -1;      // ADELIE_HIP_STD_PANEL=0: a standardized dense / 2-bit view stays on its full-Gram engines
    int lookahead = -1, speculate = -1;
    int factor_sweep = -1;   // ADELIE_HIP_FACTOR_SWEEP (-1: unset)
    int relu_sweep = -1;     // ADELIE_HIP_RELU_SWEEP (-1: unset)
    int filter_sweep = -1;   // ADELIE_HIP_FILTER_SWEEP (-1: unset)
    int filter_depth = -1;   // ADELIE_HIP_FILTER_DEPTH (-1: unset)
    double filter_depth_margin = -1; // ADELIE_HIP_FILTER_DEPTH_MARGIN (< 0: unset)
    double irls_reuse = -1;
    bool time_panel = false;
    bool cons_host = false; // ADELIE_HIP_CONS_HOST=1: box / one-sided objects on several coefficients visited on the host (A/B, tests)
    int trace = 0;
    static Hooks from_env() {
        Hooks h;
        if (const char* e = std::getenv("ADELIE_HIP_CD_BLOCK_MIN_NV")) h.cd_block_min_nv = std::atoll(e);
        if (const char* e = std::getenv("ADELIE_HIP_PANEL_BSZ")) {
            const int v = std::atoi(e);
            h.panel_bsz = (v == 32 || v == 64 || v == 128) ? v : 0;
        }
        if (const char* e = std::getenv("ADELIE_HIP_LOOKAHEAD")) h.lookahead = std::atoi(e) != 0;
        if (const char* e = std::getenv("ADELIE_HIP_SPECULATE")) h.speculate = std::atoi(e) != 0;
        if (const char* e = std::getenv("ADELIE_HIP_IRLS_REUSE")) h.irls_reuse = std::max(0.0, std::atof(e));
        h.time_panel = std::getenv("ADELIE_HIP_TIME_PANEL") != nullptr;
        if (const char* e = std::getenv("ADELIE_HIP_CONS_HOST")) h.cons_host = std::atoi(e) != 0;
        if (const char* e = std::getenv("ADELIE_HIP_SPARSE_PANEL")) h.sparse_panel = std::atoi(e) != 0;
        if (const char* e = std::getenv("ADELIE_HIP_STD_PANEL")) h.std_panel = std::atoi(e) != 0;
        if (const char* e = std::getenv("ADELIE_HIP_TRACE")) h.trace = std::max(1, std::atoi(e));
        h.factor_sweep = factor_sweep_env();
        h.relu_sweep = relu_sweep_env();
        h.filter_sweep = filter_sweep_env();
        if (const char* e = std::getenv("ADELIE_HIP_FILTER_DEPTH")) h.filter_depth = std::atoi(e) != 0;
        if (const char* e = std::getenv("ADELIE_HIP_FILTER_DEPTH_MARGIN")) h.filter_depth_margin = std::max(0.0, std::atof(e));
        return h;
    }
    static int filter_sweep_env() {
        const char* e = std::getenv("ADELIE_HIP_FILTER_SWEEP");
        return e ? int(std::atoi(e) != 0) : -1;
    }
    static int shadow_kind_env() { return shadow_kind_parse(std::getenv("ADELIE_HIP_SHADOW_KIND")); }
    static int64_t shadow_min_bytes_env() {
        const char* e = std::getenv("ADELIE_HIP_SHADOW_MIN_BYTES");
        return e ? int64_t(std::atoll(e)) : kShadowMinBytesDefault;
    }
    static int factor_sweep_env() {
        const char* e = std::getenv("ADELIE_HIP_FACTOR_SWEEP");
        return e ? int(std::atoi(e) != 0) : -1;
    }
    static int relu_sweep_env() {
        const char* e = std::getenv("ADELIE_HIP_RELU_SWEEP");
        return e ? int(std::atoi(e) != 0) : -1;
    }
};
// The hooks that choose a structured full sweep, one per structured kind of design (design_ops.hpp: raw_sweep_structured).  A
// solve passes what it read when it started, the matrix operations read them at the call.
struct SweepHooks {
    int factor = -1, relu = -1;
    static SweepHooks from_env() { return SweepHooks{Hooks::factor_sweep_env(), Hooks::relu_sweep_env()}; }
};
// Whether the full sweeps of a factor design take the structured kernel when ADELIE_HIP_FACTOR_SWEEP is unset: only once it is
// measured at least as fast as the dense sweep on both shapes of scripts/bench_factor.py (profiles/factor_sweep.txt).
constexpr bool kFactorSweepDefault = false;
inline bool factor_sweep_on(int hook) { return hook < 0 ? kFactorSweepDefault : hook != 0; }
// The same rule for a convex-relu design and ADELIE_HIP_RELU_SWEEP, on both shapes of scripts/bench_relu.py.  On: measured
// faster than the dense sweep on both (profiles/relu_sweep.txt).
constexpr bool kReluSweepDefault = true;
inline bool relu_sweep_on(int hook) { return hook < 0 ? kReluSweepDefault : hook != 0; }
// The same hook on a convex-relu design kept sparse (kernels_relu_sparse.hip), by the same rule on both shapes of
// scripts/bench_relu_sparse.py against the compressed-column sweep of the expansion (profiles/relu_sparse_sweep.txt).
// On: measured faster on both, far beyond the spread.
constexpr bool kReluSparseSweepDefault = true;
inline bool relu_sparse_sweep_on(int hook) { return hook < 0 ? kReluSparseSweepDefault : hook != 0; }
// Whether an eligible Gaussian lambda takes the filtered invariance sweep (float32 shadow, kernels_filter.hip) when
// ADELIE_HIP_FILTER_SWEEP is unset.  On: the headline gains 16 ms of 252 ms per path against a parent-to-hook-off spread of
// 0.3 ms in one interleaved job, with identical outputs (profiles/filter_sweep.txt).
constexpr bool kFilterSweepDefault = true;
inline bool filter_sweep_on(int hook) { return hook < 0 ? kFilterSweepDefault : hook != 0; }
// The same for ADELIE_HIP_FILTER_DEPTH (profiles/filter_depth.txt).
constexpr bool kFilterDepthDefault = true;
inline bool filter_depth_on(int hook) { return hook < 0 ? kFilterDepthDefault : hook != 0; }


// (core_error itself: dev_array_host.hpp)
inline core_error make_core_error(const std::string& m) { return core_error("adelie_core: " + m); }
inline core_error make_solver_error(const std::string& m) { return core_error("adelie_core solver: " + m); }

#define AHIP_CHECK(expr)                                                                                   \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess)                                                                              \
            throw ::ahip::core_error(std::string("adelie_hip: HIP error '") + hipGetErrorString(_e) +     \
                                     "' at " #expr);                                                       \
    } while (0)

// ---- the frame of a C-ABI entry ------------------------------------------------------------------------------------------------
// ABI_TRY ... ABI_CATCH around an entry's body: an exception's message becomes adelie_hip_last_error() (thread-local, design.hip)
// and the entry returns 1; otherwise it returns 0.  A handler that does more (frees a result, waits for a stream) is written out.
void set_last_error(const std::string& s);
#define ABI_TRY try {
#define ABI_CATCH                         \
    }                                     \
    catch (const std::exception& e) {     \
        ::ahip::set_last_error(e.what()); \
        return 1;                         \
    }                                     \
    return 0;
// runs the statement(s) once with T = the value type of `d` (a design, or an argument block with a dtype)
#define DTYPE_DISPATCH(d, ...)                                                            \
    if ((d)->dtype == ADELIE_HIP_F64) { using T = double; (void)sizeof(T); __VA_ARGS__; } \
    else { using T = float; (void)sizeof(T); __VA_ARGS__; }

// wall-clock spent in hipMalloc / hipFree by the DevBufs of this process (tuning aid, printed under ADELIE_HIP_TRACE_ENQ)
struct DevAllocStats {
    static double& seconds() { static double s = 0; return s; }
    static long& calls() { static long c = 0; return c; }
};

// Process-wide caches of what a solve would otherwise create and destroy every time: pinned host blocks (the staging arena,
// the host-mapped pass report: hipHostMalloc / hipHostFree pin and unpin pages, ~1 ms for the 8 MB arena) and non-blocking
// streams.  Same contract as DevPool below: an owner hands a block / stream back only after it synchronised what used it.
struct HostPool {
    struct Entry { size_t bytes; unsigned flags; void* p; };
    static std::mutex& mu() { static std::mutex* m = new std::mutex; return *m; }
    static std::vector<Entry>& parked() { static auto* v = new std::vector<Entry>; return *v; }
    static void* take(size_t bytes, unsigned flags) {
        {
            std::lock_guard<std::mutex> lk(mu());
            auto& v = parked();
            for (size_t i = 0; i < v.size(); ++i)
                if (v[i].bytes == bytes && v[i].flags == flags) {
                    void* p = v[i].p;
                    v[i] = v.back();
                    v.pop_back();
                    return p;
                }
        }
        void* hp = nullptr;
        if (hipHostMalloc(&hp, bytes, flags) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return hp;
    }
    static void give(void* p, size_t bytes, unsigned flags) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> lk(mu());
            if (parked().size() < 64) {
                parked().push_back(Entry{bytes, flags, p});
                return;
            }
        }
        (void)hipHostFree(p);
    }
};
struct StreamPool {
    struct Entry { int dev; hipStream_t s; };
    static std::mutex& mu() { static std::mutex* m = new std::mutex; return *m; }
    static std::vector<Entry>& parked() { static auto* v = new std::vector<Entry>; return *v; }
    static hipStream_t take() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) throw core_error("adelie_hip: hipGetDevice failed");
        {
            std::lock_guard<std::mutex> lk(mu());
            auto& v = parked();
            for (size_t i = 0; i < v.size(); ++i)
                if (v[i].dev == dev) {
                    hipStream_t s = v[i].s;
                    v[i] = v.back();
                    v.pop_back();
                    return s;
                }
        }
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
            throw core_error("adelie_hip: hipStreamCreateWithFlags failed");
        return s;
    }
    // `s` is idle (the owner synchronised it)
    static void give(hipStream_t s) {
        if (!s) return;
        int dev = 0;
        hipDevice_t sd;
        // the stream's own device (see DevPool::give); older runtimes without the query fall back to the current device
        const bool known = hipStreamGetDevice(s, &sd) == hipSuccess ? (dev = int(sd), true) : (hipGetDevice(&dev) == hipSuccess);
        if (known) {
            std::lock_guard<std::mutex> lk(mu());
            if (parked().size() < 64) {
                parked().push_back(Entry{dev, s});
                return;
            }
        }
        (void)hipStreamDestroy(s);
    }
};

// Pinned staging arena for the many small host<->device copies of a path (screen-set appends, per-fit scalars, coefficient
// downloads: ~15 per lambda).  hipMemcpyAsync on pageable host memory costs the calling thread ~20 us per copy on this
// platform (staging + an internal wait); from / to pinned memory it is an enqueue.  A solve installs its arena for the
// calling thread (Staging::Scope) and DevBuf::upload / download on the arena's stream go through it: uploads snapshot the
// host data into a slot, downloads land in a slot and reach their destination at the next Staging::flush() — which the
// owner calls after every host wait that covers the staged copies (stream synchronisation, or an event recorded behind
// them).  Slots are recycled after a full stream synchronisation (reset()) or up to a mark whose event was waited for (release()).  When the arena is exhausted the
// copies fall back to the pageable path (correct, slower).
struct Staging {
    char* base = nullptr;
    size_t cap = 0, head = 0, tail = 0; // ring: slots live in [tail, head) (modulo cap); head == tail: empty
    hipStream_t stream = nullptr;
    struct Pend { void* dst; const void* src; size_t bytes; };
    std::vector<Pend> pend;
    size_t n_fallback = 0; // copies on this arena's stream that did not fit and went the pageable way
    Staging() = default;
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging() { HostPool::give(base, cap, hipHostMallocDefault); } // (the owner synchronised its stream)
    void init(size_t bytes, hipStream_t s) {
        stream = s;
        if (base) return;
        if (void* hp = HostPool::take(bytes, hipHostMallocDefault)) {
            base = static_cast<char*>(hp);
            cap = bytes;
        }
    }
    void* take(size_t bytes) {
        if (!base) return nullptr;
        bytes = (bytes + 63) & ~size_t(63);
        size_t at;
        if (head >= tail) { // free: [head, cap) and [0, tail)
            if (head + bytes <= cap) at = head;
            else if (bytes < tail) at = 0;
            else return nullptr;
        } else {            // free: [head, tail)
            if (head + bytes < tail) at = head;
            else return nullptr;
        }
        head = at + bytes;
        return base + at;
    }
    // every staged download is complete (the owner waited for the stream, or for an event recorded behind them)
    void flush() {
        for (const Pend& q : pend) std::memcpy(q.dst, q.src, q.bytes);
        pend.clear();
    }
    // `m = mark()` taken when an event was recorded; after waiting for that event the slots handed out before it are free
    size_t mark() const { return head; }
    void release(size_t m) { tail = m; }
    // after a full stream synchronisation
    void reset() {
        flush();
        head = tail = 0;
    }
    static Staging*& current() { static thread_local Staging* cur = nullptr; return cur; }
    struct Scope {
        Staging* prev;
        explicit Scope(Staging* s) : prev(current()) { current() = s; }
        ~Scope() { current() = prev; }
    };
};

// Process-wide cache of device allocations.  Every solve builds ~100 DevBufs and drops them again (2.7 ms of hipMalloc /
// hipFree per headline path, 17 solves per 8-fold CV), and hipFree synchronises the device.  Released buffers are parked here by
// (device, size) and handed to the next request of a similar size; consecutive solves on one design ask for the same sizes,
// so after the first solve nothing is allocated.  Contents are NOT zeroed (neither does hipMalloc promise that).  A buffer is
// only parked by its owner's destructor / release(), i.e. after the owner's streams were synchronised.  At most
// `limit_bytes()` stay parked (default 6 GB; adelie_hip_set_config("pool_limit_mb", x); 0 disables the cache and
// "pool_trim" frees what is parked).
struct DevPool {
    struct Entry { size_t bytes; void* p; int dev; };
    static std::mutex& mu() { static std::mutex* m = new std::mutex; return *m; }
    static std::vector<Entry>& parked() { static auto* v = new std::vector<Entry>; return *v; } // (never destroyed: no HIP calls at exit)
    static size_t& parked_bytes() { static size_t b = 0; return b; }
    static size_t& limit_bytes() { static size_t b = size_t(6) << 30; return b; }
    static void* take(size_t bytes) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        std::lock_guard<std::mutex> lk(mu());
        auto& v = parked();
        size_t best = v.size();
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].dev == dev && v[i].bytes >= bytes && v[i].bytes <= bytes + bytes / 8 + 4096 &&
                (best == v.size() || v[i].bytes < v[best].bytes))
                best = i;
        if (best == v.size()) return nullptr;
        void* p = v[best].p;
        parked_bytes() -= v[best].bytes;
        v[best] = v.back();
        v.pop_back();
        return p;
    }
    // returns false when the buffer was not parked (the caller frees it)
    static bool give(void* p, size_t bytes) {
        // the device the block LIVES on, not the calling thread's current one: a result may be destroyed from any thread
        // (C-ABI users, a garbage collector), and a block parked under the wrong device would be handed to a later solve there
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        const int dev = at.device;
        std::lock_guard<std::mutex> lk(mu());
        if (parked_bytes() + bytes > limit_bytes() || parked().size() >= 4096) return false;
        parked().push_back(Entry{bytes, p, dev});
        parked_bytes() += bytes;
        return true;
    }
    static void trim() {
        std::vector<Entry> v;
        {
            std::lock_guard<std::mutex> lk(mu());
            v.swap(parked());
            parked_bytes() = 0;
        }
        for (const Entry& e : v) (void)hipFree(e.p);
    }
};

// Device blocks a DevBuf outgrew in the middle of a solve.  hipFree waits for the whole device, i.e. it drains the queue the
// host has built up (≈ 5 growth events per headline path); with a list installed for the calling thread (run<T>) the old
// block is kept until the end of the solve instead and parked in DevPool once the solve's streams are idle, where the next
// solve's same growth step finds it.
struct DeferredFrees {
    struct Blk { void* p; size_t bytes; };
    std::vector<Blk> v;
    static DeferredFrees*& current() { static thread_local DeferredFrees* cur = nullptr; return cur; }
    struct Scope {
        DeferredFrees* prev;
        explicit Scope(DeferredFrees* d) : prev(current()) { current() = d; }
        ~Scope() { current() = prev; }
    };
    // nothing on the device uses the blocks any more
    void drain() {
        for (const Blk& b : v)
            if (!DevPool::give(b.p, b.bytes)) {
                const auto t0 = std::chrono::steady_clock::now();
                (void)hipFree(b.p);
                DevAllocStats::seconds() += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                ++DevAllocStats::calls();
            }
        v.clear();
    }
    ~DeferredFrees() { drain(); }
};

// Owning device buffer (grow-only).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    // The destructor parks the block in the process-wide cache: the owner has synchronised its streams by then.  A release in
    // the middle of a solve (growth) goes through hipFree, which waits for whatever may still be using the old block.
    ~DevBuf() { release(true); }
    void release(bool park = false) {
        if (p && !park && DeferredFrees::current()) {
            DeferredFrees::current()->v.push_back(DeferredFrees::Blk{p, cap * sizeof(T)});
        } else if (p && !(park && DevPool::give(p, cap * sizeof(T)))) {
            const auto t0 = std::chrono::steady_clock::now();
            (void)hipFree(p);
            DevAllocStats::seconds() += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            ++DevAllocStats::calls();
        }
        p = nullptr;
        cap = 0;
    }
    // allocation through the process-wide cache; `cap` is set to what the block really holds
    static T* alloc(size_t want, size_t& got) {
        // sizes are rounded up so that requests that differ a little between solves (screen sets of slightly different
        // lengths) still find their parked block
        size_t bytes = want * sizeof(T);
        const size_t gran = bytes < (size_t(1) << 16) ? 4096 : (bytes < (size_t(1) << 24) ? (size_t(1) << 16) : (size_t(1) << 21));
        bytes = (bytes + gran - 1) / gran * gran;
        void* q = DevPool::take(bytes);
        if (!q) {
            const auto t0 = std::chrono::steady_clock::now();
            hipError_t e = hipMalloc(&q, bytes);
            if (e != hipSuccess) { // out of memory with blocks parked: give them back and try once more
                (void)hipGetLastError();
                DevPool::trim();
                AHIP_CHECK(hipMalloc(&q, bytes));
            }
            DevAllocStats::seconds() += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            ++DevAllocStats::calls();
        }
        got = bytes / sizeof(T);
        return static_cast<T*>(q);
    }
    // ensure capacity >= n elements; contents are NOT preserved
    T* reserve(size_t n) {
        if (n > cap) {
            release();
            size_t want = n < 16 ? 16 : n;
            p = alloc(want, cap);
        }
        return p;
    }
    // ensure capacity, preserving the first `keep` elements
    T* grow(size_t n, size_t keep, hipStream_t s) {
        if (n <= cap) return p;
        size_t want = cap * 2 > n ? cap * 2 : n;
        if (want < 16) want = 16;
        size_t got = 0;
        T* q = alloc(want, got);
        if (p && keep) AHIP_CHECK(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s));
        if (p && DeferredFrees::current()) { // the copy is ordered on `s`; the old block lives until the end of the solve
            DeferredFrees::current()->v.push_back(DeferredFrees::Blk{p, cap * sizeof(T)});
        } else if (p) {
            AHIP_CHECK(hipStreamSynchronize(s));
            (void)hipFree(p);
        }
        p = q;
        cap = got;
        return p;
    }
    void upload(const T* h, size_t n, hipStream_t s, size_t off = 0) {
        if (!n) return;
        Staging* sg = Staging::current();
        if (sg && sg->stream == s) {
            if (void* slot = sg->take(n * sizeof(T))) {
                std::memcpy(slot, h, n * sizeof(T));
                AHIP_CHECK(hipMemcpyAsync(p + off, slot, n * sizeof(T), hipMemcpyHostToDevice, s));
                return;
            }
            ++sg->n_fallback;
        }
        AHIP_CHECK(hipMemcpyAsync(p + off, h, n * sizeof(T), hipMemcpyHostToDevice, s));
    }
    // NOTE: with a staging arena installed the data reaches `h` at the owner's next Staging::flush() (Solver::sync()).
    void download(T* h, size_t n, hipStream_t s, size_t off = 0) const {
        if (!n) return;
        Staging* sg = Staging::current();
        if (sg && sg->stream == s) {
            if (void* slot = sg->take(n * sizeof(T))) {
                AHIP_CHECK(hipMemcpyAsync(slot, p + off, n * sizeof(T), hipMemcpyDeviceToHost, s));
                sg->pend.push_back(Staging::Pend{h, slot, n * sizeof(T)});
                return;
            }
        }
        AHIP_CHECK(hipMemcpyAsync(h, p + off, n * sizeof(T), hipMemcpyDeviceToHost, s));
    }
};

// The memory of the arrays a design handle owns (dev_array_host.hpp).  A refusal leaves no sticky error behind; a request for
// no bytes still yields a block, so that "null" always means "refused".
struct HipMem {
    static void* alloc(size_t bytes) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 1) == hipSuccess) return q;
        (void)hipGetLastError();
        return nullptr;
    }
    static void free(void* p) { (void)hipFree(p); }
};
template <class T> using DevArr = OwnedArr<T, HipMem>;

// The column of ones of a multi-response view (MultiView::ones): nb ones, padded with zeros like a design column so that vector
// loads past nb stay in bounds.  Enqueued on `s`; the caller synchronises.
template <class T>
void alloc_multi_ones(DevArr<void>& ones, int64_t nb, hipStream_t s) {
    const int64_t len = ((nb + 31) / 32) * 32;
    ones.alloc(size_t(len) * sizeof(T));
    AHIP_CHECK(hipMemsetAsync(ones, 0, size_t(len) * sizeof(T), s));
    launch_fill<T>(static_cast<T*>(ones.get()), T(1), nb, s);
}

// ---- the device arrays of a design handle, grouped by what they belong to ------------------------------------------------------
// Every array is a DevArr: the handle that allocated it frees it when it is deleted, a handle that borrowed it (an alias, a
// slice, a view) frees nothing.  borrow_from() under each group is all that adelie_hip_design_alias does with it, so a new
// array goes into its group's fields and into the borrow_from below them.  Arrays of the design's value type are DevArr<void>.
struct DenseArrs {
    DevArr<void> X; // column-major, leading dimension ld
    int64_t ld = 0;
    void borrow_from(const DenseArrs& o) { X.borrow(o.X), ld = o.ld; }
};
struct SnpArrs {
    DevArr<uint8_t> bits; // 2 bits per call, ldb bytes per column
    int64_t ldb = 0;
    DevArr<void> impute; // (p,) value_t
    void borrow_from(const SnpArrs& o) { bits.borrow(o.bits), ldb = o.ldb, impute.borrow(o.impute); }
};
// sparse (kind 3): column-compressed and row-compressed copies of the stored entries
struct CscArrs {
    DevArr<int64_t> cptr, rptr;
    DevArr<int32_t> cidx, rcol;
    DevArr<void> cval, rval;
    int64_t nnz = 0;
    DevArr<int64_t> bptr; // per-column row-block pointers (p x (sp_nb + 1)) when sp_nb > 1
    int sp_nb = 1;
    int64_t sp_rb = 0;
    // tile-major copy of the entries for the full sweeps (kernels_sparse.hip: csc_tile_sweep_kernel), sp_nt > 0
    DevArr<int64_t> tptr;
    DevArr<uint16_t> trow;
    DevArr<void> tval;
    int sp_nt = 0;
    int64_t sp_th = 0;
    int sp_parts() const { return sp_nb > sp_nt ? sp_nb : sp_nt; } // partial sums per column a sweep may leave
    void borrow_from(const CscArrs& o) {
        cptr.borrow(o.cptr), cidx.borrow(o.cidx), cval.borrow(o.cval), rptr.borrow(o.rptr), rcol.borrow(o.rcol), rval.borrow(o.rval);
        nnz = o.nnz;
        bptr.borrow(o.bptr), sp_nb = o.sp_nb, sp_rb = o.sp_rb;
        tptr.borrow(o.tptr), trow.borrow(o.trow), tval.borrow(o.tval), sp_nt = o.sp_nt, sp_th = o.sp_th;
    }
};
// standardized view (adelie_hip_design_create_standardized): (p,) value_t each, allocated by the view on top of an alias
struct StdArrs {
    DevArr<void> std_center, std_iscale;
    void borrow_from(const StdArrs& o) { std_center.borrow(o.std_center), std_iscale.borrow(o.std_iscale); }
};
// factor design (adelie_hip_design_create_one_hot / _interaction): X is the expanded matrix; next to it a column-major copy of
// the d columns of Z and the per-block descriptors that the structured full sweep reads (kernels_factor.hip).  f_outer (host) =
// the blocks' first columns and P; an alias keeps the structure: CV folds sweep the same way.
struct FactorArrs {
    DevArr<void> fz; // (a convex-relu design keeps its copy of Z here too)
    int64_t fz_ld = 0;
    DevArr<ahip::FactorBlock> fblk;
    DevArr<ahip::FactorChunk> fchunk;
    int64_t f_nchunk = 0;
    std::vector<int64_t> f_outer;
    void borrow_from(const FactorArrs& o) {
        fz.borrow(o.fz), fz_ld = o.fz_ld, fblk.borrow(o.fblk), fchunk.borrow(o.fchunk), f_nchunk = o.f_nchunk, f_outer = o.f_outer;
    }
};
// convex-relu design (adelie_hip_design_create_convex_relu): X is the expanded (n, (gated ? 1 : 2) m d) matrix; next to it the
// column-major copy of Z in fz / fz_ld (d columns) and the (n, m) mask bytes, column-major with leading dimension rmask_ld, that
// the structured full sweep reads (kernels_relu.hip).  r_d / r_m / r_gated also describe the form kept sparse below.
struct ReluArrs {
    DevArr<uint8_t> rmask;
    int64_t rmask_ld = 0, r_d = 0, r_m = 0;
    int r_gated = 0;
    void borrow_from(const ReluArrs& o) { rmask.borrow(o.rmask), rmask_ld = o.rmask_ld, r_d = o.r_d, r_m = o.r_m, r_gated = o.r_gated; }
};
// convex-relu design over a sparse base, kept sparse (adelie_hip_design_create_convex_relu_csc): kind is kCsc and the compressed
// arrays hold the expansion; next to them a copy of Z's column-compressed entries (rz_seg: Z's column pointers refined by the row
// tiles of relu_sparse_shape, rz_idx, rz_val) and the mask packed to 32-bit words per row (rbits), which the structured full
// sweep reads (kernels_relu_sparse.hip).
struct ReluCscArrs {
    DevArr<int64_t> rz_seg;
    DevArr<int32_t> rz_idx;
    DevArr<void> rz_val;
    DevArr<uint32_t> rbits;
    int64_t rz_nnz = 0;
    void borrow_from(const ReluCscArrs& o) {
        rz_seg.borrow(o.rz_seg), rz_idx.borrow(o.rz_idx), rz_val.borrow(o.rz_val), rbits.borrow(o.rbits), rz_nnz = o.rz_nnz;
    }
};
// design made of pieces (adelie_hip_design_create_pieces; pieces_host.hpp): the arrays of up to kMaxPieces dense or 2-bit designs,
// all borrowed -- the pieces own them and outlive this handle (the Python wrapper keeps them) -- with their leading dimensions,
// kinds and first columns.  pc_impute[m] is null on a dense piece.
struct PiecesArrs {
    DevArr<void> pc_base[kMaxPieces], pc_impute[kMaxPieces];
    int64_t pc_ld[kMaxPieces] = {};
    int pc_kind[kMaxPieces] = {};
    int32_t pc_first[kMaxPieces + 1] = {};
    int pc_k = 0;
    void borrow_from(const PiecesArrs& o) {
        for (int m = 0; m < kMaxPieces; ++m)
            pc_base[m].borrow(o.pc_base[m]), pc_impute[m].borrow(o.pc_impute[m]), pc_ld[m] = o.pc_ld[m], pc_kind[m] = o.pc_kind[m];
        for (int m = 0; m <= kMaxPieces; ++m) pc_first[m] = o.pc_first[m];
        pc_k = o.pc_k;
    }
};
// float32 shadow of a dense f64 design for the filtered invariance sweep (kernels_filter.hip: ShadowView), made on the first
// eligible solve.  Like the batcher it lives with the design the aliases were made from: nobody borrows it, the aliases read
// their owner's.  sh_kind (shadow_kind_host.hpp): float32 values, or int16 with the per-column scales in sh_scale.
struct ShadowArrs {
    DevArr<void> sh_X;
    int sh_kind = ahip::kShadowF32;
    DevArr<double> sh_scale; // (p,) q15 only
    int64_t sh_ld = 0;
    DevArr<double> sh_err; // (p,) ||x_j - xs_j||_2
    DevArr<double> sh_nrm; // (p,) ||xs_j||_2
    void reset() { sh_X.reset(), sh_err.reset(), sh_nrm.reset(), sh_scale.reset(), sh_ld = 0, sh_kind = ahip::kShadowF32; }
};

} // namespace ahip

// ---- the opaque handles of include/adelie_hip.h ------------------------------------------------------------
struct adelie_hip_design : ahip::DenseArrs, ahip::SnpArrs, ahip::CscArrs, ahip::StdArrs, ahip::FactorArrs, ahip::ReluArrs,
                           ahip::ReluCscArrs, ahip::PiecesArrs, ahip::ShadowArrs {
    // what adelie_hip_design_alias shares with `o`; o must outlive this handle
    void borrow_arrays(const adelie_hip_design& o) {
        DenseArrs::borrow_from(o), SnpArrs::borrow_from(o), CscArrs::borrow_from(o), StdArrs::borrow_from(o);
        FactorArrs::borrow_from(o), ReluArrs::borrow_from(o), ReluCscArrs::borrow_from(o), PiecesArrs::borrow_from(o);
    }
    int dtype = ADELIE_HIP_F64;
    int device = 0;
    // storage kinds: dense, snp (2-bit), multi-response view of a dense or 2-bit design (adelie_hip_design_create_multi),
    // sparse kept sparse (adelie_hip_design_create_csc: CSC + CSR copies of the entries, kernels_sparse.hip), column blocks of
    // dense and 2-bit designs that stay as they are (adelie_hip_design_create_pieces: PiecesArrs; X, bits and the rest are null)
    enum : int { kDense = 0, kSnp = 1, kMulti = 2, kCsc = 3, kPieces = 4 };
    int kind = kDense;
    bool is_dense() const { return kind == kDense; }
    bool is_snp() const { return kind == kSnp; }
    bool is_multi() const { return kind == kMulti; }
    bool is_csc() const { return kind == kCsc; }
    bool is_pieces() const { return kind == kPieces; }
    // standardized view over a dense or 2-bit design (adelie_hip_design_create_standardized): the base kernels run on the raw
    // matrix, centring and scaling are applied around them; a view over compressed columns applies them inside its kernels
    bool is_std_view() const { return std_center != nullptr && kind != kCsc; }
    // covariance-method matrix A (adelie_hip_design_create_cov_dense): a dense (p, p) design with n == p that only
    // adelie_hip_gaussian_cov_solve and the cov_* operations accept; cov == 2: the stored matrix is A^T (row-major input)
    int cov = 0;
    // ... or kept sparse (adelie_hip_design_create_cov_csc): kind is kCsc with the column-compressed arrays cptr / cidx / cval
    // only -- the row arrays, block pointers and tile copy stay null, so whatever reads those must test `cov` first;
    // cov_lanes is the lane group of kernels_cov_sparse.hip
    int cov_lanes = 0;
    bool cov_csc() const { return cov != 0 && kind == kCsc; }
    // constraint matrix (adelie_hip_design_create_constraint_dense / _csc): this dense or kCsc handle is the (d, m) matrix A' of an
    // (m, d) constraint matrix A, so n == d and p == m; only adelie_hip_constraint_op and adelie_hip_pinball_solve accept it
    int constraint = 0;
    int64_t n = 0, p = 0;
    // multi-response view: [1 (x) I_K, X (x) I_K] over the base's X (nb x pb); n = nb*K, p = (pb + micpt)*K
    int64_t mK = 0, nb = 0, pb = 0;
    int micpt = 0;
    ahip::DevArr<void> ones; // nb ones
    // Sweep batching across solvers that run concurrently on one resident matrix (cv_grpnet folds on alias handles): the
    // batcher object lives with the design the aliases were made from (solver.hip::SweepBatcher, created on first use).
    adelie_hip_design* batch_owner = nullptr; // nullptr: this design itself
    void* batcher = nullptr;
    int sh_state = 0; // the shadow: 0: none yet, 1: built, -1: ineligible (an entry float32 cannot hold, memory, a failed staleness check)
    int64_t sh_n_ineligible = 0, sh_n_builds = 0;
    std::mutex sh_mu;
    hipStream_t stream = nullptr;
    // scratch for the host-vector matrix ops (value_t typed, grow-only)
    ahip::DevBuf<char> s_n1, s_n2, s_p1, s_work, s_misc, s_idx1, s_idx2;

    template <class T> ahip::DenseView<T> dense() const { return ahip::DenseView<T>{static_cast<const T*>(X), n, p, ld}; }
    ahip::SnpView snp() const { return ahip::SnpView{bits, n, p, ldb}; }
    template <class T> ahip::PiecesView<T> pieces() const {
        ahip::PiecesView<T> v{};
        for (int m = 0; m < ahip::kMaxPieces; ++m)
            v.base[m] = pc_base[m], v.ld[m] = pc_ld[m], v.impute[m] = static_cast<const T*>(pc_impute[m]);
        for (int m = 0; m <= ahip::kMaxPieces; ++m) v.first[m] = pc_first[m];
        v.k = pc_k, v.n = n, v.p = p;
        return v;
    }
    template <class T> ahip::CscView<T> csc() const {
        return ahip::CscView<T>{cptr, cidx, static_cast<const T*>(cval), rptr, rcol, static_cast<const T*>(rval), n, p, nnz,
                                bptr, sp_nb, sp_rb, static_cast<const T*>(std_center), static_cast<const T*>(std_iscale),
                                tptr, trow, static_cast<const T*>(tval), sp_nt, sp_th};
    }
    template <class T> ahip::CovCscView<T> cov_csc_view() const {
        return ahip::CovCscView<T>{cptr, cidx, static_cast<const T*>(cval), p, cov_lanes};
    }
    bool factor() const { return fblk != nullptr; }
    template <class T> ahip::FactorView<T> factor_view() const {
        return ahip::FactorView<T>{static_cast<const T*>(fz), n, fz_ld, p, fblk, fchunk, f_nchunk};
    }
    bool relu() const { return rmask != nullptr; }
    template <class T> ahip::ReluView<T> relu_view() const {
        return ahip::ReluView<T>{static_cast<const T*>(fz), n, fz_ld, rmask, rmask_ld, r_d, r_m, r_gated};
    }
    bool relu_csc() const { return rbits != nullptr; }
    template <class T> ahip::ReluCscView<T> relu_csc_view() const {
        const ahip::ReluSparseShape sh = ahip::relu_sparse_shape(n, r_m);
        return ahip::ReluCscView<T>{rz_seg, rz_idx, static_cast<const T*>(rz_val), rbits, n, r_d, r_m, r_gated, sh.tile_rows, int(sh.tiles)};
    }
    template <class T> ahip::MultiView<T> multi() const {
        return ahip::MultiView<T>{static_cast<const T*>(X), nb, pb, ld, static_cast<const T*>(ones), int32_t(mK), int32_t(micpt),
                                  bits, ldb, static_cast<const T*>(impute)};
    }
};

// The shadow of `d` (of the design its aliases were made from), built on d's stream if there is none yet: false when the
// design has none and cannot have one.  mark_stale: a staleness check failed -- no later solve takes the shadow.
extern "C" {
bool adelie_hip_internal_shadow_acquire(adelie_hip_design* d, ahip::ShadowView* out); // design.hip
void adelie_hip_internal_shadow_mark_stale(adelie_hip_design* d);
}
