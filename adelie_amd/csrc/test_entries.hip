// test_entries.hip — C ABI: the entries that exist for the tests and the micro-benchmarks only.
//
// Each one runs ONE piece of the device code on caller-supplied inputs -- a sweep, a block build, a piece of the group engine, a
// launcher of kernels_multi.hip, a touch of the covariance matrix -- through the launcher or dispatcher the solver itself calls
// (kernels.hpp, design_ops.hpp, filter_host.hpp), so that a test sees what a solve would launch.  Nothing here touches the path
// driver of solver.hip.  Everything a kernel indexes by is checked against the buffers' sizes before anything is launched, and a
// caller's array is written only after the last download and its synchronise.
#include "common.hpp"
#include "design_ops.hpp"
#include "filter_host.hpp"

#include <algorithm>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

namespace ahip {
// the IRLS launchers of kernels_glm.hip, as solver.hip declares them beside its path driver (launch_glm_loss2 and
// launch_multi_loss2 are in kernels.hpp)
template <class T>
void launch_irls_prepare(int kind, const T* y, const T* w, const T* eta, const T* resid, const T* offsets, T hessian_min,
                         int64_t n, T* hess, T* irls_resid, T* irls_y, T* sums, hipStream_t s, int K);
template <class T>
void launch_irls_weights(const T* hess, T hess_sum, const T* irls_y, T shift, int64_t n, T* wts, T* irls_resid, T* sums,
                         hipStream_t s);
template <class T>
void launch_irls_finish(int kind, const T* y, const T* w, const T* irls_y, const T* offsets, const T* irls_resid, T shift,
                        int64_t n, T* eta, T* resid, T* sums, hipStream_t s, int K);
template <class T>
void launch_glm_gradient(int kind, const T* y, const T* w, const T* eta, int64_t n, T* resid, hipStream_t s, int K);
template <class T>
void launch_glm_loss(int kind, const T* y, const T* w, const T* eta, int64_t n, T* sums, hipStream_t s, int K);
template <class T>
void launch_null_step(int kind, const T* y, const T* w, const T* eta, const T* resid, const T* offsets, T hessian_min,
                      int64_t n, T* sums, hipStream_t s, int K, const T* cb_hess, const T* cb_z);
template <class T>
void launch_set_eta(const T* offsets, T beta0, int64_t n, T* eta, hipStream_t s);
template <class T>
void launch_dot_diff(const T* a, const T* a0, const T* b, const T* b0, int64_t n, T* sums, hipStream_t s);
template <class T>
void launch_rel_change(const T* a, T* prev, int64_t n, T* out, hipStream_t s);
template <class T>
void launch_gather(const T* src, const int32_t* idx, int64_t cnt, T* dst, hipStream_t s);
template <class T>
void launch_scatter(const T* src, const int32_t* idx, int64_t cnt, T* dst, hipStream_t s);
} // namespace ahip

using namespace ahip;

namespace {

// The host <-> device staging of an entry on its stream `s`.
struct Stage {
    hipStream_t s = nullptr;
    struct Back { void* dst; std::vector<char> h; };
    std::deque<Back> back; // downloads under way, in the order they were asked for
    // reserve + upload
    template <class B, class H>
    void up(B& buf, const H* h, int64_t n) const { buf.reserve(size_t(n)); buf.upload(h, size_t(n), s); }
    // reserve + clear
    template <class B>
    void zeros(B& buf, int64_t n) const { AHIP_CHECK(hipMemsetAsync(buf.reserve(size_t(n)), 0, size_t(n) * sizeof(*buf.p), s)); }
    void down(void* h, const void* dev, size_t bytes) const { AHIP_CHECK(hipMemcpyAsync(h, dev, bytes, hipMemcpyDeviceToHost, s)); }
    // download towards the caller's array `dst`: it lands in a host block of the stage and reaches dst in deliver()
    void fetch(void* dst, const void* dev, size_t bytes) {
        back.push_back(Back{dst, std::vector<char>(bytes)});
        down(back.back().h.data(), dev, bytes);
    }
    void sync() const { AHIP_CHECK(hipStreamSynchronize(s)); }
    // after sync(): the caller's arrays
    void deliver() {
        for (const Back& b : back) std::memcpy(b.dst, b.h.data(), b.h.size());
        back.clear();
    }
    void land() { sync(), deliver(); }
    // check the launches, download, synchronise, then write the caller's array
    void finish(void* dst, const void* dev, size_t bytes) {
        AHIP_CHECK(hipGetLastError());
        fetch(dst, dev, bytes);
        land();
    }
};

// the plain strip kernel while this lives: set_strip_lds(true) comes back on every way out, a throwing launch included
struct PlainStrips {
    const bool on;
    explicit PlainStrips(bool o) : on(o) { if (on) set_strip_lds(false); }
    ~PlainStrips() { if (on) set_strip_lds(true); }
};

} // namespace

extern "C" {

// Times `reps` launches of the dominant kernel with HIP events on the design's own stream.
int adelie_hip_bench_sweep(adelie_hip_design* d, int64_t reps, double* ms_per_launch) {
    ABI_TRY
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
    DTYPE_DISPATCH(d, body(T{}))
    ABI_CATCH
}

// One filtered invariance sweep on a dense f64 design, as a solve at one lambda enqueues it: v = w o r, the shadow sweep, the
// classification against tstar, the exact sweeps of the screen groups' columns, of the groups without a penalty and of the
// groups listed.  grad (p), exact (p: 1 where the value is the full sweep's), info: [0] columns listed, [1] flags (1: more
// than the cap of max(1024, p/4) were wanted, 2: a column swept both ways left its bound), [2] 1 if the route ran, 0 if
// the plain full sweep answered (hook off, no shadow), [3] columns wanted.
int adelie_hip_filter_sweep_test(adelie_hip_design* d, const double* w, const double* r, double sub_scale, const double* sub_vec,
                                 const int64_t* screen_groups, int64_t n_screen, const int64_t* groups, const int64_t* group_sizes,
                                 int64_t G, const double* penalty, double tstar, double* grad, uint8_t* exact, int64_t* info) {
    ABI_TRY
    if (!d || !w || !r || !groups || !group_sizes || !penalty || !grad || !exact || !info || G < 1 || n_screen < 0)
        throw make_core_error("bad arguments.");
    if (!d->is_dense() || d->dtype != ADELIE_HIP_F64 || d->cov || d->constraint || d->std_center) throw make_core_error("a dense f64 design is required.");
    AHIP_CHECK(hipSetDevice(d->device));
    hipStream_t s = d->stream;
    const Stage st{s};
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
    dv.reserve(n); dgrad.reserve(p); dlist.reserve(cap); dmeta.reserve(4); dmetad.reserve(2);
    const int n_part = filter_norm_parts(n);
    dpart.reserve(n_part);
    work.reserve(size_t(std::max(filtered_sweep_work_elems(n, p, int64_t(scols.size() + pen0.size()), cap), sweep_work_elems(n, p))));
    st.up(dw, w, n); st.up(dr, r, n); st.up(dsc, &sub_scale, 1); st.up(dpen, penalty, G);
    st.up(dgroups, groups, G); st.up(dgs, group_sizes, G); st.up(dslot, slot.data(), G);
    if (sub_vec) st.up(dxm, sub_vec, p);
    if (!scols.empty()) st.up(dscols, scols.data(), int64_t(scols.size()));
    if (!pen0.empty()) st.up(dpen0, pen0.data(), int64_t(pen0.size()));
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
        st.down(meta, dmeta.p, sizeof(meta));
        st.sync();
        list.resize(size_t(meta[0]));
        if (meta[0] > 0) st.down(list.data(), dlist.p, size_t(meta[0]) * sizeof(int32_t));
        std::fill(exact, exact + p, uint8_t(0));
    }
    st.down(grad, dgrad.p, size_t(p) * sizeof(double));
    st.sync();
    if (route) {
        for (int32_t c : scols) exact[c] = 1;
        for (int32_t c : pen0) exact[c] = 1;
        for (int32_t c : list) exact[c] = 1;
        if (meta[1] & 2) adelie_hip_internal_shadow_mark_stale(d);
    }
    info[0] = meta[0]; info[1] = meta[1]; info[2] = route ? 1 : 0; info[3] = meta[2];
    ABI_CATCH
}

// One block build on caller-supplied inputs, through the launcher the solver calls (include/adelie_hip.h has the layout of `table`
// and `info`).
int adelie_hip_block_build_test(adelie_hip_design* d, int mode, int64_t row_off, const void* w, const int32_t* cols, int64_t n_cols,
                                const int64_t* table, int64_t count, const void* xm, int center, int64_t ldc, int strip_plain,
                                void* out0, int64_t out0_elems, void* out1, int64_t out1_elems, int64_t* info) {
    ABI_TRY
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
    const Stage st{s};
    last_build_launch() = BuildLaunchInfo{};
    auto body = [&](auto tag) {
        using T = decltype(tag);
        DevBuf<T> dw, dxm, dC, dX, work;
        DevBuf<int32_t> dcols;
        st.up(dw, static_cast<const T*>(w), n);
        st.up(dcols, cols, n_cols);
        if (xm) st.up(dxm, static_cast<const T*>(xm), p);
        st.up(dC, static_cast<const T*>(out0), out0_elems);
        if (out1) st.up(dX, static_cast<const T*>(out1), out1_elems);
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
            const PlainStrips plain(strip_plain != 0);
            launch_strip_batch<T>(Xd, dw.p, dcols.p, stb, xmp, ctr, dC.p, out1 ? dX.p : dC.p, ldc, wk, s);
        }
        AHIP_CHECK(hipGetLastError());
        st.down(out0, dC.p, size_t(out0_elems) * sizeof(T));
        if (out1) st.down(out1, dX.p, size_t(out1_elems) * sizeof(T));
        st.sync();
    };
    DTYPE_DISPATCH(d, body(T{}))
    const BuildLaunchInfo& r = last_build_launch();
    info[0] = r.kind; info[1] = r.nsplit; info[2] = r.kchunk; info[3] = r.tile; info[4] = r.n128; info[5] = r.n64;
    info[6] = r.vec16; info[7] = r.strip_lt; info[8] = r.symmetric;
    info[9] = d->is_csc() ? d->sp_nb : 0;
    ABI_CATCH
}

// One device piece of the group engine on caller-supplied inputs, through the launcher the solver calls (include/adelie_hip.h has
// the modes and the arrays).
int adelie_hip_group_piece_test(const adelie_hip_group_piece* a, int64_t* info) {
    ABI_TRY
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
    Stage st{s};
    int64_t launches = 0;
    auto body = [&](auto tag) {
        using T = decltype(tag);
        if (mode == ADELIE_HIP_GROUP_EIG) {
            DevBuf<T> dsrc, dvars, dV;
            DevBuf<EigDesc> dd;
            st.up(dsrc, static_cast<const T*>(a->src), a->src_elems);
            st.up(dvars, static_cast<const T*>(a->vars), a->vars_elems);
            st.up(dV, static_cast<const T*>(a->V), a->V_elems);
            st.up(dd, edesc.data(), int64_t(edesc.size()));
            launch_grp_eig<T>(dsrc.p, dd.p, int(a->count), int(a->max_q), dvars.p, dV.p, s);
            ++launches;
            AHIP_CHECK(hipGetLastError());
            st.fetch(a->vars, dvars.p, size_t(a->vars_elems) * sizeof(T));
            st.fetch(a->V, dV.p, size_t(a->V_elems) * sizeof(T));
            st.land();
            return;
        }
        if (mode == ADELIE_HIP_GROUP_ROTATE) {
            DevBuf<T> dD, dS, dV, scratch;
            st.up(dD, static_cast<const T*>(a->D), SLOT);
            if (a->Dsrc) st.up(dS, static_cast<const T*>(a->Dsrc), SLOT);
            st.up(dV, static_cast<const T*>(a->V), a->V_elems);
            scratch.reserve(size_t(SLOT));
            launch_grp_block_rotate<T>(dD.p, a->Dsrc ? dS.p : dD.p, dV.p, rot, scratch.p, s);
            ++launches;
            st.finish(a->D, dD.p, size_t(SLOT) * sizeof(T));
            return;
        }
        const int64_t nblk = a->nblk, ns = a->ns, nv = a->nv;
        DevBuf<int32_t> dsb, dsz, dg0, dlist, ddesc, dvcol, dact, ddcol, ddidx;
        DevBuf<int64_t> dvoff;
        DevBuf<int8_t> disact;
        DevBuf<T> dvars, dV, dxm, dspen, dbeta, dg, dC, dDb, dgb, ddlt, ddd, dDbuf;
        DevBuf<CdBlkState<T>> dst;
        st.up(dsb, a->sbegin, ns); st.up(dsz, a->ssize, ns); st.up(dvoff, a->voff, ns); st.up(dg0, a->blk_g0, nblk + 1);
        if (a->list) st.up(dlist, a->list, a->n_list);
        st.zeros(ddesc, nblk * GDESC_STRIDE); // (the unnamed gaps)
        CdGrpBlkParams<T> p{};
        p.nv = int32_t(nv);
        p.sbegin = dsb.p; p.ssize = dsz.p; p.voff = dvoff.p; p.blk_g0 = dg0.p; p.list = a->list ? dlist.p : nullptr;
        p.nblk = int32_t(nblk);
        launch_grp_layout<T>(p, int(nblk), ddesc.p, s);
        ++launches;
        AHIP_CHECK(hipGetLastError());
        st.fetch(a->desc, ddesc.p, size_t(nblk * GDESC_STRIDE) * sizeof(int32_t));
        if (!solve) {
            st.land();
            return;
        }
        const bool panel = mode == ADELIE_HIP_GROUP_PANEL_SOLVE;
        st.up(dvars, static_cast<const T*>(a->vars), nv); st.up(dV, static_cast<const T*>(a->V), a->V_elems);
        st.up(dxm, static_cast<const T*>(a->xmean), nv); st.up(dspen, static_cast<const T*>(a->spen), ns);
        st.up(dbeta, static_cast<const T*>(a->beta), nv); st.up(dvcol, a->vcol, nv); st.up(disact, a->is_active, ns);
        dact.reserve(size_t(2 * ns + 1)); // a group is marked at most once: active_size <= ns on entry, at most ns more
        dact.upload(a->active_set, size_t(ns), s);
        CdBlkState<T> st0{};
        st0.rsq = T(a->rsq); st0.resid_sum = T(a->resid_sum); st0.n_updates = a->n_updates; st0.active_size = int32_t(a->active_size);
        st.up(dst, &st0, 1);
        p.vars = dvars.p; p.xmean = dxm.p; p.beta = dbeta.p; p.is_active = disact.p; p.active_set = dact.p;
        p.l1 = T(a->l1); p.l2 = T(a->l2); p.newton_tol = T(a->newton_tol); p.dbeta_tol = T(a->dbeta_tol);
        p.newton_max_iters = int32_t(a->newton_max_iters); p.max_active_size = int32_t(a->max_active_size); p.mark = a->mark ? 1 : 0;
        p.V = dV.p; p.spen = dspen.p; p.st = dst.p; p.vcol = dvcol.p;
        std::vector<CdBlkState<T>> hst(size_t(panel ? nblk : 1));
        if (panel) {
            st.up(dDb, static_cast<const T*>(a->Dblk), nblk * SLOT); st.up(dgb, static_cast<const T*>(a->gblk), nblk * G);
            st.up(ddlt, static_cast<const T*>(a->dlt), nblk * G); st.up(ddd, static_cast<const T*>(a->dd), nblk * G); st.up(ddcol, a->dcol, nblk * G);
            p.rot = 1; p.desc = ddesc.p;
            for (int64_t j = 0; j < nblk; ++j) {
                p.Dptr = dDb.p + j * SLOT; p.gblk = dgb.p + j * G;
                p.dlt = ddlt.p + j * G; p.dd = ddd.p + j * G; p.dcol = ddcol.p + j * G;
                launch_cd_group_panel_solve<T>(p, int(j), s);
                ++launches;
                st.down(&hst[size_t(j)], dst.p, sizeof(CdBlkState<T>));
            }
            AHIP_CHECK(hipGetLastError());
            st.fetch(a->dlt, ddlt.p, size_t(nblk * G) * sizeof(T)); st.fetch(a->dd, ddd.p, size_t(nblk * G) * sizeof(T));
            st.fetch(a->dcol, ddcol.p, size_t(nblk * G) * sizeof(int32_t));
        } else {
            st.up(dC, static_cast<const T*>(a->C), a->ldc * nv);
            st.up(dg, static_cast<const T*>(a->g), nv);
            dDbuf.reserve(size_t(2 * SLOT)); ddlt.reserve(size_t(G)); ddidx.reserve(size_t(G));
            p.C = dC.p; p.ldc = a->ldc; p.g = dg.p; p.Dbuf = dDbuf.p; p.dlt = ddlt.p; p.didx = ddidx.p; p.rot = 0;
            launch_cd_group_block_pass<T>(p, s);
            launches += 1 + 2 * nblk;
            AHIP_CHECK(hipGetLastError());
            st.down(&hst[0], dst.p, sizeof(CdBlkState<T>));
            st.fetch(a->g, dg.p, size_t(nv) * sizeof(T));
        }
        st.fetch(a->beta, dbeta.p, size_t(nv) * sizeof(T));
        st.fetch(a->active_set, dact.p, size_t(ns) * sizeof(int32_t));
        st.fetch(a->is_active, disact.p, size_t(ns));
        st.land();
        for (size_t j = 0; j < hst.size(); ++j) {
            a->st_f[3 * j] = double(hst[j].rsq); a->st_f[3 * j + 1] = double(hst[j].resid_sum); a->st_f[3 * j + 2] = double(hst[j].cm);
            a->st_i[4 * j] = hst[j].n_updates; a->st_i[4 * j + 1] = hst[j].active_size; a->st_i[4 * j + 2] = hst[j].status;
            a->st_i[4 * j + 3] = hst[j].nz;
        }
    };
    DTYPE_DISPATCH(a, body(T{}))
    info[0] = launches;
    info[1] = rot_wide ? 1 : 0;
    ABI_CATCH
}

// One launcher of kernels_multi.hip on caller-supplied inputs (include/adelie_hip.h has the modes and the arrays).
int adelie_hip_multi_piece_test(const adelie_hip_multi_piece* a, int64_t* info) {
    ABI_TRY
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
    Stage st{s};
    for (int q = 0; q < 8; ++q) info[q] = 0;
    auto body = [&](auto tag) {
        using T = decltype(tag);
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
                st.up(dbits, a->bits, a->bits_elems);
                st.up(dimp, static_cast<const T*>(a->impute), pb);
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
            st.up(dout, static_cast<const T*>(a->out), ncol);
            dwork.reserve(size_t(multi_sweep_work_elems<T>(mv)));
            const T* v = dv.p + a->v_off;
            const MSweepPlan pl = multi_sweep_plan<T>(mv, v);
            if (int64_t(pl.nsplit) * ncol > multi_sweep_work_elems<T>(mv)) throw make_core_error("SWEEP: the work size does not cover the plan.");
            launch_multi_sweep<T>(mv, v, dout.p, dwork.p, s);
            info[0] = pl.variant; info[1] = pl.vec; info[2] = pl.kt; info[3] = pl.feats; info[4] = pl.blocks_c; info[5] = pl.nsplit;
            info[6] = pl.rows_per_split; info[7] = pl.kchunks;
            st.finish(a->out, dout.p, size_t(ncol) * sizeof(T));
            return;
        }
        if (step || mode == ADELIE_HIP_MULTI_AXPY) {
            st.up(dr, static_cast<const T*>(a->r), nb * K);
            ddcol.reserve(size_t(G)); ddlt.reserve(size_t(G));
            if (a->n_dcol > 0) st.up(ddcol, a->dcol, a->n_dcol);
            if (n_used > 0) st.up(ddlt, static_cast<const T*>(a->dlt), a->n_dcol);
            const int32_t nz32 = int32_t(a->nz);
            st.up(dnz, &nz32, 1);
        }
        if (mode == ADELIE_HIP_MULTI_AXPY) {
            launch_multi_axpy_cols<T>(mv, ddcol.p, ddlt.p, dnz.p, T(a->sign), dr.p, s);
            st.finish(a->r, dr.p, size_t(nb * K) * sizeof(T));
            return;
        }
        if (step) {
            const bool fused = mode == ADELIE_HIP_MULTI_FUSED_STEP;
            const int vec = multi_step_vec<T>(mv);
            const int64_t ld = fused ? mfused_part_ld(nb, vec) : mstep_slices(nb, vec);
            if (a->nb_cols * ld > a->part_elems) throw make_core_error("STEP: part holds fewer than nb_cols * slices elements.");
            st.up(dw, static_cast<const T*>(a->w), nb * K);
            st.up(dpart, static_cast<const T*>(a->part), a->part_elems);
            dcols.reserve(size_t(2 * G));
            if (a->nb_cols > 0) st.up(dcols, a->cols, a->nb_cols);
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
                st.up(dsb, &zero32, 1); st.up(dsz, &one32, 1); st.up(dvoff, &zero64, 1); st.up(dg0, g0, 2);
                st.zeros(ddesc, GDESC_STRIDE);
                CdGrpBlkParams<T> p{};
                p.nv = 1;
                p.sbegin = dsb.p; p.ssize = dsz.p; p.voff = dvoff.p; p.blk_g0 = dg0.p; p.list = nullptr;
                p.nblk = 1;
                launch_grp_layout<T>(p, 1, ddesc.p, s);
                st.up(dvars, &one, 1); st.up(dV, &one, 1); st.up(dxm, &zero, 1); st.up(dspen, &one, 1); st.up(dbeta, &zero, 1);
                st.up(dvcol, &zero32, 1); st.up(disact, &zero8, 1);
                st.zeros(dact, 3);
                CdBlkState<T> st0{};
                st.up(dst, &st0, 1);
                st.zeros(dDb, SLOT); st.zeros(dgb, G); st.zeros(dsdlt, G); st.zeros(dsdd, G); st.zeros(dsdcol, G);
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
            st.fetch(a->r, dr.p, size_t(nb * K) * sizeof(T));
            st.fetch(a->part, dpart.p, size_t(a->part_elems) * sizeof(T));
            st.sync();
            if (got != ld) throw make_core_error("STEP: the launcher's leading dimension differs from the one part was sized for.");
            st.deliver();
            return;
        }
        if (mode == ADELIE_HIP_MULTI_BLOCK_LISTS) {
            DevBuf<int32_t> du, dsl, drs;
            st.up(dcols, a->cols, a->nv); st.up(du, a->ulist, a->nv); st.up(dsl, a->slot, a->nv); st.up(drs, a->resp, a->nv);
            launch_multi_block_lists(dcols.p, int(a->nv), int(K), du.p, dsl.p, drs.p, s);
            AHIP_CHECK(hipGetLastError());
            st.fetch(a->ulist, du.p, size_t(a->nv) * 4); st.fetch(a->slot, dsl.p, size_t(a->nv) * 4); st.fetch(a->resp, drs.p, size_t(a->nv) * 4);
            st.land();
            return;
        }
        if (mode == ADELIE_HIP_MULTI_EXPAND || mode == ADELIE_HIP_MULTI_EXPAND_CROSS) {
            DevBuf<int32_t> dsl, drs, dslc, drsc;
            DevBuf<T> dC, dD;
            st.up(dsl, a->slot, a->nv); st.up(drs, a->resp, a->nv);
            st.up(dC, static_cast<const T*>(a->C), a->C_elems); st.up(dD, static_cast<const T*>(a->D), a->D_elems);
            if (mode == ADELIE_HIP_MULTI_EXPAND) {
                for (int64_t q = 0; q < a->n_lsel; ++q)
                    launch_multi_expand<T>(dC.p, a->ldc, dsl.p, drs.p, int(a->nv), int(a->lsel_list[q]), dD.p, a->ldd, s);
            } else {
                st.up(dslc, a->slot_c, a->nc); st.up(drsc, a->resp_c, a->nc);
                launch_multi_expand_cross<T>(dC.p, a->ldc, dsl.p, drs.p, int(a->nv), dslc.p, drsc.p, int(a->nc), dD.p, a->ldd, s);
            }
            st.finish(a->D, dD.p, size_t(a->D_elems) * sizeof(T));
            return;
        }
        if (mode == ADELIE_HIP_MULTI_TO_MAJOR || mode == ADELIE_HIP_MULTI_FROM_MAJOR) {
            st.up(dv, static_cast<const T*>(a->v), nb * K); st.up(dout, static_cast<const T*>(a->out), nb * K);
            if (mode == ADELIE_HIP_MULTI_TO_MAJOR) launch_multi_to_major<T>(dv.p, nb, int(K), dout.p, s);
            else launch_multi_from_major<T>(dv.p, nb, int(K), dout.p, s);
            st.finish(a->out, dout.p, size_t(nb * K) * sizeof(T));
            return;
        }
        // BATCH_PICK
        st.up(dv, static_cast<const T*>(a->v), pb * K); st.up(dout, static_cast<const T*>(a->out), pb);
        const T scale = T(a->sign);
        st.up(dr, &scale, 1);
        if (a->w) st.up(dw, static_cast<const T*>(a->w), pb);
        launch_batch_pick<T>(dv.p, pb, int(K), int(a->lsel), dr.p, a->w ? dw.p : nullptr, dout.p, s);
        st.finish(a->out, dout.p, size_t(pb) * sizeof(T));
    };
    DTYPE_DISPATCH(a, body(T{}))
    ABI_CATCH
}

// One launcher of kernels_glm.hip on caller-supplied inputs (include/adelie_hip.h has the modes and the arrays).
int adelie_hip_glm_piece_test(const adelie_hip_glm_piece* a, int64_t* info) {
    ABI_TRY
    if (!a || !info) throw make_core_error("bad arguments.");
    if (a->dtype != ADELIE_HIP_F64 && a->dtype != ADELIE_HIP_F32) throw make_core_error("bad dtype.");
    if (a->mode < ADELIE_HIP_GLM_PIECE_PREPARE || a->mode > ADELIE_HIP_GLM_PIECE_SCATTER) throw make_core_error("unknown mode.");
    constexpr int64_t BIG = int64_t(1) << 24, SUMS = 16 + 4 * 256;
    const int mode = int(a->mode);
    const int64_t n = a->n, nb = a->nb, K = a->K, cnt = a->cnt;
    const bool moves = mode == ADELIE_HIP_GLM_PIECE_GATHER || mode == ADELIE_HIP_GLM_PIECE_SCATTER;
    const bool irls = mode == ADELIE_HIP_GLM_PIECE_PREPARE || mode == ADELIE_HIP_GLM_PIECE_FINISH || mode == ADELIE_HIP_GLM_PIECE_NULL_STEP;
    const bool member = irls || mode == ADELIE_HIP_GLM_PIECE_GRADIENT || mode == ADELIE_HIP_GLM_PIECE_LOSS ||
                        mode == ADELIE_HIP_GLM_PIECE_LOSS2 || mode == ADELIE_HIP_GLM_PIECE_MULTI_LOSS2; // takes a kind
    const bool reduces = !(moves || mode == ADELIE_HIP_GLM_PIECE_FINISH || mode == ADELIE_HIP_GLM_PIECE_GRADIENT ||
                           mode == ADELIE_HIP_GLM_PIECE_SET_ETA);
    int kind = 0;
    bool multinomial = false, cb = false, pre = false;
    if (member) {
        if (a->kind < ADELIE_HIP_GLM_GAUSSIAN || a->kind > ADELIE_HIP_GLM_COX) throw make_core_error("unknown kind.");
        kind = int(a->kind);
        multinomial = kind == ADELIE_HIP_GLM_MULTINOMIAL;
        cb = kind == ADELIE_HIP_GLM_CALLBACK;
        pre = cb || kind == ADELIE_HIP_GLM_COX;
        if (pre && !irls) throw make_core_error("the CALLBACK and COX kinds are taken by PREPARE, FINISH and NULL_STEP only.");
        if (mode == ADELIE_HIP_GLM_PIECE_MULTI_LOSS2 && kind != ADELIE_HIP_GLM_GAUSSIAN && !multinomial)
            throw make_core_error("MULTI_LOSS2 takes the kinds GAUSSIAN and MULTINOMIAL.");
        if (mode == ADELIE_HIP_GLM_PIECE_LOSS2 && multinomial) throw make_core_error("LOSS2 does not take MULTINOMIAL (MULTI_LOSS2 does).");
    }
    // the sizes the kernels index by
    const bool row_coupled = mode == ADELIE_HIP_GLM_PIECE_MULTI_LOSS2 ||
                             (multinomial && (mode == ADELIE_HIP_GLM_PIECE_PREPARE || mode == ADELIE_HIP_GLM_PIECE_FINISH ||
                                              mode == ADELIE_HIP_GLM_PIECE_GRADIENT || mode == ADELIE_HIP_GLM_PIECE_LOSS));
    if (!moves) {
        if (n < 1 || n > BIG) throw make_core_error("1 <= n <= 2^24 is required.");
        if (row_coupled && (K < 1 || K > 64 || nb < 1 || nb > BIG || n != nb * K))
            throw make_core_error("a row-coupled launch needs 1 <= K <= 64, nb >= 1 and n == nb * K.");
        if (multinomial && mode == ADELIE_HIP_GLM_PIECE_NULL_STEP && (K < 1 || K > 64)) throw make_core_error("NULL_STEP: 1 <= K <= 64 is required.");
    } else {
        if (cnt < 0 || cnt > BIG || !a->idx || !a->src || !a->dst) throw make_core_error("GATHER / SCATTER: 0 <= cnt <= 2^24, idx, src and dst are required.");
        const int64_t range = mode == ADELIE_HIP_GLM_PIECE_GATHER ? a->src_elems : a->dst_elems;
        if (range < 1 || range > BIG) throw make_core_error("GATHER / SCATTER: 1 <= src_elems (dst_elems) <= 2^24 is required.");
        std::vector<uint8_t> seen(mode == ADELIE_HIP_GLM_PIECE_SCATTER ? size_t(range) : 0, 0);
        for (int64_t q = 0; q < cnt; ++q) {
            if (a->idx[q] < 0 || a->idx[q] >= range) throw make_core_error("GATHER / SCATTER: an index lies outside the array it addresses.");
            if (mode == ADELIE_HIP_GLM_PIECE_SCATTER) {
                if (seen[size_t(a->idx[q])]) throw make_core_error("SCATTER: the indices must be distinct.");
                seen[size_t(a->idx[q])] = 1;
            }
        }
    }
    if (reduces && !a->sums) throw make_core_error("sums is required.");
    // the arrays the launcher reads or writes for this mode and kind
    auto need = [&](const void* p, const char* what) {
        if (!p) throw make_core_error(std::string(what) + " is required for this mode and kind.");
    };
    switch (mode) {
    case ADELIE_HIP_GLM_PIECE_PREPARE:
        need(a->eta, "eta"), need(a->off, "off"), need(a->hess, "hess"), need(a->irls_resid, "irls_resid"), need(a->irls_y, "irls_y");
        if (!pre) need(a->y, "y"), need(a->w, "w");
        if (!cb) need(a->resid, "resid");
        break;
    case ADELIE_HIP_GLM_PIECE_WEIGHTS:
        need(a->hess, "hess"), need(a->irls_y, "irls_y"), need(a->wts, "wts"), need(a->irls_resid, "irls_resid");
        if (!(a->hess_sum == a->hess_sum) || a->hess_sum == 0) throw make_core_error("WEIGHTS: hess_sum must be a non-zero number.");
        break;
    case ADELIE_HIP_GLM_PIECE_FINISH:
        need(a->irls_y, "irls_y"), need(a->off, "off"), need(a->irls_resid, "irls_resid"), need(a->eta, "eta"), need(a->resid, "resid");
        if (!pre) need(a->y, "y"), need(a->w, "w");
        break;
    case ADELIE_HIP_GLM_PIECE_NULL_STEP:
        need(a->eta, "eta"), need(a->off, "off");
        if (!pre) need(a->y, "y"), need(a->w, "w");
        if (!cb) need(a->resid, "resid");
        if (pre) need(a->hess, "hess");
        if (cb) need(a->cb_z, "cb_z");
        break;
    case ADELIE_HIP_GLM_PIECE_GRADIENT:
        need(a->y, "y"), need(a->w, "w"), need(a->eta, "eta"), need(a->resid, "resid");
        break;
    case ADELIE_HIP_GLM_PIECE_LOSS:
        need(a->y, "y"), need(a->w, "w"), need(a->eta, "eta");
        break;
    case ADELIE_HIP_GLM_PIECE_LOSS2:
    case ADELIE_HIP_GLM_PIECE_MULTI_LOSS2:
        need(a->y, "y"), need(a->w, "w"), need(a->wb, "wb"), need(a->eta, "eta"), need(a->off, "off");
        if (mode == ADELIE_HIP_GLM_PIECE_MULTI_LOSS2) need(a->b0v, "b0v");
        break;
    case ADELIE_HIP_GLM_PIECE_SET_ETA:
        need(a->off, "off"), need(a->eta, "eta");
        break;
    case ADELIE_HIP_GLM_PIECE_DOT_DIFF:
        need(a->resid, "resid"), need(a->resid_prev, "resid_prev"), need(a->eta, "eta"), need(a->eta_prev, "eta_prev");
        break;
    case ADELIE_HIP_GLM_PIECE_REL_CHANGE:
        need(a->wts, "wts"), need(a->prev, "prev");
        break;
    default: break;
    }
    AHIP_CHECK(hipSetDevice(0));
    hipStream_t s = nullptr;
    Stage st{s};
    for (int q = 0; q < 8; ++q) info[q] = 0;
    auto body = [&](auto tag) {
        using T = decltype(tag);
        DevBuf<T> dy, dw, dwb, deta, dresid, doff, dhess, dir, diy, dwts, dz, db0v, drp, dep, dprev, dsrc, ddst, dsums;
        DevBuf<int32_t> didx;
        // an array of `len` values on the device, or no array where the caller gave none
        auto put = [&](DevBuf<T>& buf, const void* h, int64_t len) -> T* {
            if (!h) return nullptr;
            st.up(buf, static_cast<const T*>(h), len);
            return buf.p;
        };
        if (moves) {
            const bool gather = mode == ADELIE_HIP_GLM_PIECE_GATHER;
            const int64_t ns = gather ? a->src_elems : std::max<int64_t>(cnt, 1), nd = gather ? std::max<int64_t>(cnt, 1) : a->dst_elems;
            const int64_t ups = gather ? a->src_elems : cnt, upd = gather ? cnt : a->dst_elems;
            dsrc.reserve(size_t(ns)); ddst.reserve(size_t(nd)); didx.reserve(size_t(std::max<int64_t>(cnt, 1)));
            if (ups > 0) dsrc.upload(static_cast<const T*>(a->src), size_t(ups), s);
            if (upd > 0) ddst.upload(static_cast<const T*>(a->dst), size_t(upd), s);
            if (cnt > 0) didx.upload(a->idx, size_t(cnt), s);
            if (gather) launch_gather<T>(dsrc.p, didx.p, cnt, ddst.p, s);
            else launch_scatter<T>(dsrc.p, didx.p, cnt, ddst.p, s);
            info[0] = 1;
            AHIP_CHECK(hipGetLastError());
            if (upd > 0) st.fetch(a->dst, ddst.p, size_t(upd) * sizeof(T));
            st.land();
            return;
        }
        const std::vector<T> hs(size_t(SUMS), T(a->sentinel));
        st.up(dsums, hs.data(), SUMS);
        T* sums = dsums.p;
        const int64_t nw = mode == ADELIE_HIP_GLM_PIECE_MULTI_LOSS2 ? nb : n; // (MULTI_LOSS2: one weight per observation)
        const T* y = put(dy, a->y, n);
        const T* w = put(dw, a->w, nw);
        const T* wb = put(dwb, a->wb, nw);
        T* eta = put(deta, a->eta, n);
        T* resid = put(dresid, a->resid, n);
        const T* off = put(doff, a->off, n);
        T* hess = put(dhess, a->hess, n);
        T* ir = put(dir, a->irls_resid, n);
        T* iy = put(diy, a->irls_y, n);
        T* wts = put(dwts, a->wts, n);
        const T* z = put(dz, a->cb_z, n);
        const T* b0v = put(db0v, a->b0v, std::max<int64_t>(K, 1));
        const T* rp = put(drp, a->resid_prev, n);
        const T* ep = put(dep, a->eta_prev, n);
        T* prev = put(dprev, a->prev, n);
        auto back = [&](void* h, const T* dev, int64_t len) { st.fetch(h, dev, size_t(len) * sizeof(T)); };
        const int Ki = int(std::max<int64_t>(K, 1));
        switch (mode) {
        case ADELIE_HIP_GLM_PIECE_PREPARE:
            launch_irls_prepare<T>(kind, y, w, eta, resid, off, T(a->hmin), n, hess, ir, iy, sums, s, Ki);
            AHIP_CHECK(hipGetLastError());
            back(a->hess, hess, n), back(a->irls_resid, ir, n), back(a->irls_y, iy, n);
            break;
        case ADELIE_HIP_GLM_PIECE_WEIGHTS:
            launch_irls_weights<T>(hess, T(a->hess_sum), iy, T(a->shift), n, wts, ir, sums, s);
            AHIP_CHECK(hipGetLastError());
            back(a->wts, wts, n), back(a->irls_resid, ir, n);
            break;
        case ADELIE_HIP_GLM_PIECE_FINISH:
            launch_irls_finish<T>(kind, y, w, iy, off, ir, T(a->shift), n, eta, resid, sums, s, Ki);
            AHIP_CHECK(hipGetLastError());
            back(a->eta, eta, n), back(a->resid, resid, n);
            break;
        case ADELIE_HIP_GLM_PIECE_NULL_STEP:
            launch_null_step<T>(kind, y, w, eta, resid, off, T(a->hmin), n, sums, s, Ki, hess, z);
            break;
        case ADELIE_HIP_GLM_PIECE_GRADIENT:
            launch_glm_gradient<T>(kind, y, w, eta, n, resid, s, Ki);
            AHIP_CHECK(hipGetLastError());
            back(a->resid, resid, n);
            break;
        case ADELIE_HIP_GLM_PIECE_LOSS:
            launch_glm_loss<T>(kind, y, w, eta, n, sums, s, Ki);
            break;
        case ADELIE_HIP_GLM_PIECE_LOSS2:
            launch_glm_loss2<T>(kind, y, w, wb, eta, T(a->b0), off, n, sums, s);
            break;
        case ADELIE_HIP_GLM_PIECE_MULTI_LOSS2:
            launch_multi_loss2<T>(kind, y, w, wb, eta, b0v, off, nb, Ki, sums, s);
            break;
        case ADELIE_HIP_GLM_PIECE_SET_ETA:
            launch_set_eta<T>(off, T(a->b0), n, eta, s);
            AHIP_CHECK(hipGetLastError());
            back(a->eta, eta, n);
            break;
        case ADELIE_HIP_GLM_PIECE_DOT_DIFF:
            launch_dot_diff<T>(resid, rp, eta, ep, n, sums, s);
            break;
        default: // REL_CHANGE
            launch_rel_change<T>(wts, prev, n, sums + 15, s);
            AHIP_CHECK(hipGetLastError());
            back(a->prev, prev, n);
            break;
        }
        info[0] = 1;
        AHIP_CHECK(hipGetLastError());
        if (reduces) back(a->sums, sums, 16);
        st.land();
    };
    DTYPE_DISPATCH(a, body(T{}))
    ABI_CATCH
}

// One of the two places where the path solver touches the covariance matrix A, through the dispatcher the solver calls
// (design_ops.hpp: raw_cov_gather / raw_cov_grad), on either storage (include/adelie_hip.h has the arguments).
int adelie_hip_cov_piece_test(adelie_hip_design* A, int what, const int32_t* vcol, int64_t nv, int64_t pos0, int64_t N, int64_t ldc,
                              double sentinel, const void* v, const int32_t* cols, const void* coef, int64_t count, void* out) {
    ABI_TRY
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
    const Stage st{s};
    auto body = [&](auto tag) {
        using T = decltype(tag);
        DevBuf<int32_t> dlist, dpos, dcnt;
        dlist.reserve(size_t(n_list) + 1);
        if (n_list) AHIP_CHECK(hipMemcpyAsync(dlist.p, list, size_t(n_list) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (gather) {
            DevBuf<T> dC;
            std::vector<T> hC(size_t(ldc) * size_t(nv), T(sentinel));
            dpos.reserve(size_t(p));
            st.up(dC, hC.data(), int64_t(hC.size()));
            if (pos0 > 0) raw_cov_gather<T>(*A, dlist.p, int32_t(pos0), 0, int32_t(pos0), dC.p, ldc, dpos.p, s);
            raw_cov_gather<T>(*A, dlist.p, int32_t(nv), int32_t(pos0), int32_t(N), dC.p, ldc, dpos.p, s);
            AHIP_CHECK(hipGetLastError());
            st.down(out, dC.p, hC.size() * sizeof(T));
            st.sync();
        } else {
            DevBuf<T> dv, dcoef, dgrad, dw;
            dcoef.reserve(size_t(count) + 1); dgrad.reserve(size_t(p)); dw.reserve(size_t(p));
            const int32_t c32 = int32_t(count);
            st.up(dv, static_cast<const T*>(v), p);
            if (count) AHIP_CHECK(hipMemcpyAsync(dcoef.p, coef, size_t(count) * sizeof(T), hipMemcpyHostToDevice, s));
            st.up(dcnt, &c32, 1);
            raw_cov_grad<T>(*A, dv.p, dlist.p, dcoef.p, dcnt.p, count, dgrad.p, dw.p, s);
            AHIP_CHECK(hipGetLastError());
            st.down(out, dgrad.p, size_t(p) * sizeof(T));
            st.sync();
        }
    };
    DTYPE_DISPATCH(A, body(T{}))
    ABI_CATCH
}

} // extern "C"
