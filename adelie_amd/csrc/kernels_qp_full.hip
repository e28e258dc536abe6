// kernels_qp_full.hip — full-matrix NNQP, lasso and pinball descents, a batch per call (adelie.optimization.StateNNQPFull /
// StateLassoFull / StatePinballFull: nnqp_full.hpp, lasso_full.hpp, pinball_full.hpp).  The C-ABI entry point
// adelie_hip_qp_full_solve and its host driver; the rules and the two kernels: qp_full_body.hpp.
//
// One call: every host vector and every small host matrix of the batch is packed into one block and uploaded in one copy
// (a matrix of a MiB or more goes up from the caller's memory directly; a matrix already on the device is read in place), the
// problems with d <= 64 run in one launch of the wave form, those with d > 64 in one launch of the block form (a second one when
// some of them keep their state in global memory), all on one stream, and x, grad and the (iters, status) reports come back in one
// copy.  Problems are independent: a workgroup reads and writes its own problem only.
#include "qp_full_body.hpp"

namespace ahip {

int64_t g_qp_full_lds_max_d = 0; // adelie_hip_set_config("qp_full_lds_max_d", x): 0 = automatic

namespace {

constexpr size_t kQpDirectBytes = size_t(1) << 20; // a host matrix from this size on is not packed

inline size_t qp_align(size_t b) { return (b + 63) & ~size_t(63); }

// synchronises the stream and hands it back before the buffers declared in front of it are parked
struct QpStream {
    hipStream_t s = StreamPool::take();
    ~QpStream() {
        (void)hipStreamSynchronize(s);
        StreamPool::give(s);
    }
};

template <class T, class Rule>
void qp_full_launch(const QpFullProb* tab, const int32_t* list, const std::vector<int32_t>& wave,
                    const std::vector<int32_t>& blk_lds, const std::vector<int32_t>& blk_glb, int max_d_lds, int max_d_glb,
                    int lds_limit, hipStream_t s) {
    auto threads_for = [](int max_d) { return unsigned(std::min(kQpBlockThreads, (max_d + 63) / 64 * 64)); };
    if (!wave.empty())
        hipLaunchKernelGGL((qp_full_wave_kernel<T, Rule>), dim3(unsigned(wave.size())), dim3(kQpWave), 0, s, tab, list);
    if (!blk_lds.empty()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(qp_full_block_kernel<T, true, Rule>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds_limit);
        (void)hipGetLastError();
        hipLaunchKernelGGL((qp_full_block_kernel<T, true, Rule>), dim3(unsigned(blk_lds.size())), dim3(threads_for(max_d_lds)),
                           qp_block_state_bytes<T>(max_d_lds), s, tab, list + wave.size());
    }
    if (!blk_glb.empty())
        hipLaunchKernelGGL((qp_full_block_kernel<T, false, Rule>), dim3(unsigned(blk_glb.size())), dim3(threads_for(max_d_glb)), 0,
                           s, tab, list + wave.size() + blk_lds.size());
    AHIP_CHECK(hipGetLastError());
}

template <class T>
void qp_full_run(const adelie_hip_qp_full_args* a) {
    const int64_t n = a->n_problems;
    const int kind = a->kind;
    AHIP_CHECK(hipSetDevice(a->device));
    int lds_limit = 0;
    if (hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, a->device) != hipSuccess || lds_limit <= 0) {
        (void)hipGetLastError();
        lds_limit = 65536;
    }
    const int64_t lds_max_d = g_qp_full_lds_max_d;

    // the three launch lists and the layout of the packed block, the direct matrices and the global state
    std::vector<int32_t> wave, blk_lds, blk_glb;
    int max_d_lds = 0, max_d_glb = 0;
    struct Slot { size_t q, pa, pb, x, g, scratch; bool q_packed, q_direct; };
    std::vector<Slot> slot(static_cast<size_t>(n));
    const bool has_pa = kind != ADELIE_HIP_QP_FULL_NNQP, has_pb = kind == ADELIE_HIP_QP_FULL_PINBALL;
    size_t in_bytes = qp_align(size_t(n) * sizeof(QpFullProb)) + qp_align(size_t(n) * sizeof(int32_t));
    size_t direct_bytes = 0, scratch_bytes = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t d = a->d[k];
        const size_t vec = qp_align(size_t(d) * sizeof(T)), mat = qp_align(size_t(d) * size_t(d) * sizeof(T));
        Slot& sl = slot[size_t(k)];
        const bool dev = a->quad_is_dev && a->quad_is_dev[k];
        sl.q_direct = !dev && mat >= kQpDirectBytes;
        sl.q_packed = !dev && !sl.q_direct;
        if (sl.q_packed) sl.q = in_bytes, in_bytes += mat;
        if (sl.q_direct) sl.q = direct_bytes, direct_bytes += mat;
        if (has_pa) sl.pa = in_bytes, in_bytes += vec;
        if (has_pb) sl.pb = in_bytes, in_bytes += vec;
        sl.scratch = 0;
        if (d <= kQpWave) wave.push_back(int32_t(k));
        else if (qp_block_state_bytes<T>(d) + 256 <= size_t(lds_limit) && (lds_max_d <= 0 || d < lds_max_d)) {
            blk_lds.push_back(int32_t(k));
            max_d_lds = std::max(max_d_lds, int(d));
        } else {
            blk_glb.push_back(int32_t(k));
            max_d_glb = std::max(max_d_glb, int(d));
            sl.scratch = scratch_bytes, scratch_bytes += qp_align(qp_block_state_bytes<T>(d));
        }
    }
    // what comes back: x and grad of every problem, then the reports
    const size_t out_begin = in_bytes;
    size_t total = in_bytes;
    for (int64_t k = 0; k < n; ++k) {
        const size_t vec = qp_align(size_t(a->d[k]) * sizeof(T));
        slot[size_t(k)].x = total, total += vec;
        slot[size_t(k)].g = total, total += vec;
    }
    const size_t report_at = total;
    total += qp_align(size_t(n) * 2 * sizeof(int64_t));

    DevBuf<char> d_pack, d_direct, d_scratch;
    QpStream qs;
    hipStream_t s = qs.s;
    d_pack.reserve(total);
    if (direct_bytes) d_direct.reserve(direct_bytes);
    if (scratch_bytes) d_scratch.reserve(scratch_bytes);

    std::vector<char> h(total);
    QpFullProb* tab = reinterpret_cast<QpFullProb*>(h.data());
    int32_t* list = reinterpret_cast<int32_t*>(h.data() + qp_align(size_t(n) * sizeof(QpFullProb)));
    {
        int32_t* w = list;
        for (const auto* v : {&wave, &blk_lds, &blk_glb})
            for (int32_t k : *v) *w++ = k;
    }
    for (int64_t k = 0; k < n; ++k) {
        const int64_t d = a->d[k];
        const Slot& sl = slot[size_t(k)];
        const size_t vb = size_t(d) * sizeof(T), mb = size_t(d) * size_t(d) * sizeof(T);
        QpFullProb& P = tab[k];
        P = QpFullProb{};
        if (sl.q_packed) {
            if (mb) std::memcpy(h.data() + sl.q, a->quad[k], mb);
            P.Q = d_pack.p + sl.q;
        } else if (sl.q_direct) {
            AHIP_CHECK(hipMemcpyAsync(d_direct.p + sl.q, a->quad[k], mb, hipMemcpyHostToDevice, s));
            P.Q = d_direct.p + sl.q;
        } else {
            P.Q = a->quad[k];
        }
        if (has_pa) {
            if (vb) std::memcpy(h.data() + sl.pa, a->penalty_a[k], vb);
            P.pa = d_pack.p + sl.pa;
        }
        if (has_pb) {
            if (vb) std::memcpy(h.data() + sl.pb, a->penalty_b[k], vb);
            P.pb = d_pack.p + sl.pb;
        }
        if (vb) {
            std::memcpy(h.data() + sl.x, a->x[k], vb);
            std::memcpy(h.data() + sl.g, a->grad[k], vb);
        }
        P.x = d_pack.p + sl.x;
        P.g = d_pack.p + sl.g;
        P.scratch = d_scratch.p ? d_scratch.p + sl.scratch : nullptr;
        P.report = reinterpret_cast<int64_t*>(d_pack.p + report_at) + 2 * k;
        // the threshold of a sweep, formed in the value type: nnqp_full.hpp:93, lasso_full.hpp:101, pinball_full.hpp:114
        const T tol = T(a->tol[k]);
        const T thr = kind == ADELIE_HIP_QP_FULL_NNQP ? T(d) * tol : (kind == ADELIE_HIP_QP_FULL_LASSO ? tol : T(a->y_var[k]) * tol);
        P.thr = double(thr);
        P.max_iters = a->max_iters[k];
        P.d = int32_t(d);
    }
    // (x, grad and the report slots go up as well: the report slots are overwritten by every problem)
    d_pack.upload(h.data(), total, s);

    const QpFullProb* d_tab = reinterpret_cast<const QpFullProb*>(d_pack.p);
    const int32_t* d_list = reinterpret_cast<const int32_t*>(d_pack.p + qp_align(size_t(n) * sizeof(QpFullProb)));
    if (kind == ADELIE_HIP_QP_FULL_NNQP)
        qp_full_launch<T, NnqpFullRule<T>>(d_tab, d_list, wave, blk_lds, blk_glb, max_d_lds, max_d_glb, lds_limit, s);
    else if (kind == ADELIE_HIP_QP_FULL_LASSO)
        qp_full_launch<T, LassoFullRule<T>>(d_tab, d_list, wave, blk_lds, blk_glb, max_d_lds, max_d_glb, lds_limit, s);
    else
        qp_full_launch<T, PinballFullRule<T>>(d_tab, d_list, wave, blk_lds, blk_glb, max_d_lds, max_d_glb, lds_limit, s);

    d_pack.download(h.data() + out_begin, total - out_begin, s, out_begin);
    AHIP_CHECK(hipStreamSynchronize(s));
    for (int64_t k = 0; k < n; ++k) {
        const Slot& sl = slot[size_t(k)];
        const size_t vb = size_t(a->d[k]) * sizeof(T);
        if (vb) {
            std::memcpy(a->x[k], h.data() + sl.x, vb);
            std::memcpy(a->grad[k], h.data() + sl.g, vb);
        }
        const int64_t* rep = reinterpret_cast<const int64_t*>(h.data() + report_at) + 2 * k;
        a->iters[k] = rep[0];
        a->status[k] = int32_t(rep[1]);
    }
}

} // namespace
} // namespace ahip

using namespace ahip;

extern "C" int adelie_hip_qp_full_solve(const adelie_hip_qp_full_args* a) {
    ABI_TRY
    const auto t0 = std::chrono::steady_clock::now();
    if (!a) throw make_core_error("null argument.");
    if (a->kind != ADELIE_HIP_QP_FULL_NNQP && a->kind != ADELIE_HIP_QP_FULL_LASSO && a->kind != ADELIE_HIP_QP_FULL_PINBALL)
        throw make_core_error("qp_full: unknown kind.");
    if (a->dtype != ADELIE_HIP_F32 && a->dtype != ADELIE_HIP_F64) throw make_core_error("qp_full: bad dtype.");
    const int64_t n = a->n_problems;
    if (n < 0 || n >= (int64_t(1) << 31)) throw make_core_error("qp_full: n_problems must be in [0, 2^31).");
    if (n > 0) {
        if (!a->d || !a->quad || !a->x || !a->grad || !a->tol || !a->max_iters || !a->iters || !a->status ||
            (a->kind != ADELIE_HIP_QP_FULL_NNQP && !a->penalty_a) || (a->kind == ADELIE_HIP_QP_FULL_PINBALL && (!a->penalty_b || !a->y_var)))
            throw make_core_error("null argument.");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess) {
            (void)hipGetLastError();
            count = 0;
        }
        if (a->device < 0 || a->device >= count) throw make_core_error("qp_full: no such device (adelie_amd has no CPU fallback).");
        for (int64_t k = 0; k < n; ++k) {
            const int64_t d = a->d[k];
            if (d < 0 || d > (int64_t(1) << 20)) throw make_core_error("qp_full: d must be in [0, 2^20].");
            if (a->tol[k] < 0) throw make_solver_error("tol must be >= 0.");
            if (a->max_iters[k] < 0) throw make_core_error("qp_full: max_iters must be >= 0.");
            if (d > 0 && (!a->quad[k] || !a->x[k] || !a->grad[k] || (a->kind != ADELIE_HIP_QP_FULL_NNQP && !a->penalty_a[k]) ||
                          (a->kind == ADELIE_HIP_QP_FULL_PINBALL && !a->penalty_b[k])))
                throw make_core_error("null argument.");
        }
        DTYPE_DISPATCH(a, qp_full_run<T>(a))
    }
    if (a->time_elapsed) *a->time_elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ABI_CATCH
}
