// design.hip — C ABI: library info, design-matrix handles and the MatrixNaiveBase operations.
// (include/adelie_hip.h documents which reference method each entry point replaces.)
#include <atomic>
#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include "common.hpp"
#include "cox.hpp"
#include "design_ops.hpp"
#include "csc_build_host.hpp"
#include "cov_csc_host.hpp"
#include "cov_batch_host.hpp"
#include "phased_decode_host.hpp"
#include "snp_decode_host.hpp"

using namespace ahip;

namespace {

thread_local std::string g_last_error; // written by ahip::set_last_error (below), read by adelie_hip_last_error

template <class T>
T* scratch(DevBuf<char>& b, size_t n) {
    return reinterpret_cast<T*>(b.reserve((n ? n : 1) * sizeof(T)));
}

void set_device(const adelie_hip_design* d) { AHIP_CHECK(hipSetDevice(d->device)); }

void check_device(int device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
        throw make_core_error("no HIP device is visible: adelie_hip has no CPU fallback.");
    if (device < 0 || device >= cnt) throw make_core_error("device ordinal out of range.");
    AHIP_CHECK(hipSetDevice(device));
}

// a temporary device block, freed on every way out
using DevTmp = DevArr<void>;

std::string gib(double bytes) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.2f GiB", bytes / double(int64_t(1) << 30));
    return buf;
}

// The padded column-major (d->n, d->p) matrix of a design under construction: columns start 128/256-byte aligned (32 elements;
// kernels_relu.hip's steps never leave a column's padding), at least 16 bytes.  zero_all clears the array on d's stream, otherwise
// only the padding rows are cleared, so that vector loads past n never see NaN payloads.  With `what` (a constructor's name) a
// refusal names the size that did not fit.
template <class T>
T* alloc_dense(adelie_hip_design* d, bool zero_all, const char* what = nullptr) {
    constexpr int64_t kAlign = 32;
    static_assert(kAlign % kReluStep == 0, "the padded rows must cover the structured relu sweep's last step");
    const int64_t n = d->n, p = d->p, ld = ((n + kAlign - 1) / kAlign) * kAlign;
    const size_t bytes = size_t(ld) * size_t(p) * sizeof(T);
    if (!what) d->X.alloc(std::max<size_t>(16, bytes));
    else if (!d->X.try_alloc(std::max<size_t>(16, bytes)))
        throw make_core_error(std::string(what) + "(): could not allocate the expanded design (" + std::to_string(n) + " x " +
                              std::to_string(p) + ", " + gib(double(ld) * double(p) * sizeof(T)) + ") on the device.");
    d->ld = ld;
    d->kind = adelie_hip_design::kDense;
    T* X = static_cast<T*>(d->X);
    if (zero_all) AHIP_CHECK(hipMemsetAsync(X, 0, bytes, d->stream));
    else if (ld > n && p > 0) AHIP_CHECK(hipMemset2DAsync(X + n, size_t(ld) * sizeof(T), 0, size_t(ld - n) * sizeof(T), size_t(p), d->stream));
    return X;
}
// the same for a 2-bit design: kind, the leading dimension of the 2-bit columns and the packed matrix itself; the (p,) imputed means
void snp_alloc_bits(adelie_hip_design* d) {
    d->kind = adelie_hip_design::kSnp;
    d->ldb = (((d->n + 3) / 4 + 127) / 128) * 128;
    d->bits.alloc(size_t(d->ldb) * size_t(d->p));
}
void snp_alloc_impute(adelie_hip_design* d) { d->impute.alloc(size_t(d->p) * (d->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float))); }

template <class T>
void create_dense_t(adelie_hip_design* d, const void* src, bool src_on_device, int order) {
    const int64_t n = d->n, p = d->p;
    if (src_on_device && order == ADELIE_HIP_COL_MAJOR) { // adopted in place: the caller frees it
        d->X.borrow(const_cast<void*>(src));
        d->ld = n;
        return;
    }
    T* X = alloc_dense<T>(d, order != ADELIE_HIP_COL_MAJOR);
    const int64_t ld = d->ld;
    if (order == ADELIE_HIP_COL_MAJOR) {
        AHIP_CHECK(hipMemcpy2DAsync(X, size_t(ld) * sizeof(T), src, size_t(n) * sizeof(T), size_t(n) * sizeof(T), size_t(p),
                                    hipMemcpyHostToDevice, d->stream));
    } else {
        // row-major source: stage (if on host) and transpose on device
        const T* rsrc = static_cast<const T*>(src);
        DevTmp tmp;
        if (!src_on_device) {
            tmp.alloc(size_t(n) * size_t(p) * sizeof(T));
            AHIP_CHECK(hipMemcpyAsync(tmp, src, size_t(n) * size_t(p) * sizeof(T), hipMemcpyHostToDevice, d->stream));
            rsrc = static_cast<const T*>(tmp);
        }
        launch_transpose<T>(rsrc, n, p, X, ld, d->stream);
        AHIP_CHECK(hipStreamSynchronize(d->stream));
    }
    AHIP_CHECK(hipStreamSynchronize(d->stream));
}

template <class T>
void create_sparse_t(adelie_hip_design* d, const int64_t* indptr, const int32_t* indices, const void* values) {
    const int64_t n = d->n, p = d->p;
    const int64_t nnz = indptr[p];
    T* X = alloc_dense<T>(d, true);
    const size_t nz1 = size_t(std::max<int64_t>(nnz, 1));
    DevArr<int64_t> dptr;
    DevArr<int32_t> didx;
    DevArr<T> dval;
    dptr.alloc(size_t(p + 1)), didx.alloc(nz1), dval.alloc(nz1);
    AHIP_CHECK(hipMemcpyAsync(dptr, indptr, size_t(p + 1) * sizeof(int64_t), hipMemcpyHostToDevice, d->stream));
    AHIP_CHECK(hipMemcpyAsync(didx, indices, size_t(nnz) * sizeof(int32_t), hipMemcpyHostToDevice, d->stream));
    AHIP_CHECK(hipMemcpyAsync(dval, values, size_t(nnz) * sizeof(T), hipMemcpyHostToDevice, d->stream));
    launch_csc_scatter<T>(dptr, didx, dval, n, p, X, d->ld, d->stream);
    AHIP_CHECK(hipStreamSynchronize(d->stream));
}

// Designs alive in this process.  When the last one goes, the device blocks that finished solves parked for re-use (DevPool,
// up to 6 GB) are released: nothing of this library keeps device memory that another library in the process might want once
// the caller holds no design any more.
std::atomic<int>& live_designs() { static std::atomic<int> c{0}; return c; }

adelie_hip_design* new_design(int64_t n, int64_t p, int dtype, int device) {
    if (n <= 0 || p <= 0) throw make_core_error("matrix must have positive dimensions.");
    if (dtype != ADELIE_HIP_F32 && dtype != ADELIE_HIP_F64) throw make_core_error("dtype must be F32 or F64.");
    if (p >= (int64_t(1) << 31)) throw make_core_error("number of columns must fit in int32.");
    check_device(device);
    auto* d = new adelie_hip_design();
    d->dtype = dtype;
    d->device = device;
    d->n = n;
    d->p = p;
    AHIP_CHECK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    live_designs().fetch_add(1);
    return d;
}

// Owns a design under construction: a create entry point that throws destroys what it has built so far, one that succeeds
// hands the design over with release().
struct DesignDeleter {
    void operator()(adelie_hip_design* d) const { adelie_hip_design_destroy(d); }
};
using DesignGuard = std::unique_ptr<adelie_hip_design, DesignDeleter>;

// ---- host-vector matrix operations ----------------------------------------------------------------------
// (cols_host: the sweep over a column list, adelie_hip_design_bmul_cols; c0 is 0 then)
template <class T>
void op_sweep(adelie_hip_design* d, int64_t c0, int64_t ncols, const T* v, const T* w, T* out, bool square,
              const int32_t* cols_host = nullptr) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t n = d->n;
    T* dv = scratch<T>(d->s_n1, n);
    T* dw = scratch<T>(d->s_n2, n);
    T* dout = scratch<T>(d->s_p1, ncols);
    int32_t* dcols = nullptr;
    if (cols_host) {
        dcols = scratch<int32_t>(d->s_idx1, ncols);
        AHIP_CHECK(hipMemcpyAsync(dcols, cols_host, ncols * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    const bool structured = raw_sweep_structured(*d, c0, ncols, dcols, square, SweepHooks::from_env());
    T* work = scratch<T>(d->s_work, size_t(raw_sweep_work_elems(*d, ncols, structured, c0)));
    AHIP_CHECK(hipMemcpyAsync(dv, v, n * sizeof(T), hipMemcpyHostToDevice, s));
    if (w) {
        AHIP_CHECK(hipMemcpyAsync(dw, w, n * sizeof(T), hipMemcpyHostToDevice, s));
        launch_vmul<T>(dv, dw, dv, n, s);
    }
    raw_sweep<T>(*d, dv, dout, c0, ncols, dcols, nullptr, nullptr, square, structured, work, s);
    AHIP_CHECK(hipMemcpyAsync(out, dout, ncols * sizeof(T), hipMemcpyDeviceToHost, s));
    AHIP_CHECK(hipStreamSynchronize(s));
}

// L sweeps at once (diagnostic.gradients, reference adelie/diagnostic.py:320-387: one X.mul per residual vector): the
// vectors go through the K-wide sweep eight at a time, so the design (dense or 2-bit SNP) is streamed once per eight vectors.
template <class T>
void op_mul_batch(adelie_hip_design* d, const T* V, int64_t L, T* out) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t n = d->n, p = d->p;
    constexpr int64_t KB = 8;
    // sparse: one pass over the stored entries per vector (a convex-relu design: over those of Z, by the hook); a design made of
    // pieces: one sweep per vector as well, every piece at its own rate (the K-wide kernels below take one dense or 2-bit view)
    if (d->is_csc() || d->is_pieces()) {
        T* dv1 = scratch<T>(d->s_n1, size_t(n));
        T* dout1 = scratch<T>(d->s_p1, size_t(p));
        const bool structured = raw_sweep_structured(*d, 0, p, nullptr, false, SweepHooks::from_env());
        T* work1 = scratch<T>(d->s_work, size_t(raw_sweep_work_elems(*d, p, structured)));
        for (int64_t l = 0; l < L; ++l) {
            AHIP_CHECK(hipMemcpyAsync(dv1, V + l * n, size_t(n) * sizeof(T), hipMemcpyHostToDevice, s));
            raw_sweep<T>(*d, dv1, dout1, 0, p, nullptr, nullptr, nullptr, false, structured, work1, s);
            AHIP_CHECK(hipMemcpyAsync(out + l * p, dout1, size_t(p) * sizeof(T), hipMemcpyDeviceToHost, s));
            AHIP_CHECK(hipStreamSynchronize(s));
        }
        return;
    }
    T* dv = scratch<T>(d->s_n1, size_t(KB) * size_t(n));
    T* dout = scratch<T>(d->s_p1, size_t(KB) * size_t(p));
    // one work buffer for both kernels (a lone last vector goes through the single-vector sweep); the K-wide sweep's
    // work size only depends on (n, p, K)
    const MultiView<T> shape{nullptr, n, p, n, nullptr, int32_t(KB), 0};
    T* work = scratch<T>(d->s_work, std::max<size_t>(size_t(raw_sweep_work_elems(*d, p, false)), size_t(multi_sweep_work_elems<T>(shape))));
    std::vector<T> hout(size_t(KB) * size_t(p));
    for (int64_t l0 = 0; l0 < L; l0 += KB) {
        const int64_t K = std::min(KB, L - l0);
        AHIP_CHECK(hipMemcpyAsync(dv, V + l0 * n, size_t(K) * size_t(n) * sizeof(T), hipMemcpyHostToDevice, s));
        if (K == 1) {
            raw_sweep<T>(*d, dv, dout, 0, p, nullptr, nullptr, nullptr, false, false, work, s);
            AHIP_CHECK(hipMemcpyAsync(out + l0 * p, dout, size_t(p) * sizeof(T), hipMemcpyDeviceToHost, s));
            AHIP_CHECK(hipStreamSynchronize(s));
            continue;
        }
        no_pieces(*d, "the K-wide sweep"); // (unreachable: taken above)
        if (d->is_dense()) {
            const DenseView<T> X = d->dense<T>();
            launch_multi_sweep<T>(MultiView<T>{X.X, n, p, X.ld, nullptr, int32_t(K), 0}, dv, dout, work, s);
        } else {
            launch_multi_sweep_snp<T>(d->snp(), snp_impute<T>(*d), int(K), dv, dout, work, s);
        }
        AHIP_CHECK(hipMemcpyAsync(hout.data(), dout, size_t(K) * size_t(p) * sizeof(T), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
        for (int64_t l = 0; l < K; ++l) {
            T* o = out + (l0 + l) * p;
            for (int64_t u = 0; u < p; ++u) o[u] = hout[size_t(u) * size_t(K) + size_t(l)];
        }
    }
}

// (cols_host: the q columns of adelie_hip_design_btmul_cols instead of j .. j + q - 1)
template <class T>
void op_axpy(adelie_hip_design* d, int64_t j, int64_t q, const T* coef, T* out, const int32_t* cols_host = nullptr) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t n = d->n;
    T* dout = scratch<T>(d->s_n1, n);
    T* dcoef = scratch<T>(d->s_p1, q);
    int32_t* dcols = scratch<int32_t>(d->s_idx1, q);
    std::vector<int32_t> cols(q);
    for (int64_t k = 0; k < q; ++k) cols[k] = cols_host ? cols_host[k] : int32_t(j + k);
    AHIP_CHECK(hipMemcpyAsync(dout, out, n * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dcoef, coef, q * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dcols, cols.data(), q * sizeof(int32_t), hipMemcpyHostToDevice, s));
    T* delta = nullptr;
    if (d->is_csc()) {
        delta = scratch<T>(d->s_misc, size_t(d->p) + 8);
        AHIP_CHECK(hipMemsetAsync(delta, 0, (size_t(d->p) + 8) * sizeof(T), s));
    }
    raw_axpy_cols<T>(*d, dcols, dcoef, nullptr, int32_t(q), T(1), dout, delta, s);
    AHIP_CHECK(hipMemcpyAsync(out, dout, n * sizeof(T), hipMemcpyDeviceToHost, s));
    AHIP_CHECK(hipStreamSynchronize(s));
}

template <class T>
void op_cov(adelie_hip_design* d, int64_t j, int64_t q, const T* sw, T* out) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t n = d->n;
    T* dw = scratch<T>(d->s_n1, n);
    T* dC = scratch<T>(d->s_p1, q * q);
    T* work = scratch<T>(d->s_work, size_t(raw_gram_work_elems(*d, n, q, q)));
    int32_t* dcols = scratch<int32_t>(d->s_idx1, q);
    std::vector<int32_t> cols(q);
    for (int64_t k = 0; k < q; ++k) cols[k] = int32_t(j + k);
    AHIP_CHECK(hipMemcpyAsync(dw, sw, n * sizeof(T), hipMemcpyHostToDevice, s));
    launch_vmul<T>(dw, dw, dw, n, s); // weights = sqrt_weights^2
    AHIP_CHECK(hipMemcpyAsync(dcols, cols.data(), q * sizeof(int32_t), hipMemcpyHostToDevice, s));
    raw_gram<T>(*d, dw, dcols, int32_t(q), 0, dcols, int32_t(q), 0, nullptr, false, dC, q, work, s);
    AHIP_CHECK(hipMemcpyAsync(out, dC, q * q * sizeof(T), hipMemcpyDeviceToHost, s));
    AHIP_CHECK(hipStreamSynchronize(s));
}

// A = X^T X in column panels of 2048 columns (the Gram kernel's K-split partials stay bounded); unit weights, no centring
template <class T>
static void cov_lazy_t(adelie_hip_design* X, adelie_hip_design* A) {
    constexpr int64_t PANEL = 2048;
    const int64_t n = X->n, p = X->p;
    hipStream_t s = A->stream;
    T* C = alloc_dense<T>(A, true);
    const int64_t ld = A->ld;
    DevBuf<T> ones, work;
    DevBuf<int32_t> cols;
    std::vector<T> h1(size_t(n), T(1));
    std::vector<int32_t> hc(static_cast<size_t>(p));
    for (int64_t j = 0; j < p; ++j) hc[size_t(j)] = int32_t(j);
    ones.reserve(size_t(n));
    cols.reserve(size_t(p));
    ones.upload(h1.data(), size_t(n), s);
    cols.upload(hc.data(), size_t(p), s);
    work.reserve(size_t(raw_gram_work_elems(*X, n, p, std::min<int64_t>(p, PANEL))));
    for (int64_t c0 = 0; c0 < p; c0 += PANEL) {
        const int64_t nc = std::min<int64_t>(PANEL, p - c0);
        raw_gram<T>(*X, ones.p, cols.p, int32_t(p), 0, cols.p + c0, int32_t(nc), int32_t(c0), nullptr, false, C, ld, work.p, s);
    }
    AHIP_CHECK(hipStreamSynchronize(s));
}

// The CSR operand of sp_tmul and the loss paths on the device: indptr (rows + 1) in s_idx1, indices in s_idx2, the values at the
// front of s_p1 with room for `extra` more elements behind them.
template <class T>
struct DevCsr {
    int64_t *ptr, *ind;
    T* val;
};
template <class T>
DevCsr<T> upload_csr(adelie_hip_design* d, int64_t rows, const int64_t* indptr, const int64_t* indices, const T* values,
                     size_t extra = 0) {
    hipStream_t s = d->stream;
    const int64_t nnz = indptr[rows];
    DevCsr<T> A{scratch<int64_t>(d->s_idx1, rows + 1), scratch<int64_t>(d->s_idx2, nnz), scratch<T>(d->s_p1, size_t(nnz) + extra)};
    AHIP_CHECK(hipMemcpyAsync(A.ptr, indptr, (rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (nnz) {
        AHIP_CHECK(hipMemcpyAsync(A.ind, indices, nnz * sizeof(int64_t), hipMemcpyHostToDevice, s));
        AHIP_CHECK(hipMemcpyAsync(A.val, values, nnz * sizeof(T), hipMemcpyHostToDevice, s));
    }
    return A;
}
// eta = V X^T for the L groups of K consecutive CSR rows each, a panel of at most ~1 GiB of eta (s_misc) at a time:
// per_panel(l0, lc, eta) follows the sp_tmul of groups [l0, l0 + lc) on the design's stream (the csc form works in s_work).
template <class T, class F>
void for_each_eta_panel(adelie_hip_design* d, const DevCsr<T>& A, int64_t L, int64_t K, F&& per_panel) {
    const int64_t len = d->n * K;
    const int64_t Lp = std::max<int64_t>(1, (int64_t(1) << 30) / int64_t(len * sizeof(T)));
    T* eta = scratch<T>(d->s_misc, size_t(std::min(Lp, L)) * len);
    const int64_t wn = raw_sp_tmul_work_elems(*d);
    T* work = wn ? scratch<T>(d->s_work, size_t(wn)) : nullptr;
    for (int64_t l0 = 0; l0 < L; l0 += Lp) {
        const int64_t lc = std::min(Lp, L - l0);
        raw_sp_tmul<T>(*d, lc * K, A.ptr + l0 * K, A.ind, A.val, eta, work, d->stream);
        per_panel(l0, lc, eta);
    }
}
// the (loss under wa, loss under wb) pairs of L fits, left on the device by the loss kernels -> out[0..L) and out[L..2L)
template <class T>
void download_loss_pairs(adelie_hip_design* d, const T* dres, int64_t L, double* out) {
    std::vector<T> res(size_t(2) * L);
    AHIP_CHECK(hipMemcpyAsync(res.data(), dres, res.size() * sizeof(T), hipMemcpyDeviceToHost, d->stream));
    AHIP_CHECK(hipStreamSynchronize(d->stream));
    for (int64_t l = 0; l < L; ++l) {
        out[l] = double(res[2 * l]);
        out[L + l] = double(res[2 * l + 1]);
    }
}

template <class T>
void op_sp_tmul(adelie_hip_design* d, int64_t L, const int64_t* indptr, const int64_t* indices, const T* values, T* out) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t n = d->n;
    const DevCsr<T> A = upload_csr<T>(d, L, indptr, indices, values);
    for_each_eta_panel<T>(d, A, L, 1, [&](int64_t l0, int64_t lc, const T* eta) {
        AHIP_CHECK(hipMemcpyAsync(out + l0 * n, eta, size_t(lc) * n * sizeof(T), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
    });
}

// Per-row losses of eta_l = X beta_l + intercepts[l] + offsets under two weight vectors, without moving eta to the host.
template <class T>
void op_path_losses(adelie_hip_design* d, int kind, int64_t L, const int64_t* indptr, const int64_t* indices,
                    const T* values, const T* intercepts, const T* offsets, const T* y, const T* wa, const T* wb,
                    double* out) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t n = d->n;
    const DevCsr<T> A = upload_csr<T>(d, L, indptr, indices, values);
    // n-vectors y, wa, wb, offsets and the reduction scratch share one buffer
    const size_t SUMS = 16 + 4 * 256;
    T* vec = scratch<T>(d->s_n1, size_t(4) * n + SUMS + size_t(2) * L);
    T *dy = vec, *dwa = vec + n, *dwb = vec + 2 * n, *doff = vec + 3 * n, *sums = vec + 4 * n, *dres = sums + SUMS;
    AHIP_CHECK(hipMemcpyAsync(dy, y, n * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dwa, wa, n * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dwb, wb, n * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(doff, offsets, n * sizeof(T), hipMemcpyHostToDevice, s));
    for_each_eta_panel<T>(d, A, L, 1, [&](int64_t l0, int64_t lc, const T* eta) {
        for (int64_t l = 0; l < lc; ++l) {
            launch_glm_loss2<T>(kind, dy, dwa, dwb, eta + l * n, intercepts[l0 + l], doff, n, sums, s);
            AHIP_CHECK(hipMemcpyAsync(dres + 2 * (l0 + l), sums, 2 * sizeof(T), hipMemcpyDeviceToDevice, s));
        }
    });
    download_loss_pairs<T>(d, dres, L, out);
}

// The same for multi-response fits on the base design `d`: row l of the CSR is a coefficient vector over the view columns
// (feature*K + response, intercept columns already split off), intercepts (L, K), offsets / y (n, K) row-major.  Each row is
// split into its K per-response rows over the base features, so that one sp_tmul yields eta_l response-major.
template <class T>
void op_multi_path_losses(adelie_hip_design* d, int kind, int K, int64_t L, const int64_t* indptr, const int64_t* indices,
                          const T* values, const T* intercepts, const T* offsets, const T* y, const T* wa, const T* wb,
                          double* out) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t n = d->n, p = d->p;
    const int64_t nnz = indptr[L];
    // per-response CSR rows (counting sort by response inside every row; the order of the features is kept)
    const size_t nz = size_t(nnz);
    std::vector<int64_t> ptr(size_t(L) * K + 1, 0), ind(nz);
    std::vector<T> val(nz);
    for (int64_t l = 0; l < L; ++l)
        for (int64_t e = indptr[l]; e < indptr[l + 1]; ++e) {
            if (indices[e] < 0 || indices[e] >= p * K) throw make_core_error("multi_path_losses: column index out of range.");
            ++ptr[size_t(l) * K + size_t(indices[e] % K) + 1];
        }
    for (size_t r = 0; r < size_t(L) * K; ++r) ptr[r + 1] += ptr[r];
    {
        std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
        for (int64_t l = 0; l < L; ++l)
            for (int64_t e = indptr[l]; e < indptr[l + 1]; ++e) {
                const size_t r = size_t(l) * K + size_t(indices[e] % K);
                ind[size_t(fill[r])] = indices[e] / K;
                val[size_t(fill[r])] = values[e];
                ++fill[r];
            }
    }
    // (n, K) row-major -> response-major
    std::vector<T> ym(size_t(n) * K), om(size_t(n) * K);
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < K; ++k) {
            ym[size_t(k) * n + i] = y[i * K + k];
            om[size_t(k) * n + i] = offsets[i * K + k];
        }
    const DevCsr<T> A = upload_csr<T>(d, L * K, ptr.data(), ind.data(), val.data(), size_t(L) * K); // (+ the intercepts)
    T* dicpt = A.val + nnz;
    AHIP_CHECK(hipMemcpyAsync(dicpt, intercepts, size_t(L) * K * sizeof(T), hipMemcpyHostToDevice, s));
    const size_t SUMS = 16 + 4 * 256;
    const size_t nK = size_t(n) * K;
    T* vec = scratch<T>(d->s_n1, 2 * nK + 2 * size_t(n) + SUMS + size_t(2) * L);
    T *dy = vec, *doff = vec + nK, *dwa = vec + 2 * nK, *dwb = dwa + n, *sums = dwb + n, *dres = sums + SUMS;
    AHIP_CHECK(hipMemcpyAsync(dy, ym.data(), nK * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(doff, om.data(), nK * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dwa, wa, n * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dwb, wb, n * sizeof(T), hipMemcpyHostToDevice, s));
    for_each_eta_panel<T>(d, A, L, K, [&](int64_t l0, int64_t lc, const T* eta) {
        for (int64_t l = 0; l < lc; ++l) {
            launch_multi_loss2<T>(kind, dy, dwa, dwb, eta + size_t(l) * nK, dicpt + (l0 + l) * K, doff, n, K, sums, s);
            AHIP_CHECK(hipMemcpyAsync(dres + 2 * (l0 + l), sums, 2 * sizeof(T), hipMemcpyDeviceToDevice, s));
        }
    });
    download_loss_pairs<T>(d, dres, L, out);
}

// The Cox losses of eta_l = X beta_l + intercepts[l] + offsets under two families over the same rows: the etas stay in their
// panel, cox_loss_batch evaluates them `mb` at a time (five launches per sub-batch, whatever its size).
template <class T>
void op_cox_path_losses(adelie_hip_design* d, const CoxPack& pa, const CoxPack& pb, int64_t L, const int64_t* indptr,
                        const int64_t* indices, const T* values, const T* intercepts, const T* offsets, int64_t max_batch,
                        double* out) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t n = d->n;
    for (int64_t e = indptr[0]; e < indptr[L]; ++e)
        if (indices[e] < 0 || indices[e] >= d->p) throw make_core_error("cox_path_losses: column index out of range.");
    // etas per cox_loss_batch call: as many as keep the Cox scratch within 1 GiB (the eta panel's own bound) unless told
    constexpr int64_t kMaxGridY = 65535;
    const int64_t fit = (int64_t(1) << 30) / int64_t(cox_loss_batch_scratch_doubles(n, 1) * sizeof(double));
    const int64_t mb = std::min(std::min(kMaxGridY, L), std::max<int64_t>(1, max_batch > 0 ? max_batch : fit));
    const DevCsr<T> A = upload_csr<T>(d, L, indptr, indices, values);
    // one buffer: the loss pairs and the Cox scratch (doubles), then the offsets and the intercepts
    const size_t nscr = cox_loss_batch_scratch_doubles(n, mb);
    const size_t tail = ((size_t(n) + size_t(L)) * sizeof(T) + sizeof(double) - 1) / sizeof(double);
    double* dres = scratch<double>(d->s_n1, size_t(2) * L + nscr + tail);
    double* scr = dres + size_t(2) * L;
    T* doff = reinterpret_cast<T*>(scr + nscr);
    T* db0 = doff + n;
    AHIP_CHECK(hipMemcpyAsync(doff, offsets, n * sizeof(T), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(db0, intercepts, L * sizeof(T), hipMemcpyHostToDevice, s));
    for_each_eta_panel<T>(d, A, L, 1, [&](int64_t l0, int64_t lc, const T* eta) {
        for (int64_t l = 0; l < lc; l += mb) {
            const int64_t c = std::min(mb, lc - l);
            cox_loss_batch<T>(pa, pb, eta + size_t(l) * size_t(n), db0 + l0 + l, doff, c, scr, dres + 2 * (l0 + l), s);
        }
    });
    download_loss_pairs<double>(d, dres, L, out);
}

// the multi-response view only serves grpnet_solve; its matrix ops go through the base design
void no_view(const adelie_hip_design* d) {
    if (d && d->is_std_view())
        throw make_core_error("the matrix operations of a standardized view over a dense or SNP design are composed by the caller "
                              "(adelie_amd.matrix); the handle only serves grpnet_solve.");
    if (d && d->is_multi()) throw multi_view_error();
    if (d && d->cov)
        throw make_core_error("this entry point takes a design matrix, not a covariance matrix (matrix.dense(method=\"cov\")).");
    if (d && d->constraint)
        throw make_core_error("this entry point takes a design matrix, not a constraint matrix (matrix.dense(method=\"constraint\")).");
}
void need_cov(const adelie_hip_design* d) {
    if (!d) throw make_core_error("null argument.");
    if (!d->cov) throw make_core_error("A must be a covariance matrix (matrix.dense(method=\"cov\")).");
}

void check_col(const adelie_hip_design* d, int64_t j, int64_t q, const char* what) {
    if (j < 0 || q < 0 || j + q > d->p) throw make_core_error(std::string(what) + "() is given inconsistent inputs!");
}

// ---- factor designs: one-hot / pairwise interactions of a resident table Z ---------------------------------------------------
// `blocks` describe the expanded design (col0 / ncols still unset); fills them in, allocates the expanded matrix, the copy of Z
// and the tables on Z's device, and runs the expansion kernel.  `what`: "one_hot" / "interaction" for the messages.
template <class T>
void create_factor_t(adelie_hip_design* Z, std::vector<FactorBlock>& blocks, const char* what, adelie_hip_design** out) {
    const int64_t n = Z->n, dz = Z->p;
    std::vector<int64_t> outer(blocks.size() + 1, 0);
    const double max_cols = double((int64_t(1) << 31) - 64);
    for (size_t b = 0; b < blocks.size(); ++b) {
        const double sz = double(blocks[b].l0) * double(blocks[b].l1) - double(blocks[b].shift);
        if (double(outer[b]) + sz > max_cols)
            throw make_core_error(std::string(what) + "(): the expanded design has more columns than the solver's 32-bit column "
                                  "indices address (" + gib((double(outer[b]) + sz) * double(n) * sizeof(T)) + " of values at least).");
        outer[b + 1] = outer[b] + int64_t(sz);
    }
    const int64_t P = outer.back();
    std::vector<FactorChunk> chunks;
    for (size_t b = 0; b < blocks.size(); ++b) {
        blocks[b].col0 = int32_t(outer[b]);
        blocks[b].ncols = int32_t(outer[b + 1] - outer[b]);
        for (int32_t t0 = 0; t0 < blocks[b].ncols; t0 += kFactorChunk)
            chunks.push_back(FactorChunk{int32_t(b), t0, std::min<int32_t>(kFactorChunk, blocks[b].ncols - t0), 0});
    }
    DesignGuard g(new_design(n, P, Z->dtype, Z->device));
    adelie_hip_design* d = g.get();
    hipStream_t s = d->stream;
    T* X = alloc_dense<T>(d, false, what); // (padding rows zeroed: vector loads past n never see NaN payloads)
    const int64_t ld = d->ld;
    d->fz.alloc(size_t(ld) * size_t(dz) * sizeof(T));
    T* fz = static_cast<T*>(d->fz);
    d->fz_ld = ld;
    d->fblk.alloc(blocks.size());
    d->fchunk.alloc(chunks.size());
    d->f_nchunk = int64_t(chunks.size());
    d->f_outer = outer;
    AHIP_CHECK(hipMemcpyAsync(d->fblk, blocks.data(), blocks.size() * sizeof(FactorBlock), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(d->fchunk, chunks.data(), chunks.size() * sizeof(FactorChunk), hipMemcpyHostToDevice, s));
    // copy Z (its padding rows zeroed too) and expand
    AHIP_CHECK(hipMemsetAsync(fz, 0, size_t(ld) * size_t(dz) * sizeof(T), s));
    AHIP_CHECK(hipStreamSynchronize(Z->stream)); // (Z's own creation may still be in flight on its stream)
    launch_derive_dense<T>(Z->dense<T>(), n, dz, nullptr, nullptr, nullptr, nullptr, fz, ld, s);
    launch_factor_expand<T>(d->factor_view<T>(), X, ld, s);
    AHIP_CHECK(hipStreamSynchronize(s)); // (the host tables above go out of scope)
    *out = g.release();
}

// The expanded (n, P) convex-relu design of Z and the host's column-major (n, m) mask bytes, with the copies of Z and of the
// mask that the structured sweep reads, on Z's device.
template <class T>
void create_relu_t(adelie_hip_design* Z, const uint8_t* mask, int64_t m, int gated, adelie_hip_design** out) {
    const int64_t n = Z->n, dz = Z->p;
    const double cols = double(gated ? 1 : 2) * double(m) * double(dz);
    if (cols > double((int64_t(1) << 31) - 64))
        throw make_core_error("convex_relu(): the expanded design has more columns than the solver's 32-bit column indices address (" +
                              gib(cols * double(n) * sizeof(T)) + " of values at least).");
    const int64_t P = int64_t(cols);
    DesignGuard g(new_design(n, P, Z->dtype, Z->device));
    adelie_hip_design* d = g.get();
    hipStream_t s = d->stream;
    T* X = alloc_dense<T>(d, false, "convex_relu"); // (padding rows zeroed: the sweep's vector loads run into them)
    const int64_t ld = d->ld;
    d->fz.alloc(std::max<size_t>(16, size_t(ld) * size_t(dz) * sizeof(T)));
    T* fz = static_cast<T*>(d->fz);
    d->fz_ld = ld;
    d->rmask.alloc(std::max<size_t>(16, size_t(ld) * size_t(m)));
    d->rmask_ld = ld;
    d->r_d = dz;
    d->r_m = m;
    d->r_gated = gated ? 1 : 0;
    // copy Z and the mask (their padding rows zeroed too) and expand
    AHIP_CHECK(hipMemsetAsync(fz, 0, size_t(ld) * size_t(dz) * sizeof(T), s));
    AHIP_CHECK(hipMemsetAsync(d->rmask, 0, size_t(ld) * size_t(m), s));
    if (n > 0 && m > 0)
        AHIP_CHECK(hipMemcpy2DAsync(d->rmask, size_t(ld), mask, size_t(n), size_t(n), size_t(m), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipStreamSynchronize(Z->stream)); // (Z's own creation may still be in flight on its stream)
    launch_derive_dense<T>(Z->dense<T>(), n, dz, nullptr, nullptr, nullptr, nullptr, fz, ld, s);
    launch_relu_expand<T>(d->relu_view<T>(), X, ld, s);
    AHIP_CHECK(hipStreamSynchronize(s)); // (the host's mask may go away)
    *out = g.release();
}

void check_factor_source(const adelie_hip_design* Z, const int64_t* levels, const void* out, const char* what) {
    if (!Z || !levels || !out) throw make_core_error("null argument.");
    if (!Z->is_dense() || Z->cov || Z->constraint || Z->std_center)
        throw make_core_error(std::string(what) + "(): mat must be a resident dense naive design (not an SNP, sparse, view or "
                              "covariance handle).");
    for (int64_t j = 0; j < Z->p; ++j)
        if (levels[j] > int64_t(0x7fffffff)) throw make_core_error(std::string(what) + "(): levels must fit in int32.");
}
// basis size and "discrete" flag of feature j
inline int32_t factor_basis(const int64_t* levels, int64_t j, bool& disc) {
    disc = levels[j] > 0;
    return disc ? int32_t(levels[j]) : 2;
}

template <class T>
void derive_t(adelie_hip_design* src, adelie_hip_design* d, const int64_t* rows, int64_t nrows, const int64_t* cols,
              int64_t ncols, const double* centers, const double* scales) {
    no_pieces(*src, "subset / standardize"); // (unreachable: adelie_hip_design_create_derived refuses it before allocating)
    const int64_t nout = d->n, pout = d->p;
    hipStream_t s = d->stream;
    int64_t *drows = nullptr, *dcols = nullptr;
    if (rows) {
        drows = scratch<int64_t>(d->s_idx1, size_t(nrows));
        AHIP_CHECK(hipMemcpyAsync(drows, rows, size_t(nrows) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    if (cols) {
        dcols = scratch<int64_t>(d->s_idx2, size_t(ncols));
        AHIP_CHECK(hipMemcpyAsync(dcols, cols, size_t(ncols) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    if (src->is_snp() && !centers && !scales) { // a subset of a 2-bit design stays 2 bits per call
        snp_alloc_bits(d);
        snp_alloc_impute(d);
        AHIP_CHECK(hipStreamSynchronize(src->stream));
        launch_snp_subset(src->snp(), nout, pout, drows, dcols, d->bits, d->ldb, s);
        launch_gather_cols<T>(snp_impute<T>(*src), dcols, pout, static_cast<T*>(d->impute), s);
        AHIP_CHECK(hipStreamSynchronize(s));
        return;
    }
    T* X = alloc_dense<T>(d, true);
    const int64_t ld = d->ld;
    T *dc = nullptr, *ds = nullptr;
    std::vector<T> hc, hs;
    if (centers) {
        hc.assign(centers, centers + pout);
        dc = scratch<T>(d->s_p1, size_t(pout));
        AHIP_CHECK(hipMemcpyAsync(dc, hc.data(), size_t(pout) * sizeof(T), hipMemcpyHostToDevice, s));
    }
    if (scales) {
        hs.assign(scales, scales + pout);
        ds = scratch<T>(d->s_misc, size_t(pout));
        AHIP_CHECK(hipMemcpyAsync(ds, hs.data(), size_t(pout) * sizeof(T), hipMemcpyHostToDevice, s));
    }
    // the source's stream may still be writing it (e.g. its own creation): order after it
    AHIP_CHECK(hipStreamSynchronize(src->stream));
    if (src->is_csc()) throw make_core_error("derived designs of a sparse design are composed on the host (adelie_amd.matrix).");
    if (src->is_dense()) launch_derive_dense<T>(src->dense<T>(), nout, pout, drows, dcols, dc, ds, X, ld, s);
    else launch_derive_dense_snp<T>(src->snp(), snp_impute<T>(*src), nout, pout, drows, dcols, dc, ds, X, ld, s);
    AHIP_CHECK(hipStreamSynchronize(s));
}
// concatenation of resident designs along the columns (axis 1) or the rows (axis 0): every source is copied (SNP sources
// decoded) into its slice of a new dense array
template <class T>
void concat_t(adelie_hip_design* const* srcs, int64_t k, int axis, adelie_hip_design* d) {
    for (int64_t m = 0; m < k; ++m) no_pieces(*srcs[m], "a further concatenate"); // (unreachable: refused at the entry point)
    hipStream_t s = d->stream;
    bool all_snp = axis == 1;
    for (int64_t m = 0; m < k && all_snp; ++m) all_snp = srcs[m]->is_snp() && !srcs[m]->std_center && srcs[m]->ldb == srcs[0]->ldb;
    if (all_snp) { // 2-bit designs side by side stay a 2-bit design: their columns are copied as they are
        snp_alloc_bits(d); // (ldb follows from n alone: the sources' own)
        snp_alloc_impute(d);
        int64_t off = 0;
        for (int64_t m = 0; m < k; ++m) {
            adelie_hip_design* src = srcs[m];
            AHIP_CHECK(hipStreamSynchronize(src->stream));
            AHIP_CHECK(hipMemcpyAsync(d->bits + off * d->ldb, src->bits, size_t(src->ldb) * size_t(src->p), hipMemcpyDeviceToDevice, s));
            AHIP_CHECK(hipMemcpyAsync(static_cast<T*>(d->impute) + off, src->impute, size_t(src->p) * sizeof(T), hipMemcpyDeviceToDevice, s));
            off += src->p;
        }
        AHIP_CHECK(hipStreamSynchronize(s));
        return;
    }
    T* X = alloc_dense<T>(d, true);
    const int64_t ld = d->ld;
    int64_t off = 0;
    for (int64_t m = 0; m < k; ++m) {
        adelie_hip_design* src = srcs[m];
        AHIP_CHECK(hipStreamSynchronize(src->stream));
        T* dst = axis == 1 ? X + off * ld : X + off;
        if (src->is_csc()) throw make_core_error("concatenations with a sparse design are composed on the host (adelie_amd.matrix).");
        if (src->is_dense()) launch_derive_dense<T>(src->dense<T>(), src->n, src->p, nullptr, nullptr, nullptr, nullptr, dst, ld, s);
        else launch_derive_dense_snp<T>(src->snp(), snp_impute<T>(*src), src->n, src->p, nullptr, nullptr,
                                        nullptr, nullptr, dst, ld, s);
        off += axis == 1 ? src->p : src->n;
    }
    AHIP_CHECK(hipStreamSynchronize(s));
}
} // namespace

void adelie_hip_internal_free_batcher(void* b); // solver.hip
void adelie_hip_internal_batch_stats(void* b, double* out);

namespace {
// A matrix kept sparse (kernels_cov_sparse.hip): the dense (p,) vector its column dots read, values[i] summed at indices[i] on
// the host (an index that repeats adds up, as in the dense kernels) and uploaded into s_work.  Not a hot path.
template <class T>
const T* cov_csc_upload_w(adelie_hip_design* d, const int64_t* indices, const T* values, int64_t ni) {
    std::vector<T> w(size_t(d->p), T(0));
    for (int64_t k = 0; k < ni; ++k) w[size_t(indices[k])] += values[k];
    T* dw = scratch<T>(d->s_work, size_t(d->p));
    AHIP_CHECK(hipMemcpyAsync(dw, w.data(), size_t(d->p) * sizeof(T), hipMemcpyHostToDevice, d->stream));
    AHIP_CHECK(hipStreamSynchronize(d->stream)); // (w goes out of scope)
    return dw;
}
template <class T>
void op_cov_bmul(adelie_hip_design* d, const int64_t* subset, int64_t ns, const int64_t* indices, const T* values, int64_t ni,
                 T* out) {
    set_device(d);
    hipStream_t s = d->stream;
    int64_t* dsub = scratch<int64_t>(d->s_idx1, ns + 1);
    int64_t* dind = scratch<int64_t>(d->s_idx2, ni + 1);
    T* dval = scratch<T>(d->s_n1, ni + 1);
    T* dout = scratch<T>(d->s_p1, ns + 1);
    AHIP_CHECK(hipMemcpyAsync(dsub, subset, size_t(ns) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dind, indices, size_t(ni) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dval, values, size_t(ni) * sizeof(T), hipMemcpyHostToDevice, s));
    if (d->cov_csc()) launch_cov_csc_coldot<T>(d->cov_csc_view<T>(), dsub, ns, cov_csc_upload_w<T>(d, indices, values, ni), nullptr, dout, s);
    else launch_cov_bmul<T>(static_cast<const T*>(d->X), d->ld, d->cov == 2, dsub, ns, dind, dval, ni, dout, s);
    AHIP_CHECK(hipMemcpyAsync(out, dout, size_t(ns) * sizeof(T), hipMemcpyDeviceToHost, s));
    AHIP_CHECK(hipStreamSynchronize(s));
}
template <class T>
void op_cov_mul(adelie_hip_design* d, const int64_t* indices, const T* values, int64_t ni, T* out) {
    set_device(d);
    hipStream_t s = d->stream;
    int64_t* dind = scratch<int64_t>(d->s_idx2, ni + 1);
    T* dval = scratch<T>(d->s_n1, ni + 1);
    T* dout = scratch<T>(d->s_p1, d->p);
    AHIP_CHECK(hipMemcpyAsync(dind, indices, size_t(ni) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(dval, values, size_t(ni) * sizeof(T), hipMemcpyHostToDevice, s));
    if (d->cov_csc()) launch_cov_csc_coldot<T>(d->cov_csc_view<T>(), nullptr, d->p, cov_csc_upload_w<T>(d, indices, values, ni), nullptr, dout, s);
    else launch_cov_mul<T>(static_cast<const T*>(d->X), d->ld, d->p, dind, dval, ni, dout, s);
    AHIP_CHECK(hipMemcpyAsync(out, dout, size_t(d->p) * sizeof(T), hipMemcpyDeviceToHost, s));
    AHIP_CHECK(hipStreamSynchronize(s));
}
// out[l, :] = v - A beta_l (v null: A beta_l) for the L rows of a validated CSR matrix, cov_batch_chunk_rows rows at a time: the
// chunk's part of B (kept sparse) or its union plan (dense storage; cov_batch_host.hpp) goes up, the batches run, and the
// finished rows come down, so the device scratch is one chunk's whatever L is.
template <class T>
void op_cov_mul_batch(adelie_hip_design* d, int64_t L, const int64_t* indptr, const int64_t* indices, const T* values, const T* v,
                      T* out) {
    set_device(d);
    hipStream_t s = d->stream;
    const int64_t p = d->p, chunk = cov_batch_chunk_rows(p, sizeof(T));
    constexpr int Lb = kCovBatchLb;
    T* dv = nullptr;
    if (v) {
        dv = scratch<T>(d->s_n2, size_t(p));
        AHIP_CHECK(hipMemcpyAsync(dv, v, size_t(p) * sizeof(T), hipMemcpyHostToDevice, s));
    }
    T* dout = scratch<T>(d->s_p1, size_t(std::min(chunk, L)) * size_t(p));
    CovBatchPlan<T> plan;
    for (int64_t l0 = 0; l0 < L; l0 += chunk) {
        const int64_t lc = std::min(chunk, L - l0);
        if (d->cov_csc()) {
            const int64_t e0 = indptr[l0], ne = indptr[l0 + lc] - e0;
            int64_t* dptr = scratch<int64_t>(d->s_idx1, size_t(lc) + 1);
            int64_t* dind = scratch<int64_t>(d->s_idx2, size_t(ne));
            T* dval = scratch<T>(d->s_n1, size_t(ne));
            T* dw = scratch<T>(d->s_work, size_t(p) * Lb);
            AHIP_CHECK(hipMemcpyAsync(dptr, indptr + l0, size_t(lc + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
            if (ne) {
                AHIP_CHECK(hipMemcpyAsync(dind, indices + e0, size_t(ne) * sizeof(int64_t), hipMemcpyHostToDevice, s));
                AHIP_CHECK(hipMemcpyAsync(dval, values + e0, size_t(ne) * sizeof(T), hipMemcpyHostToDevice, s));
            }
            for (int64_t b0 = 0; b0 < lc; b0 += Lb) {
                const int rows = int(std::min<int64_t>(Lb, lc - b0));
                int64_t max_row = 0;
                for (int r = 0; r < rows; ++r) max_row = std::max(max_row, indptr[l0 + b0 + r + 1] - indptr[l0 + b0 + r]);
                launch_cov_csc_fill_w_batch<T>(dptr + b0, dind, dval, e0, rows, max_row, dw, p, s);
                launch_cov_csc_coldot_batch<T>(d->cov_csc_view<T>(), dw, dv, rows, dout + size_t(b0) * size_t(p), s);
            }
        } else {
            cov_batch_plan_unions<T>(l0, lc, indptr, indices, values, plan);
            const size_t nu = plan.ucols.size();
            int64_t* duptr = scratch<int64_t>(d->s_idx1, plan.uptr.size());
            int32_t* ducols = scratch<int32_t>(d->s_idx2, nu);
            T* dcoef = scratch<T>(d->s_n1, nu * Lb);
            AHIP_CHECK(hipMemcpyAsync(duptr, plan.uptr.data(), plan.uptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
            if (nu) {
                AHIP_CHECK(hipMemcpyAsync(ducols, plan.ucols.data(), nu * sizeof(int32_t), hipMemcpyHostToDevice, s));
                AHIP_CHECK(hipMemcpyAsync(dcoef, plan.coef.data(), nu * Lb * sizeof(T), hipMemcpyHostToDevice, s));
            }
            launch_cov_mul_batch<T>(static_cast<const T*>(d->X), d->ld, p, duptr, ducols, dcoef, dv, lc, dout, s);
        }
        AHIP_CHECK(hipGetLastError());
        AHIP_CHECK(hipMemcpyAsync(out + size_t(l0) * size_t(p), dout, size_t(lc) * size_t(p) * sizeof(T), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s)); // (the next chunk overwrites the plan and the scratch)
    }
}
template <class T>
void op_cov_to_dense(adelie_hip_design* d, int64_t i, int64_t q, T* out) {
    set_device(d);
    if (d->cov_csc()) { // zeros and the stored entries of the block
        T* dout = scratch<T>(d->s_p1, size_t(q) * size_t(q));
        launch_cov_csc_to_dense<T>(d->cov_csc_view<T>(), i, q, dout, d->stream);
        AHIP_CHECK(hipMemcpyAsync(out, dout, size_t(q) * size_t(q) * sizeof(T), hipMemcpyDeviceToHost, d->stream));
        AHIP_CHECK(hipStreamSynchronize(d->stream));
        return;
    }
    const T* S = static_cast<const T*>(d->X);
    AHIP_CHECK(hipMemcpy2DAsync(out, size_t(q) * sizeof(T), S + i + i * d->ld, size_t(d->ld) * sizeof(T), size_t(q) * sizeof(T),
                                size_t(q), hipMemcpyDeviceToHost, d->stream));
    AHIP_CHECK(hipStreamSynchronize(d->stream));
    if (d->cov == 2) // the stored block is the transpose
        for (int64_t b = 0; b < q; ++b)
            for (int64_t a = b + 1; a < q; ++a) std::swap(out[a + b * q], out[b + a * q]);
}

// The MatrixConstraintBase operations (matrix_constraint_base.hpp) on a constraint handle: d->n == d, d->p == m, a row of A is
// column j of the stored matrix, dense or compressed (adelie_hip_design_create_constraint_csc).  Host vectors in and out; none
// of these is a hot path.
template <class T>
void op_constraint(adelie_hip_design* A, int op, int64_t j, const T* in, const int64_t* indices, int64_t ni, T* out) {
    set_device(A);
    hipStream_t s = A->stream;
    const int64_t d = A->n, m = A->p;
    const bool sparse = A->is_csc();
    const DenseView<T> Av = A->dense<T>(); // (null on a matrix kept sparse, and unused there)
    auto up = [&](T* dst, const T* src, size_t n) { AHIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, s)); };
    auto down = [&](T* dst, const T* src, size_t n) {
        AHIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
    };
    switch (op) {
        case ADELIE_HIP_CONS_TMUL:
        case ADELIE_HIP_CONS_RVMUL: { // the column sweep, over all rows of A or over row j
            const int64_t c0 = op == ADELIE_HIP_CONS_TMUL ? 0 : j, nc = op == ADELIE_HIP_CONS_TMUL ? m : 1;
            T* dv = scratch<T>(A->s_n1, size_t(d));
            T* dout = scratch<T>(A->s_p1, size_t(nc));
            T* work = scratch<T>(A->s_work, size_t(raw_sweep_work_elems(*A, nc, false)));
            up(dv, in, size_t(d));
            raw_sweep<T>(*A, dv, dout, c0, nc, nullptr, nullptr, nullptr, false, false, work, s);
            down(out, dout, size_t(nc));
            break;
        }
        case ADELIE_HIP_CONS_MUL:
        case ADELIE_HIP_CONS_SP_MUL:
        case ADELIE_HIP_CONS_RVTMUL: { // the column axpy
            int64_t q = op == ADELIE_HIP_CONS_MUL ? m : (op == ADELIE_HIP_CONS_SP_MUL ? ni : 1);
            std::vector<int32_t> cols(static_cast<size_t>(q));
            for (int64_t k = 0; k < q; ++k)
                cols[size_t(k)] = int32_t(op == ADELIE_HIP_CONS_MUL ? k : (op == ADELIE_HIP_CONS_SP_MUL ? indices[k] : j));
            std::vector<T> coef;
            if (sparse && op == ADELIE_HIP_CONS_SP_MUL) { // the compressed axpy wants distinct columns: repeats are summed here
                std::vector<int64_t> pos(static_cast<size_t>(q));
                for (int64_t k = 0; k < q; ++k) pos[size_t(k)] = k;
                std::stable_sort(pos.begin(), pos.end(), [&](int64_t a, int64_t b) { return indices[a] < indices[b]; });
                int64_t u = 0;
                for (int64_t k = 0; k < q; ++k) {
                    const int64_t at = pos[size_t(k)];
                    if (u > 0 && cols[size_t(u - 1)] == int32_t(indices[at])) coef[size_t(u - 1)] += in[at];
                    else cols[size_t(u++)] = int32_t(indices[at]), coef.push_back(in[at]);
                }
                q = u;
                in = coef.data();
            }
            T* dout = scratch<T>(A->s_n1, size_t(d));
            T* dcoef = scratch<T>(A->s_p1, size_t(q));
            int32_t* dcols = scratch<int32_t>(A->s_idx1, size_t(q));
            T* delta = nullptr;
            if (sparse) { // the zeroed p + 8 elements the compressed axpy scatters the coefficients into
                delta = scratch<T>(A->s_work, size_t(m) + 8);
                AHIP_CHECK(hipMemsetAsync(delta, 0, (size_t(m) + 8) * sizeof(T), s));
            }
            if (op == ADELIE_HIP_CONS_RVTMUL) up(dout, out, size_t(d));
            else AHIP_CHECK(hipMemsetAsync(dout, 0, size_t(d) * sizeof(T), s));
            if (q > 0) {
                up(dcoef, in, size_t(q));
                AHIP_CHECK(hipMemcpyAsync(dcols, cols.data(), size_t(q) * sizeof(int32_t), hipMemcpyHostToDevice, s));
                raw_axpy_cols<T>(*A, dcols, dcoef, nullptr, int32_t(q), T(1), dout, delta, s);
            }
            down(out, dout, size_t(d));
            break;
        }
        case ADELIE_HIP_CONS_RMMUL: { // out[c] = Q[:, c] . A[j, :]: the sweep of Q's columns with row j of A as the vector
            T* dQ = scratch<T>(A->s_misc, size_t(d) * size_t(d));
            T* dout = scratch<T>(A->s_p1, size_t(d));
            up(dQ, in, size_t(d) * size_t(d));
            if (sparse) { // row j of A times Q, through Q' (kernels_pinball_sparse.hip)
                DevBuf<T> dQT;
                dQT.reserve(size_t(d) * size_t(d));
                int32_t* dcol = scratch<int32_t>(A->s_idx1, 1);
                const int32_t jj = int32_t(j);
                AHIP_CHECK(hipMemcpyAsync(dcol, &jj, sizeof(int32_t), hipMemcpyHostToDevice, s));
                launch_transpose_square<T>(dQ, d, dQT.p, s);
                launch_csc_rows_dense<T>(A->csc<T>(), dcol, 1, dQT.p, dout, d, s);
                down(out, dout, size_t(d));
                break;
            }
            T* work = scratch<T>(A->s_work, size_t(sweep_work_elems(d, d)));
            launch_sweep<T>(DenseView<T>{dQ, d, d, d}, Av.X + j * Av.ld, dout, 0, d, nullptr, nullptr, nullptr, false, work, s);
            down(out, dout, size_t(d));
            break;
        }
        case ADELIE_HIP_CONS_COV: { // AQ[k, :] = A[k, :] Q for every row, then out[a, b] = AQ[a, :] . A[b, :]
            DevBuf<T> dQ, dAQ, dC;
            dQ.reserve(size_t(d) * size_t(d)), dAQ.reserve(size_t(d) * size_t(m)), dC.reserve(size_t(m) * size_t(m));
            up(dQ.p, in, size_t(d) * size_t(d));
            if (sparse) { // over the stored entries (kernels_pinball_sparse.hip): the rows-times-dense kernel reads the transpose of
                          // its matrix, so Q as it lies gives AQ[:, b] = Q A[b, :]', and out[a, b] = A[a, :] . AQ[:, b] = (A Q A')[a, b]
                launch_csc_rows_dense<T>(A->csc<T>(), nullptr, m, dQ.p, dAQ.p, d, s);
                launch_csc_rows_cols<T>(A->csc<T>(), nullptr, m, dAQ.p, d, m, dC.p, m, s);
            } else {
                launch_ptq<T>(dQ.p, d, nullptr, int32_t(d), Av.X, Av.ld, nullptr, int32_t(m), d, dAQ.p, d, s);
                launch_ptq<T>(dAQ.p, d, nullptr, int32_t(m), Av.X, Av.ld, nullptr, int32_t(m), d, dC.p, m, s);
            }
            down(out, dC.p, size_t(m) * size_t(m));
            break;
        }
        case ADELIE_HIP_CONS_TO_DENSE:
            if (sparse) { // zeros plus the scattered entries (for tests and small matrices)
                std::vector<int64_t> ptr(static_cast<size_t>(m) + 1);
                std::vector<int32_t> idx(static_cast<size_t>(A->nnz));
                std::vector<T> val(static_cast<size_t>(A->nnz));
                AHIP_CHECK(hipMemcpyAsync(ptr.data(), A->cptr, ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
                if (A->nnz) {
                    AHIP_CHECK(hipMemcpyAsync(idx.data(), A->cidx, idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                    AHIP_CHECK(hipMemcpyAsync(val.data(), A->cval, val.size() * sizeof(T), hipMemcpyDeviceToHost, s));
                }
                AHIP_CHECK(hipStreamSynchronize(s));
                std::fill(out, out + size_t(m) * size_t(d), T(0));
                for (int64_t r = 0; r < m; ++r)
                    for (int64_t t = ptr[size_t(r)]; t < ptr[size_t(r) + 1]; ++t) out[r * d + idx[size_t(t)]] = val[size_t(t)];
                break;
            }
            AHIP_CHECK(hipMemcpy2DAsync(out, size_t(d) * sizeof(T), Av.X, size_t(Av.ld) * sizeof(T), size_t(d) * sizeof(T), size_t(m),
                                        hipMemcpyDeviceToHost, s));
            AHIP_CHECK(hipStreamSynchronize(s));
            break;
        default: throw make_core_error("unknown constraint matrix operation.");
    }
}
} // namespace

extern "C" {

int adelie_hip_abi_version(void) { return ADELIE_HIP_ABI_VERSION; }
const char* adelie_hip_last_error(void) { return g_last_error.c_str(); }
int adelie_hip_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

int adelie_hip_design_create_dense(const void* host, int64_t n, int64_t p, int dtype, int order, int device,
                                   adelie_hip_design** out) {
    ABI_TRY
    if (!host || !out) throw make_core_error("null argument.");
    DesignGuard g(new_design(n, p, dtype, device));
    DTYPE_DISPATCH(g, create_dense_t<T>(g.get(), host, false, order))
    *out = g.release();
    ABI_CATCH
}

// adelie.matrix.dense(method="cov"): the (p, p) buffer is uploaded as it lies; a row-major input is therefore stored as A^T
// (cov == 2), which the cov_* operations account for and which is the same matrix when A is symmetric, as the method assumes
int adelie_hip_design_create_cov_dense(const void* host, int64_t p, int dtype, int order, int device, adelie_hip_design** out) {
    ABI_TRY
    if (!host || !out) throw make_core_error("null argument.");
    if (p <= 0) throw make_core_error("mat must be (p, p).");
    DesignGuard g(new_design(p, p, dtype, device));
    DTYPE_DISPATCH(g, create_dense_t<T>(g.get(), host, false, ADELIE_HIP_COL_MAJOR))
    g->cov = (order == ADELIE_HIP_ROW_MAJOR) ? 2 : 1;
    *out = g.release();
    ABI_CATCH
}

// adelie.matrix.sparse(method="cov", resident="csc") / block_diag(method="cov", resident="csc"): the column-compressed form of
// the symmetric (p, p) matrix and nothing else (cov_csc_host.hpp has the checks; kernels_cov_sparse.hip the operations).  A kCsc
// handle with the row arrays, block pointers and tile copy left null.
int adelie_hip_design_create_cov_csc(const int64_t* indptr, const int32_t* indices, const void* values, int64_t p, int dtype, int device,
                                     adelie_hip_design** out) {
    ABI_TRY
    if (!indptr || !out) throw make_core_error("null argument.");
    if (p <= 0) throw make_core_error("mat must be (p, p).");
    if (const char* e = cov_csc_validate(indptr, indices, values, p)) throw make_core_error(e);
    const int64_t nnz = indptr[p];
    DesignGuard g(new_design(p, p, dtype, device));
    adelie_hip_design* d = g.get();
    const size_t vs = dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
    const size_t nz1 = size_t(std::max<int64_t>(nnz, 1));
    d->kind = adelie_hip_design::kCsc;
    d->cov = 1;
    d->nnz = nnz;
    d->cov_lanes = cov_csc_lanes(nnz, p);
    hipStream_t s = d->stream;
    d->cptr.alloc(size_t(p + 1)), d->cidx.alloc(nz1), d->cval.alloc(nz1 * vs);
    AHIP_CHECK(hipMemcpyAsync(d->cptr, indptr, size_t(p + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (nnz) {
        AHIP_CHECK(hipMemcpyAsync(d->cidx, indices, size_t(nnz) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        AHIP_CHECK(hipMemcpyAsync(d->cval, values, size_t(nnz) * vs, hipMemcpyHostToDevice, s));
    }
    AHIP_CHECK(hipStreamSynchronize(s));
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_cov_lazy(adelie_hip_design* X, adelie_hip_design** out) {
    ABI_TRY
    if (!X || !out) throw make_core_error("null argument.");
    if (X->cov) throw make_core_error("mat must be a naive (n, p) matrix, not a covariance matrix.");
    no_view(X);
    no_pieces(*X, "lazy_cov");
    if (!X->is_dense() && !X->is_snp()) throw make_core_error("lazy_cov takes a dense or SNP design.");
    if (X->p > (int64_t(1) << 31) - 1) throw make_core_error("too many columns.");
    set_device(X);
    AHIP_CHECK(hipStreamSynchronize(X->stream));
    DesignGuard g(new_design(X->p, X->p, X->dtype, X->device));
    DTYPE_DISPATCH(X, cov_lazy_t<T>(X, g.get()))
    g->cov = 1;
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_cov_bmul(adelie_hip_design* d, const int64_t* subset, int64_t ns, const int64_t* indices,
                               const void* values, int64_t ni, void* out) {
    ABI_TRY
    need_cov(d);
    if (ns < 0 || ni < 0 || ns > d->p || ni > d->p) throw make_core_error("bmul() is given inconsistent inputs!");
    for (int64_t k = 0; k < ns; ++k)
        if (subset[k] < 0 || subset[k] >= d->p) throw make_core_error("bmul(): subset index out of range.");
    for (int64_t k = 0; k < ni; ++k)
        if (indices[k] < 0 || indices[k] >= d->p) throw make_core_error("bmul(): index out of range.");
    DTYPE_DISPATCH(d, op_cov_bmul<T>(d, subset, ns, indices, (const T*)values, ni, (T*)out))
    ABI_CATCH
}
int adelie_hip_design_cov_mul(adelie_hip_design* d, const int64_t* indices, const void* values, int64_t ni, void* out) {
    ABI_TRY
    need_cov(d);
    if (ni < 0 || ni > d->p) throw make_core_error("mul() is given inconsistent inputs!");
    for (int64_t k = 0; k < ni; ++k)
        if (indices[k] < 0 || indices[k] >= d->p) throw make_core_error("mul(): index out of range.");
    DTYPE_DISPATCH(d, op_cov_mul<T>(d, indices, (const T*)values, ni, (T*)out))
    ABI_CATCH
}
int adelie_hip_design_cov_mul_batch(adelie_hip_design* d, int64_t L, const int64_t* indptr, const int64_t* indices, const void* values,
                                    const void* v, void* out) {
    ABI_TRY
    if (!d) throw make_core_error("null argument.");
    if (!d->cov) throw make_core_error("mul_batch: A must be a covariance matrix (matrix.dense(method=\"cov\") or kept sparse), not a design matrix.");
    if (const char* e = cov_batch_validate(L, indptr, indices, values, d->p)) throw make_core_error(e);
    if (L > 0) {
        if (!out) throw make_core_error("null argument.");
        DTYPE_DISPATCH(d, op_cov_mul_batch<T>(d, L, indptr, indices, (const T*)values, (const T*)v, (T*)out))
    }
    ABI_CATCH
}
int adelie_hip_design_cov_to_dense(adelie_hip_design* d, int64_t i, int64_t q, void* out) {
    ABI_TRY
    need_cov(d);
    if (i < 0 || q < 0 || i + q > d->p) throw make_core_error("to_dense() is given inconsistent inputs!");
    if (q > 0) { DTYPE_DISPATCH(d, op_cov_to_dense<T>(d, i, q, (T*)out)) }
    ABI_CATCH
}

int adelie_hip_design_create_sparse(const int64_t* indptr, const int32_t* indices, const void* values, int64_t n, int64_t p,
                                    int dtype, int device, adelie_hip_design** out) {
    ABI_TRY
    if (!indptr || !out) throw make_core_error("null argument.");
    if (n <= 0 || p <= 0) throw make_core_error("matrix must have positive dimensions.");
    if (indptr[0] != 0) throw make_core_error("sparse(): indptr must start at 0.");
    for (int64_t j = 0; j < p; ++j)
        if (indptr[j + 1] < indptr[j]) throw make_core_error("sparse(): indptr must be non-decreasing.");
    const int64_t nnz = indptr[p];
    if (nnz > 0 && (!indices || !values)) throw make_core_error("null argument.");
    for (int64_t k = 0; k < nnz; ++k)
        if (indices[k] < 0 || indices[k] >= n) throw make_core_error("sparse(): row index out of range.");
    DesignGuard g(new_design(n, p, dtype, device));
    DTYPE_DISPATCH(g, create_sparse_t<T>(g.get(), indptr, indices, values))
    *out = g.release();
    ABI_CATCH
}

#include "design_csc.hpp"

int adelie_hip_design_create_standardized(adelie_hip_design* src, const double* centers, const double* scales,
                                          adelie_hip_design** out) {
    ABI_TRY
    if (!src || !centers || !scales || !out) throw make_core_error("null argument.");
    if (src->is_multi() || src->cov || src->constraint) no_view(src);
    no_pieces(*src, "standardize (standardize the dense piece with lazy=False before concatenating instead)");
    if (src->std_center) throw make_core_error("the design is a standardized view already.");
    for (int64_t j = 0; j < src->p; ++j)
        if (!(scales[j] != 0.0)) throw make_core_error("scales must be non-zero.");
    adelie_hip_design* d = nullptr;
    if (adelie_hip_design_alias(src, &d)) throw make_core_error(g_last_error);
    DesignGuard g(d);
    const int64_t p = src->p;
    const size_t vs = src->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
    d->std_center.alloc(size_t(p) * vs), d->std_iscale.alloc(size_t(p) * vs);
    if (src->dtype == ADELIE_HIP_F64) {
        std::vector<double> is(static_cast<size_t>(p));
        for (int64_t j = 0; j < p; ++j) is[size_t(j)] = 1.0 / scales[j];
        AHIP_CHECK(hipMemcpy(d->std_center, centers, size_t(p) * vs, hipMemcpyHostToDevice));
        AHIP_CHECK(hipMemcpy(d->std_iscale, is.data(), size_t(p) * vs, hipMemcpyHostToDevice));
    } else {
        std::vector<float> ce(static_cast<size_t>(p)), is(static_cast<size_t>(p));
        for (int64_t j = 0; j < p; ++j) { ce[size_t(j)] = float(centers[j]); is[size_t(j)] = float(1.0 / scales[j]); }
        AHIP_CHECK(hipMemcpy(d->std_center, ce.data(), size_t(p) * vs, hipMemcpyHostToDevice));
        AHIP_CHECK(hipMemcpy(d->std_iscale, is.data(), size_t(p) * vs, hipMemcpyHostToDevice));
    }
    *out = g.release();
    ABI_CATCH
}

// adelie.matrix.dense(method="constraint"): the (m, d) matrix A is kept row-major, which is the (d, m) column-major A' of a dense
// handle (a row of A is one contiguous column).  `order` is the memory order of the (m, d) source.
static int create_constraint(const void* src, bool on_device, int64_t m, int64_t d, int dtype, int order, int device,
                             adelie_hip_design** out) {
    ABI_TRY
    if (!src || !out) throw make_core_error("null argument.");
    if (m <= 0 || d <= 0) throw make_core_error("mat must be a non-empty (m, d) matrix.");
    DesignGuard g(new_design(d, m, dtype, device));
    const int stored = order == ADELIE_HIP_ROW_MAJOR ? ADELIE_HIP_COL_MAJOR : ADELIE_HIP_ROW_MAJOR; // of the (d, m) matrix A'
    DTYPE_DISPATCH(g, create_dense_t<T>(g.get(), src, on_device, stored))
    g->constraint = 1;
    *out = g.release();
    ABI_CATCH
}
int adelie_hip_design_create_constraint_dense(const void* host, int64_t m, int64_t d, int dtype, int order, int device,
                                              adelie_hip_design** out) {
    return create_constraint(host, false, m, d, dtype, order, device, out);
}
int adelie_hip_design_adopt_constraint_dense_dev(const void* dev_ptr, int64_t m, int64_t d, int dtype, int order, int device,
                                                 adelie_hip_design** out) {
    return create_constraint(dev_ptr, true, m, d, dtype, order, device, out);
}
int adelie_hip_constraint_op(adelie_hip_design* A, int op, int64_t j, const void* in, const int64_t* indices, int64_t n_indices,
                             void* out) {
    ABI_TRY
    if (!A || !out) throw make_core_error("null argument.");
    if (!A->constraint || !(A->is_dense() || A->is_csc()))
        throw make_core_error("A must be a constraint matrix (matrix.dense(method=\"constraint\")).");
    const int64_t m = A->p;
    if (op != ADELIE_HIP_CONS_TO_DENSE && !in) throw make_core_error("null argument.");
    if ((op == ADELIE_HIP_CONS_RVMUL || op == ADELIE_HIP_CONS_RVTMUL || op == ADELIE_HIP_CONS_RMMUL) && (j < 0 || j >= m))
        throw make_core_error("row index out of range.");
    if (op == ADELIE_HIP_CONS_SP_MUL) {
        if (n_indices < 0 || (n_indices > 0 && !indices)) throw make_core_error("sp_mul() is given inconsistent inputs!");
        for (int64_t k = 0; k < n_indices; ++k)
            if (indices[k] < 0 || indices[k] >= m) throw make_core_error("sp_mul(): index out of range.");
    }
    if (op == ADELIE_HIP_CONS_COV && double(m) * double(m) > 4e9) throw make_core_error("cov(): the (m, m) output is too large.");
    DTYPE_DISPATCH(A, op_constraint<T>(A, op, j, (const T*)in, indices, n_indices, (T*)out))
    ABI_CATCH
}

int adelie_hip_design_adopt_dense_dev(const void* dev_ptr, int64_t n, int64_t p, int dtype, int order, int device,
                                      adelie_hip_design** out) {
    ABI_TRY
    if (!dev_ptr || !out) throw make_core_error("null argument.");
    DesignGuard g(new_design(n, p, dtype, device));
    DTYPE_DISPATCH(g, create_dense_t<T>(g.get(), dev_ptr, true, order))
    *out = g.release();
    ABI_CATCH
}

#include "design_snp.hpp"

int adelie_hip_design_batch_stats(adelie_hip_design* d, double* out) {
    ABI_TRY
    if (!d || !out) throw make_core_error("null argument.");
    // (a design made of pieces never joins the batching: its batcher stays null and the counts are zero)
    adelie_hip_design* owner = d->batch_owner ? d->batch_owner : d;
    adelie_hip_internal_batch_stats(owner->batcher, out);
    ABI_CATCH
}

static adelie_hip_design* shadow_owner(adelie_hip_design* d) { return d->batch_owner ? d->batch_owner : d; }
static void shadow_free(adelie_hip_design* o) { o->ShadowArrs::reset(); }
static size_t shadow_bytes(int kind, int64_t p, int64_t lds) {
    return size_t(p) * size_t(lds) * (kind == ahip::kShadowQ15 ? sizeof(int16_t) : sizeof(float)) +
           (kind == ahip::kShadowQ15 ? 3 : 2) * size_t(p) * sizeof(double);
}
// One copy of `kind` built and measured on d's stream: false (and nothing left allocated) when memory is short, a call fails or
// an entry cannot be held.  (plain status checks: an error here must not leave the blocks behind with sh_state still 0)
static bool shadow_build(adelie_hip_design* d, adelie_hip_design* o, int kind) {
    const bool q15 = kind == ahip::kShadowQ15;
    const int64_t lds = q15 ? ahip::shadow_q15_ld(d->n) : (d->n + 3) / 4 * 4; // 16-byte aligned columns
    const size_t need = shadow_bytes(kind, d->p, lds);
    size_t free_b = 0, total_b = 0;
    AHIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t keep = std::max<size_t>(size_t(4) << 30, total_b / 10);
    bool ok = free_b >= need && free_b - need >= keep;
    DevArr<int32_t> bad;
    if (ok)
        ok = o->sh_X.try_alloc(size_t(d->p) * size_t(lds) * (q15 ? sizeof(int16_t) : sizeof(float))) && o->sh_err.try_alloc(size_t(d->p)) &&
             o->sh_nrm.try_alloc(size_t(d->p)) && (!q15 || o->sh_scale.try_alloc(size_t(d->p))) && bad.try_alloc(1);
    if (ok) {
        int32_t h_bad = 0;
        ok = hipMemsetAsync(bad, 0, sizeof(int32_t), d->stream) == hipSuccess;
        if (ok && q15)
            launch_shadow_build_q15(d->dense<double>(), static_cast<int16_t*>(o->sh_X), lds, o->sh_scale, o->sh_err, o->sh_nrm, bad,
                                    d->stream);
        else if (ok)
            launch_shadow_build(d->dense<double>(), static_cast<float*>(o->sh_X), lds, o->sh_err, o->sh_nrm, bad, d->stream);
        ok = ok && hipMemcpyAsync(&h_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, d->stream) == hipSuccess;
        ok = (hipStreamSynchronize(d->stream) == hipSuccess) && ok;
        if (!ok) (void)hipGetLastError();
        ok = ok && h_bad == 0; // an entry that is not finite (float32: or beyond FLT_MAX): no shadow for this design
        o->sh_ld = lds;
        o->sh_kind = kind;
        ++o->sh_n_builds;
    }
    if (!ok) shadow_free(o);
    return ok;
}
// err / nrm of the built copy on the host (the kind rule and shadow_info read them)
static bool shadow_fetch_err_nrm(adelie_hip_design* d, adelie_hip_design* o, std::vector<double>& err, std::vector<double>& nrm) {
    err.resize(size_t(d->p));
    nrm.resize(size_t(d->p));
    bool ok = hipMemcpyAsync(err.data(), o->sh_err, err.size() * sizeof(double), hipMemcpyDeviceToHost, d->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(nrm.data(), o->sh_nrm, nrm.size() * sizeof(double), hipMemcpyDeviceToHost, d->stream) == hipSuccess;
    ok = (hipStreamSynchronize(d->stream) == hipSuccess) && ok;
    if (!ok) (void)hipGetLastError();
    return ok;
}

bool adelie_hip_internal_shadow_acquire(adelie_hip_design* d, ahip::ShadowView* out) {
    if (!d || !d->is_dense() || d->dtype != ADELIE_HIP_F64 || d->cov || d->constraint || d->std_center || !d->X || d->n < 1 || d->p < 1) return false;
    adelie_hip_design* o = shadow_owner(d);
    if (o->X != d->X || o->ld != d->ld || o->n != d->n || o->p != d->p) return false;
    std::lock_guard<std::mutex> lk(o->sh_mu);
    if (o->sh_state == 0) {
        // the kind (shadow_kind_host.hpp): q15 when forced, and under `auto` on a large design whose q15 copy measures well; a
        // q15 copy the rule turns down is freed and the float32 copy made in its place
        const int forced = ahip::Hooks::shadow_kind_env();
        bool ok = false;
        if (ahip::shadow_q15_wanted(forced, d->n, d->p, ahip::Hooks::shadow_min_bytes_env())) {
            ok = shadow_build(d, o, ahip::kShadowQ15);
            if (ok && forced != ahip::kShadowQ15) {
                std::vector<double> err, nrm;
                ok = shadow_fetch_err_nrm(d, o, err, nrm);
                if (!ok || ahip::shadow_kind_pick(forced, err.data(), nrm.data(), d->p) != ahip::kShadowQ15) {
                    shadow_free(o);
                    ok = ok && shadow_build(d, o, ahip::kShadowF32);
                }
            }
        } else {
            ok = shadow_build(d, o, ahip::kShadowF32);
        }
        if (!ok) ++o->sh_n_ineligible;
        o->sh_state = ok ? 1 : -1;
    }
    if (o->sh_state != 1) return false;
    *out = ahip::ShadowView{o->sh_X, d->n, d->p, o->sh_ld, o->sh_err, o->sh_nrm, o->sh_kind, o->sh_scale};
    return true;
}
void adelie_hip_internal_shadow_mark_stale(adelie_hip_design* d) {
    adelie_hip_design* o = shadow_owner(d);
    std::lock_guard<std::mutex> lk(o->sh_mu);
    if (o->sh_state == 1) ++o->sh_n_ineligible;
    o->sh_state = -1; // (the memory stays until drop_shadow / destroy: a solve on an alias may still be reading it)
}

int adelie_hip_design_drop_shadow(adelie_hip_design* d) {
    ABI_TRY
    if (!d) throw make_core_error("null argument.");
    adelie_hip_design* o = shadow_owner(d);
    AHIP_CHECK(hipSetDevice(o->device));
    std::lock_guard<std::mutex> lk(o->sh_mu);
    AHIP_CHECK(hipDeviceSynchronize());
    shadow_free(o);
    o->sh_state = 0;
    ABI_CATCH
}
int adelie_hip_design_shadow_stats(adelie_hip_design* d, int64_t* out) {
    ABI_TRY
    if (!d || !out) throw make_core_error("null argument.");
    adelie_hip_design* o = shadow_owner(d);
    std::lock_guard<std::mutex> lk(o->sh_mu);
    out[0] = o->sh_state; out[1] = o->sh_n_builds; out[2] = o->sh_n_ineligible;
    ABI_CATCH
}
int adelie_hip_design_shadow_info(adelie_hip_design* d, int64_t* out_i, double* out_d) {
    ABI_TRY
    if (!d || !out_i || !out_d) throw make_core_error("null argument.");
    adelie_hip_design* o = shadow_owner(d);
    AHIP_CHECK(hipSetDevice(o->device));
    std::lock_guard<std::mutex> lk(o->sh_mu);
    out_i[0] = -1; out_i[1] = 0;
    out_d[0] = 0; out_d[1] = 0;
    if (o->sh_state == 1 && o->sh_X) {
        out_i[0] = o->sh_kind;
        out_i[1] = int64_t(shadow_bytes(o->sh_kind, o->p, o->sh_ld));
        std::vector<double> err, nrm;
        if (!shadow_fetch_err_nrm(o, o, err, nrm)) throw make_core_error("could not read the shadow's measurements.");
        // e_j / ||x_j|| with the copy's own norm for ||x_j|| (they differ by at most e_j); a zero column counts 0
        for (size_t j = 0; j < err.size(); ++j) {
            const double q = err[j] == 0 ? 0.0 : err[j] / nrm[j];
            err[j] = q >= 0 ? q : HUGE_VAL; // (NaN: inf / inf)
        }
        std::sort(err.begin(), err.end());
        out_d[0] = err[(err.size() - 1) / 2];
        out_d[1] = err.back();
    }
    ABI_CATCH
}

int adelie_hip_design_alias(adelie_hip_design* src, adelie_hip_design** out) {
    ABI_TRY
    if (!src || !out) throw make_core_error("null argument.");
    if (src->is_multi() || src->cov || src->constraint) no_view(src);
    DesignGuard g(new_design(src->n, src->p, src->dtype, src->device)); // own stream, own scratch
    adelie_hip_design* d = g.get();
    d->kind = src->kind;
    d->borrow_arrays(*src);
    d->batch_owner = src->batch_owner ? src->batch_owner : src;
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_slice(adelie_hip_design* base, int64_t r0, int64_t nr, int64_t c0, int64_t nc,
                                   adelie_hip_design** out) {
    ABI_TRY
    if (!base || !out) throw make_core_error("null argument.");
    if (base->constraint) no_view(base);
    no_pieces(*base, "subset");
    if ((!base->is_dense() && !base->is_snp()) || base->cov || base->std_center)
        throw make_core_error("only dense and 2-bit SNP designs are sliced in place.");
    if (r0 < 0 || nr < 1 || c0 < 0 || nc < 1 || r0 + nr > base->n || c0 + nc > base->p)
        throw make_core_error("slice out of range.");
    const int64_t es = base->dtype == ADELIE_HIP_F64 ? 8 : 4;
    if (base->is_snp() && (r0 != 0 || nr != base->n)) throw make_core_error("a 2-bit design is sliced by columns only.");
    if (base->is_dense() && (r0 * es) % 16 != 0) throw make_core_error("a row slice must start on a 16-byte boundary.");
    DesignGuard g(new_design(nr, nc, base->dtype, base->device)); // own stream, own scratch
    adelie_hip_design* d = g.get();
    d->kind = base->kind;
    if (base->is_dense()) { // (borrowed: a slice never frees what it points into)
        d->X.borrow(static_cast<char*>(base->X) + (c0 * base->ld + r0) * es);
        d->ld = base->ld;
    } else {
        d->bits.borrow(base->bits + c0 * base->ldb);
        d->ldb = base->ldb;
        d->impute.borrow(static_cast<char*>(base->impute) + c0 * es);
    }
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_multi(adelie_hip_design* base, int64_t K, int intercept, adelie_hip_design** out) {
    ABI_TRY
    if (!base || !out) throw make_core_error("null argument.");
    if (base->constraint) no_view(base);
    no_pieces(*base, "kronecker_eye / a multi-response family");
    if ((!base->is_dense() && !base->is_snp()) || base->cov || base->std_center)
        throw make_core_error("the multi-response view needs a dense or 2-bit SNP base design.");
    if (K < 1) throw make_core_error("K must be >= 1.");
    const int64_t icpt = intercept ? 1 : 0;
    if ((base->p + icpt) * K > int64_t(0x7fffffff) || base->n * K > (int64_t(1) << 40))
        throw make_core_error("the multi-response view is too large.");
    DesignGuard g(new_design(base->n * K, (base->p + icpt) * K, base->dtype, base->device)); // own stream + scratch
    adelie_hip_design* d = g.get();
    d->kind = adelie_hip_design::kMulti;
    d->DenseArrs::borrow_from(*base);
    d->SnpArrs::borrow_from(*base); // (2-bit base: the K-wide kernels decode the calls themselves, MultiView::bits)
    d->mK = K;
    d->micpt = int(icpt);
    d->nb = base->n;
    d->pb = base->p;
    DTYPE_DISPATCH(d, alloc_multi_ones<T>(d->ones, base->n, d->stream)) // the column of ones
    AHIP_CHECK(hipStreamSynchronize(d->stream));
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_derived(adelie_hip_design* src, const int64_t* rows, int64_t n_rows, const int64_t* cols,
                                     int64_t n_cols, const double* centers, const double* scales, adelie_hip_design** out) {
    ABI_TRY
    if (!src || !out) throw make_core_error("null argument.");
    no_view(src);
    no_pieces(*src, (centers || scales) ? "standardize (standardize the dense piece with lazy=False before concatenating instead)" : "subset");
    const int64_t nout = rows ? n_rows : src->n, pout = cols ? n_cols : src->p;
    if (rows)
        for (int64_t i = 0; i < n_rows; ++i)
            if (rows[i] < 0 || rows[i] >= src->n) throw make_core_error("subset contains an out-of-range row index.");
    if (cols)
        for (int64_t j = 0; j < n_cols; ++j)
            if (cols[j] < 0 || cols[j] >= src->p) throw make_core_error("subset contains an out-of-range column index.");
    if (scales)
        for (int64_t j = 0; j < pout; ++j)
            if (!(scales[j] != 0.0)) throw make_core_error("scales must be non-zero.");
    DesignGuard g(new_design(nout, pout, src->dtype, src->device));
    DTYPE_DISPATCH(src, derive_t<T>(src, g.get(), rows, n_rows, cols, n_cols, centers, scales))
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_concat(adelie_hip_design* const* srcs, int64_t k, int axis, adelie_hip_design** out) {
    ABI_TRY
    if (!srcs || !out || k <= 0) throw make_core_error("null argument.");
    if (axis != 0 && axis != 1) throw make_core_error("axis must be 0 or 1.");
    int64_t n = 0, p = 0;
    for (int64_t m = 0; m < k; ++m) {
        if (!srcs[m]) throw make_core_error("null argument.");
        no_view(srcs[m]);
        no_pieces(*srcs[m], "a further concatenate");
        if (srcs[m]->dtype != srcs[0]->dtype || srcs[m]->device != srcs[0]->device)
            throw make_core_error("concatenate(): the matrices must share dtype and device.");
        if (axis == 1) {
            if (srcs[m]->n != srcs[0]->n) throw make_core_error("All matrices must have the same number of rows.");
            p += srcs[m]->p;
            n = srcs[0]->n;
        } else {
            if (srcs[m]->p != srcs[0]->p) throw make_core_error("All matrices must have the same number of columns.");
            n += srcs[m]->n;
            p = srcs[0]->p;
        }
    }
    DesignGuard g(new_design(n, p, srcs[0]->dtype, srcs[0]->device));
    DTYPE_DISPATCH(srcs[0], concat_t<T>(srcs, k, axis, g.get()))
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_pieces(adelie_hip_design* const* srcs, int64_t k, adelie_hip_design** out) {
    ABI_TRY
    if (!srcs || !out) throw make_core_error("null argument.");
    std::vector<PieceInfo> info;
    for (int64_t m = 0; m < k; ++m) {
        const adelie_hip_design* s = srcs[m];
        if (!s) throw make_core_error("null argument.");
        info.push_back(PieceInfo{s->kind, s->std_center != nullptr, s->cov != 0, s->constraint != 0, s->dtype, s->device, s->n, s->p});
    }
    const std::string refusal = pieces_validate(info.data(), k);
    if (!refusal.empty()) throw make_core_error(refusal);
    int64_t p_of[kMaxPieces], p = 0;
    for (int64_t m = 0; m < k; ++m) {
        p += (p_of[m] = srcs[m]->p);
        if (srcs[m]->is_snp() ? (!srcs[m]->bits || !srcs[m]->impute) : !srcs[m]->X) throw make_core_error("a piece holds no array.");
    }
    set_device(srcs[0]);
    DesignGuard g(new_design(srcs[0]->n, p, srcs[0]->dtype, srcs[0]->device)); // own stream, own scratch; no array of its own
    adelie_hip_design* d = g.get();
    d->kind = adelie_hip_design::kPieces;
    d->pc_k = int(k);
    pieces_first_cols(p_of, int(k), d->pc_first);
    for (int64_t m = 0; m < k; ++m) {
        const adelie_hip_design* s = srcs[m];
        // the piece's own creation (or whatever wrote it last) ran on its stream: order this design's work after it
        AHIP_CHECK(hipStreamSynchronize(s->stream));
        d->pc_kind[m] = s->is_snp() ? kPieceSnp : kPieceDense;
        if (s->is_snp()) d->pc_base[m].borrow(static_cast<void*>(s->bits.get())), d->pc_ld[m] = s->ldb, d->pc_impute[m].borrow(s->impute);
        else d->pc_base[m].borrow(s->X), d->pc_ld[m] = s->ld;
    }
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_one_hot(adelie_hip_design* Z, const int64_t* levels, adelie_hip_design** out) {
    ABI_TRY
    check_factor_source(Z, levels, out, "one_hot");
    set_device(Z);
    std::vector<FactorBlock> blocks(static_cast<size_t>(Z->p));
    for (int64_t j = 0; j < Z->p; ++j) {
        bool disc;
        const int32_t l = factor_basis(levels, j, disc);
        // continuous: [z] = the basis [1, z] without its constant column; discrete: [z == 0, ..., z == l - 1]
        blocks[size_t(j)] = FactorBlock{0, 0, int32_t(j), int32_t(j), l, 1, disc ? 0 : 1, (disc ? 1 : 0) | 4};
    }
    DTYPE_DISPATCH(Z, create_factor_t<T>(Z, blocks, "one_hot", out))
    ABI_CATCH
}

int adelie_hip_design_create_interaction(adelie_hip_design* Z, const int64_t* pairs, int64_t n_pairs, const int64_t* levels,
                                         adelie_hip_design** out) {
    ABI_TRY
    check_factor_source(Z, levels, out, "interaction");
    if (!pairs || n_pairs <= 0) throw make_core_error("interaction(): pairs must be non-empty.");
    set_device(Z);
    std::vector<FactorBlock> blocks(static_cast<size_t>(n_pairs));
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int64_t i0 = pairs[2 * k], i1 = pairs[2 * k + 1];
        if (i0 < 0 || i0 >= Z->p || i1 < 0 || i1 >= Z->p || i0 == i1)
            throw make_core_error("interaction(): every pair must name two different columns of mat.");
        bool d0, d1;
        const int32_t l0 = factor_basis(levels, i0, d0), l1 = factor_basis(levels, i1, d1);
        blocks[size_t(k)] = FactorBlock{0, 0, int32_t(i0), int32_t(i1), l0, l1, (!d0 && !d1) ? 1 : 0, (d0 ? 1 : 0) | (d1 ? 2 : 0)};
    }
    DTYPE_DISPATCH(Z, create_factor_t<T>(Z, blocks, "interaction", out))
    ABI_CATCH
}

int adelie_hip_design_create_convex_relu(adelie_hip_design* Z, const uint8_t* mask, int64_t m, int gated, adelie_hip_design** out) {
    ABI_TRY
    if (!Z || !out || (!mask && m > 0 && Z->n > 0)) throw make_core_error("null argument.");
    if (!Z->is_dense() || Z->cov || Z->constraint || Z->std_center)
        throw make_core_error("convex_relu(): mat must be a resident dense naive design (not an SNP, sparse, view or covariance handle).");
    if (m < 0) throw make_core_error("mask must be (n, m) where mat is (n, d).");
    set_device(Z);
    DTYPE_DISPATCH(Z, create_relu_t<T>(Z, mask, m, gated, out))
    ABI_CATCH
}

int64_t adelie_hip_design_factor_groups(const adelie_hip_design* d, int64_t* groups, int64_t* group_sizes, int64_t cap) {
    if (!d || d->f_outer.empty()) return -1;
    const int64_t G = int64_t(d->f_outer.size()) - 1;
    for (int64_t g = 0; g < G && g < cap; ++g) {
        if (groups) groups[g] = d->f_outer[size_t(g)];
        if (group_sizes) group_sizes[g] = d->f_outer[size_t(g) + 1] - d->f_outer[size_t(g)];
    }
    return G;
}

int adelie_hip_design_impute(adelie_hip_design* d, double* out) {
    ABI_TRY
    no_view(d);
    if (!d || !out) throw make_core_error("null argument.");
    no_pieces(*d, "impute (ask the 2-bit pieces)");
    if (!d->is_snp()) throw make_core_error("impute is only defined for SNP designs.");
    set_device(d);
    if (d->dtype == ADELIE_HIP_F64) {
        AHIP_CHECK(hipMemcpy(out, d->impute, size_t(d->p) * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        std::vector<float> f(size_t(d->p));
        AHIP_CHECK(hipMemcpy(f.data(), d->impute, size_t(d->p) * sizeof(float), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < d->p; ++j) out[j] = f[size_t(j)];
    }
    ABI_CATCH
}

int adelie_hip_design_destroy(adelie_hip_design* d) {
    if (!d) return 0;
    (void)hipSetDevice(d->device);
    if (d->stream) {
        (void)hipStreamSynchronize(d->stream);
        (void)hipStreamDestroy(d->stream);
    }
    if (d->batcher) adelie_hip_internal_free_batcher(d->batcher);
    delete d; // (releases the arrays the handle owns)
    if (live_designs().fetch_sub(1) == 1) DevPool::trim();
    return 0;
}

int64_t adelie_hip_design_owned_bytes(void) { return owned_arr_bytes().load(); }

int64_t adelie_hip_design_rows(const adelie_hip_design* d) { return d->n; }
int64_t adelie_hip_design_cols(const adelie_hip_design* d) { return d->p; }
int adelie_hip_design_dtype(const adelie_hip_design* d) { return d->dtype; }
int adelie_hip_design_device(const adelie_hip_design* d) { return d->device; }
void* adelie_hip_design_stream(const adelie_hip_design* d) { return d->stream; }

int adelie_hip_design_cmul(adelie_hip_design* d, int64_t j, const void* v, const void* weights, double* out) {
    ABI_TRY
    no_view(d);
    check_col(d, j, 1, "cmul");
    DTYPE_DISPATCH(d, { T o; op_sweep<T>(d, j, 1, (const T*)v, (const T*)weights, &o, false); *out = o; })
    ABI_CATCH
}
int adelie_hip_design_ctmul(adelie_hip_design* d, int64_t j, double v, void* out) {
    ABI_TRY
    no_view(d);
    check_col(d, j, 1, "ctmul");
    DTYPE_DISPATCH(d, { T c = T(v); op_axpy<T>(d, j, 1, &c, (T*)out); })
    ABI_CATCH
}
int adelie_hip_design_bmul(adelie_hip_design* d, int64_t j, int64_t q, const void* v, const void* weights, void* out) {
    ABI_TRY
    no_view(d);
    check_col(d, j, q, "bmul");
    DTYPE_DISPATCH(d, op_sweep<T>(d, j, q, (const T*)v, (const T*)weights, (T*)out, false))
    ABI_CATCH
}
int adelie_hip_design_btmul(adelie_hip_design* d, int64_t j, int64_t q, const void* v, void* out) {
    ABI_TRY
    no_view(d);
    check_col(d, j, q, "btmul");
    DTYPE_DISPATCH(d, op_axpy<T>(d, j, q, (const T*)v, (T*)out))
    ABI_CATCH
}
// the column list of bmul_cols / btmul_cols, checked and narrowed to the kernels' int32
static std::vector<int32_t> checked_cols(const adelie_hip_design* d, const int64_t* cols, int64_t q, const char* what) {
    if (!d || !cols || q < 1) throw make_core_error(std::string(what) + "() is given inconsistent inputs!");
    std::vector<int32_t> c(static_cast<size_t>(q));
    for (int64_t k = 0; k < q; ++k) {
        if (cols[k] < 0 || cols[k] >= d->p) throw make_core_error(std::string(what) + "(): column index out of range.");
        c[size_t(k)] = int32_t(cols[k]);
    }
    return c;
}
int adelie_hip_design_bmul_cols(adelie_hip_design* d, const int64_t* cols, int64_t q, const void* v, const void* weights, void* out) {
    ABI_TRY
    no_view(d);
    const std::vector<int32_t> c = checked_cols(d, cols, q, "bmul_cols");
    DTYPE_DISPATCH(d, op_sweep<T>(d, 0, q, (const T*)v, (const T*)weights, (T*)out, false, c.data()))
    ABI_CATCH
}
int adelie_hip_design_btmul_cols(adelie_hip_design* d, const int64_t* cols, int64_t q, const void* v, void* out) {
    ABI_TRY
    no_view(d);
    const std::vector<int32_t> c = checked_cols(d, cols, q, "btmul_cols");
    if (d->is_csc()) { // (the compressed-column update scatters the coefficients by column)
        std::vector<int32_t> srt(c);
        std::sort(srt.begin(), srt.end());
        if (std::adjacent_find(srt.begin(), srt.end()) != srt.end())
            throw make_core_error("btmul_cols(): the columns must be distinct on a design kept sparse.");
    }
    DTYPE_DISPATCH(d, op_axpy<T>(d, 0, q, (const T*)v, (T*)out, c.data()))
    ABI_CATCH
}
int adelie_hip_design_mul(adelie_hip_design* d, const void* v, const void* weights, void* out) {
    ABI_TRY
    no_view(d);
    DTYPE_DISPATCH(d, op_sweep<T>(d, 0, d->p, (const T*)v, (const T*)weights, (T*)out, false))
    ABI_CATCH
}
int adelie_hip_design_mul_batch(adelie_hip_design* d, const void* V, int64_t L, void* out) {
    ABI_TRY
    no_view(d);
    if (L < 0 || (L > 0 && (!V || !out))) throw make_core_error("mul_batch() is given inconsistent inputs!");
    if (L == 0) return 0;
    DTYPE_DISPATCH(d, op_mul_batch<T>(d, (const T*)V, L, (T*)out))
    ABI_CATCH
}
int adelie_hip_design_cov(adelie_hip_design* d, int64_t j, int64_t q, const void* sqrt_weights, void* out) {
    ABI_TRY
    no_view(d);
    check_col(d, j, q, "cov");
    DTYPE_DISPATCH(d, op_cov<T>(d, j, q, (const T*)sqrt_weights, (T*)out))
    ABI_CATCH
}
int adelie_hip_design_sq_mul(adelie_hip_design* d, const void* weights, void* out) {
    ABI_TRY
    no_view(d);
    DTYPE_DISPATCH(d, op_sweep<T>(d, 0, d->p, (const T*)weights, (const T*)nullptr, (T*)out, true))
    ABI_CATCH
}
int adelie_hip_design_sp_tmul(adelie_hip_design* d, int64_t L, const int64_t* indptr, const int64_t* indices,
                              const void* values, void* out) {
    ABI_TRY
    no_view(d);
    if (L < 0) throw make_core_error("sp_tmul() is given inconsistent inputs!");
    if (L == 0) return 0;
    DTYPE_DISPATCH(d, op_sp_tmul<T>(d, L, indptr, indices, (const T*)values, (T*)out))
    ABI_CATCH
}

int adelie_hip_design_glm_path_losses(adelie_hip_design* d, int glm_kind, int64_t L, const int64_t* indptr,
                                      const int64_t* indices, const void* values, const void* intercepts,
                                      const void* offsets, const void* y, const void* weights_a, const void* weights_b,
                                      double* out) {
    ABI_TRY
    no_view(d);
    if (!d || !indptr || !intercepts || !offsets || !y || !weights_a || !weights_b || !out)
        throw make_core_error("null argument.");
    if (L < 0) throw make_core_error("L must be >= 0.");
    if (glm_kind == ADELIE_HIP_GLM_COX || glm_kind == ADELIE_HIP_GLM_CALLBACK || glm_kind == ADELIE_HIP_GLM_MULTINOMIAL)
        throw make_core_error("glm_path_losses: elementwise single-response families only.");
    if (L > 0) {
        DTYPE_DISPATCH(d, op_path_losses<T>(d, glm_kind, L, indptr, indices, (const T*)values, (const T*)intercepts,
                                            (const T*)offsets, (const T*)y, (const T*)weights_a, (const T*)weights_b, out))
    }
    ABI_CATCH
}

int adelie_hip_design_multi_path_losses(adelie_hip_design* d, int glm_kind, int K, int64_t L, const int64_t* indptr,
                                        const int64_t* indices, const void* values, const void* intercepts,
                                        const void* offsets, const void* y, const void* weights_a, const void* weights_b,
                                        double* out) {
    ABI_TRY
    no_view(d);
    if (!d || !indptr || !intercepts || !offsets || !y || !weights_a || !weights_b || !out)
        throw make_core_error("null argument.");
    if (L < 0) throw make_core_error("L must be >= 0.");
    if (K < 1) throw make_core_error("K must be >= 1.");
    if (glm_kind != ADELIE_HIP_GLM_GAUSSIAN && glm_kind != ADELIE_HIP_GLM_MULTINOMIAL)
        throw make_core_error("multi_path_losses: glm_kind must be GAUSSIAN (multigaussian) or MULTINOMIAL.");
    if (L > 0) {
        DTYPE_DISPATCH(d, op_multi_path_losses<T>(d, glm_kind, K, L, indptr, indices, (const T*)values, (const T*)intercepts,
                                                  (const T*)offsets, (const T*)y, (const T*)weights_a, (const T*)weights_b, out))
    }
    ABI_CATCH
}

int adelie_hip_design_cox_path_losses(adelie_hip_design* d, const adelie_hip_glm_cox* ga, const adelie_hip_glm_cox* gb, int64_t L,
                                      const int64_t* indptr, const int64_t* indices, const void* values,
                                      const void* intercepts, const void* offsets, int64_t max_batch, double* out) {
    ABI_TRY
    no_view(d);
    if (!d || !ga || !gb || !indptr || !intercepts || !offsets || !out) throw make_core_error("null argument.");
    if (L < 0) throw make_core_error("cox_path_losses: L must be >= 0.");
    if (max_batch < 0) throw make_core_error("cox_path_losses: max_batch must be >= 0 (0: chosen by the scratch bound).");
    for (const adelie_hip_glm_cox* g : {ga, gb}) {
        if (g->device != d->device) throw make_core_error("cox_path_losses: the family's handle is on another device than the design.");
        if (g->dtype != d->dtype) throw make_core_error("cox_path_losses: the family's dtype differs from the design's.");
        if (g->pack.n != d->n) throw make_core_error("cox_path_losses: the family and the design differ in their number of rows.");
    }
    if (L > 0) {
        DTYPE_DISPATCH(d, op_cox_path_losses<T>(d, ga->pack, gb->pack, L, indptr, indices, (const T*)values,
                                                (const T*)intercepts, (const T*)offsets, max_batch, out))
    }
    ABI_CATCH
}

} // extern "C"

namespace ahip {
void set_last_error(const std::string& s) { g_last_error = s; }
} // namespace ahip
