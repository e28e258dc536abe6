// kernels_css.hip — column subset selection on a resident covariance matrix (adelie.solver.css_cov: solver_css_cov.hpp,
// state_css_cov.ipp).  Kernels, the host loop driver and the C-ABI entry points of adelie_hip_css_cov_solve.
//
// Working set on the device: the caller's A (read only), one p x p residual covariance S_resid (both triangles, ld = p), the
// p-vectors beta / diag / scores, a membership mask and one record of scalars.  The reference updates one triangle with Eigen's
// rankUpdate; here both triangles are stored so that every access of the hot pass is a contiguous column (twice the bytes of
// the reference's update, all of them streamed).  One pass does  S_resid += c * beta beta^T  and, fused, the per-column score
// statistic of the UPDATED matrix; the updated diagonal  d_i + c * beta_i^2  is formed before the pass from the old diagonal, so
// the pass needs nothing from other columns.  Every element is updated as fma(c, beta_i * beta_j, S_ij): the product commutes,
// so the two triangles stay bit-identical.  A workgroup owns whole columns and reduces in a fixed order; there are no
// floating-point atomics, so two runs give the same bits.
//
// subset_factor semantics (compute_subset_factor_scores): with one thread the reference evaluates j_to_swap first and returns if
// it is +inf; otherwise it scans j ascending and stops filling scores at the first +inf (the rest stay -inf).  Here every
// column is computed.  The decision is the same: in the first case the arg-max lands on some +inf (the lowest-index one) and
// scores[j] < inf is false for scores[j] = +inf, so nothing is swapped; in the second case the lowest-index +inf is exactly
// the column the reference stopped at, it wins the arg-max (ties go to the lowest index, as Eigen's maxCoeff), and
// scores[j_to_swap] is finite in both.  The early-exit flag (any +inf) is returned in the record.
// min_det (compute_min_det_scores) zeroes only the FIRST non-member whose -max(d, 0) >= -1e-10 and returns; that column is
// found in the arg-max kernel, so that a later such column keeps its own (negative) value in the swap comparison.
#include <cmath>
#include <limits>

#include "common.hpp"
#include "wavered.hpp"

namespace ahip {
namespace {

enum { CSS_LS = 0, CSS_SF = 1, CSS_MD = 2 };
constexpr int kCssCols = 4;      // columns a workgroup handles per trip: beta_i / d_i / mask_i are loaded once for all of them
constexpr int kCssThreads = 256;
constexpr int kArgThreads = 1024;

// the scalars a pass and the host exchange; lives in device memory, read back once per swapping attempt
struct CssRec {
    double c;          // factor of the pending rank-one update (0: the update is a no-op)
    double score_j;    // score of the column being swapped out
    double score_star; // score of the arg-max
    int64_t winner;
    int32_t early;     // the score routine's early-exit flag
    int32_t stop;      // swapping: beta_j <= 0
    int32_t err;       // initial subset: S_resid(j, j) <= 1e-10
    int32_t pad;
};

template <class T>
__global__ __launch_bounds__(256) void css_diag_kernel(const T* __restrict__ A, int64_t lda, int64_t p, T* __restrict__ d) {
    const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j < p) d[j] = A[j + j * lda];
}

// "add column i to the set" (update_cov_resid_fwd): snapshots beta = S_resid[:, i] BEFORE the in-place pass, sets c = -1 / S_ii
// and the updated diagonal.  idx < 0: i is the arg-max winner in the record (greedy: no host round trip).  S_ii <= 0 (or, for
// the initial subset of swapping, S_ii <= 1e-10, which also raises the record's error flag) makes the update a no-op.
// Every thread takes the same decision from values this kernel does not write (rec->err is only ever raised when the decision
// is "no-op" already).
template <class T>
__global__ __launch_bounds__(256) void css_prep_add_kernel(const T* __restrict__ Sr, int64_t ld, int64_t p, int64_t idx,
                                                           int check_eps, T* __restrict__ beta, T* __restrict__ d,
                                                           uint8_t* __restrict__ mask, CssRec* rec) {
    const int64_t i = idx >= 0 ? idx : rec->winner;
    const T sii = Sr[i + i * ld];
    const bool bad = check_eps && sii <= T(1e-10);
    const bool noop = rec->err != 0 || bad || sii <= T(0);
    const T c = noop ? T(0) : T(-1) / sii;
    const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j < p) {
        const T b = Sr[j + i * ld];
        beta[j] = b;
        if (!noop) d[j] = fma(c, b * b, d[j]);
    }
    if (j == 0) {
        rec->c = double(c);
        rec->early = 0;
        rec->stop = 0;
        if (bad) rec->err = 1;
        mask[i] = 1;
    }
}

// "remove column j from the set" (solve_swapping): beta = A[:, j] - A[:, U] v, a gather-GEMV over the k - 1 other members of the
// original matrix (v in double, in the order of `sub`, entry jj skipped), c = +1 / beta_j.  beta_j <= 0 raises `stop` and makes
// the pass a no-op (the reference returns there).  Every thread recomputes beta_j (broadcast loads) instead of a second launch.
template <class T>
__device__ __forceinline__ T css_beta_row(const T* __restrict__ A, int64_t lda, int64_t r, int64_t j,
                                          const int64_t* __restrict__ sub, const double* __restrict__ v, int64_t k, int64_t jj) {
    double s = 0;
    for (int64_t m = 0; m < k; ++m)
        if (m != jj) s += v[m] * double(A[r + sub[m] * lda]);
    return T(double(A[r + j * lda]) - s);
}
template <class T>
__global__ __launch_bounds__(256) void css_prep_remove_kernel(const T* __restrict__ A, int64_t lda, int64_t p, int64_t j,
                                                              const int64_t* __restrict__ sub, const double* __restrict__ v,
                                                              int64_t k, int64_t jj, T* __restrict__ beta, T* __restrict__ d,
                                                              uint8_t* __restrict__ mask, CssRec* rec) {
    const T bj = css_beta_row<T>(A, lda, j, j, sub, v, k, jj);
    const bool stop = !(bj > T(0));
    const T c = stop ? T(0) : T(1) / bj;
    const int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r < p) {
        const T b = css_beta_row<T>(A, lda, r, j, sub, v, k, jj);
        beta[r] = b;
        if (!stop) d[r] = fma(c, b * b, d[r]);
    }
    if (r == 0) {
        rec->c = double(c);
        rec->early = 0;
        rec->stop = stop ? 1 : 0;
        if (!stop) mask[j] = 0;
    }
}

// The pass: S_resid[:, j] = fma(c, beta * beta_j, S_resid[:, j]) for every column j, and (SCORE) the score of column j from the
// updated values.  `d` is the UPDATED diagonal.  A thread handles V consecutive rows per step (V = 16 bytes' worth when p is a
// multiple of that, so that every column of the ld = p matrix starts 16-byte aligned; 1 otherwise).  Sums are taken in double in
// a fixed order: per thread over its rows, over the 64 lanes with wave_sum64, over the four wavefronts in order.
template <class T, int V>
struct alignas(V * sizeof(T)) CssVec {
    T v[V];
};
template <class T, int LOSS, bool SCORE, int V>
__global__ __launch_bounds__(256) void css_pass_kernel(T* __restrict__ Sr, int64_t ld, int64_t p, const T* __restrict__ beta,
                                                       const T* __restrict__ d, const uint8_t* __restrict__ mask, CssRec* rec,
                                                       double* __restrict__ scores) {
    constexpr int C = kCssCols;
    using Vec = CssVec<T, V>;
    const T c = T(rec->c);
    const bool upd = c != T(0);
    if (!upd && !SCORE) return;
    __shared__ double red[C][4];
    __shared__ int redbad[C][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t j0 = int64_t(blockIdx.x) * C; j0 < p; j0 += int64_t(gridDim.x) * C) {
        const int nc = int(p - j0 < C ? p - j0 : C);
        T bj[C], dj[C];
        bool skip[C]; // no score for this column: a member, or a non-positive diagonal (handled at the end)
#pragma unroll
        for (int cc = 0; cc < C; ++cc) {
            const bool in = cc < nc;
            bj[cc] = in ? beta[j0 + cc] : T(0);
            dj[cc] = in ? d[j0 + cc] : T(1);
            skip[cc] = !in || mask[j0 + cc] != 0 || !(dj[cc] > T(0));
        }
        double acc[C];
        int bad[C];
#pragma unroll
        for (int cc = 0; cc < C; ++cc) acc[cc] = 0, bad[cc] = 0;
        for (int64_t i = int64_t(threadIdx.x) * V; i < p; i += int64_t(kCssThreads) * V) { // (p is a multiple of V)
            const Vec bi = *reinterpret_cast<const Vec*>(beta + i);
            Vec di;
            bool mi[V];
#pragma unroll
            for (int e = 0; e < V; ++e) di.v[e] = T(1), mi[e] = false;
            if (SCORE && LOSS == CSS_SF) {
                di = *reinterpret_cast<const Vec*>(d + i);
#pragma unroll
                for (int e = 0; e < V; ++e) mi[e] = mask[i + e] != 0;
            }
#pragma unroll
            for (int cc = 0; cc < C; ++cc) {
                if (cc < nc) {
                    Vec* at = reinterpret_cast<Vec*>(Sr + i + (j0 + cc) * ld);
                    Vec s = *at;
                    if (upd) {
#pragma unroll
                        for (int e = 0; e < V; ++e) s.v[e] = fma(c, bi.v[e] * bj[cc], s.v[e]);
                        *at = s;
                    }
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        if (SCORE && LOSS == CSS_LS) acc[cc] += double(s.v[e]) * double(s.v[e]);
                        if (SCORE && LOSS == CSS_SF) {
                            if (!mi[e] && !skip[cc] && i + e != j0 + cc) {
                                const T r = di.v[e] - s.v[e] * s.v[e] / dj[cc];
                                if (r <= T(1e-10)) bad[cc] = 1;
                                else acc[cc] -= log(double(r));
                            }
                        }
                    }
                }
            }
        }
        if (SCORE) {
#pragma unroll
            for (int cc = 0; cc < C; ++cc) {
                const double w = wave_sum64(acc[cc]);
                const int b = __any(bad[cc]);
                if (lane == 0) red[cc][wave] = w, redbad[cc][wave] = b;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                const double inf = std::numeric_limits<double>::infinity();
#pragma unroll
                for (int cc = 0; cc < C; ++cc) {
                    if (cc < nc) {
                        const double tot = ((red[cc][0] + red[cc][1]) + red[cc][2]) + red[cc][3];
                        const bool anybad = (redbad[cc][0] | redbad[cc][1] | redbad[cc][2] | redbad[cc][3]) != 0;
                        const bool member = mask[j0 + cc] != 0;
                        double sc;
                        if (LOSS == CSS_LS) sc = skip[cc] ? 0.0 : tot / double(dj[cc]);
                        else if (member) sc = -inf;
                        else if (!(dj[cc] > T(0)) || anybad) sc = inf;
                        else sc = -log(double(dj[cc])) + tot;
                        scores[j0 + cc] = sc;
                        if (LOSS == CSS_SF && !member && sc == inf) rec->early = 1; // (every writer writes 1)
                    }
                }
            }
            __syncthreads();
        }
    }
}

// Masked arg-max over the p scores, one workgroup: members count as -inf, ties go to the lowest index (Eigen's maxCoeff).
// Writes the winner and the two scores of the swap decision into the record, the winner into slot[0] (greedy: the next entry of
// the subset), and gathers A[sub[m], winner] (m < k) and A[winner, winner] for the host's k x k algebra.
// MD: the scores are made here from the diagonal (see the header comment).
template <class T, bool MD>
__global__ __launch_bounds__(kArgThreads) void css_argmax_kernel(const double* __restrict__ scores, const T* __restrict__ d,
                                                                 const uint8_t* __restrict__ mask, int64_t p, int64_t j_swap,
                                                                 CssRec* rec, int64_t* slot, const T* __restrict__ A,
                                                                 int64_t lda, const int64_t* __restrict__ sub, int64_t k,
                                                                 T* __restrict__ gathered) {
    __shared__ double sv[kArgThreads];
    __shared__ int64_t si[kArgThreads];
    const int tid = threadIdx.x;
    const double inf = std::numeric_limits<double>::infinity();
    int64_t first = p; // MD: the first non-member whose score is >= -eps
    if (MD) {
        int64_t f = p;
        for (int64_t j = tid; j < p; j += kArgThreads)
            if (!mask[j] && -(d[j] > T(0) ? d[j] : T(0)) >= T(-1e-10)) {
                f = j;
                break;
            }
        si[tid] = f;
        __syncthreads();
        for (int h = kArgThreads / 2; h > 0; h >>= 1) {
            if (tid < h && si[tid + h] < si[tid]) si[tid] = si[tid + h];
            __syncthreads();
        }
        first = si[0];
        __syncthreads();
    }
    auto score_of = [&](int64_t j) -> double {
        if (!MD) return scores[j];
        return j == first ? 0.0 : -double(d[j] > T(0) ? d[j] : T(0));
    };
    double bv = -inf;
    int64_t bi = std::numeric_limits<int64_t>::max();
    for (int64_t j = tid; j < p; j += kArgThreads) {
        const double v = mask[j] ? -inf : score_of(j);
        if (v > bv || (v == bv && j < bi)) bv = v, bi = j;
    }
    sv[tid] = bv;
    si[tid] = bi;
    __syncthreads();
    for (int h = kArgThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double v = sv[tid + h];
            const int64_t j = si[tid + h];
            if (v > sv[tid] || (v == sv[tid] && j < si[tid])) sv[tid] = v, si[tid] = j;
        }
        __syncthreads();
    }
    int64_t w = si[0];
    if (w < 0 || w >= p) w = 0; // (every score a NaN)
    if (tid == 0) {
        rec->winner = w;
        rec->score_star = score_of(w);
        rec->score_j = j_swap >= 0 ? score_of(j_swap) : 0.0;
        if (MD) rec->early = first < p ? 1 : 0;
        if (slot) *slot = w;
    }
    if (gathered) {
        for (int64_t m = tid; m < k; m += kArgThreads) gathered[m] = A[sub[m] + w * lda];
        if (tid == 0) gathered[k] = A[w + w * lda];
    }
}

// out[a + b * k] = A[sub[a], sub[b]]
template <class T>
__global__ __launch_bounds__(256) void css_gather_kernel(const T* __restrict__ A, int64_t lda, const int64_t* __restrict__ sub,
                                                         int64_t k, T* __restrict__ out) {
    const int64_t a = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a >= k) return;
    for (int64_t b = blockIdx.y; b < k; b += gridDim.y) out[a + b * k] = A[sub[a] + sub[b] * lda];
}

unsigned blocks_for(int64_t n, int per) { return unsigned((n + per - 1) / per); }

} // namespace
} // namespace ahip

using namespace ahip;

struct adelie_hip_css_result {
    int dtype = ADELIE_HIP_F64, device = 0;
    int64_t p = 0, k = 0;
    bool has_resid = false;
    DevBuf<char> Sr; // (p, p) column-major, ld = p, of dtype
    std::vector<char> diag; // (p,) of dtype
    std::vector<int64_t> subset;
    std::vector<double> L_T; // (k, k) column-major, lower
    int64_t n_updates = 0, n_swaps = 0, n_attempts = 0;
    int early = 0;
    double total_time = 0;
    std::string error;
};

namespace {

// ---- the k x k algebra of swapping, host, double, row-major lower triangles -----------------------------------------------------
// L L^T = S for the symmetric (k, k) S; a non-positive pivot is stored as 0 and its column left zero (the caller tests the diagonal)
void chol_lower(const std::vector<double>& S, int64_t k, std::vector<double>& L) {
    L.assign(size_t(k) * k, 0.0);
    for (int64_t a = 0; a < k; ++a) {
        for (int64_t b = 0; b <= a; ++b) {
            double s = S[a * k + b];
            for (int64_t m = 0; m < b; ++m) s -= L[a * k + m] * L[b * k + m];
            if (a == b) L[a * k + a] = s > 0 ? std::sqrt(s) : 0.0;
            else L[a * k + b] = L[b * k + b] > 0 ? s / L[b * k + b] : 0.0;
        }
    }
}
// L L^T += x x^T for the lower (n, n) L (leading dimension n); x is overwritten
void chol_rank_one(std::vector<double>& L, int64_t n, std::vector<double>& x) {
    for (int64_t i = 0; i < n; ++i) {
        const double lii = L[i * n + i];
        const double r = std::hypot(lii, x[i]);
        if (!(r > 0) || !(lii != 0)) continue;
        const double c = r / lii, s = x[i] / lii;
        L[i * n + i] = r;
        for (int64_t m = i + 1; m < n; ++m) {
            L[m * n + i] = (L[m * n + i] + s * x[m]) / c;
            x[m] = c * x[m] - s * L[m * n + i];
        }
    }
}
void solve_lower(const std::vector<double>& L, int64_t n, std::vector<double>& b) { // L y = b
    for (int64_t a = 0; a < n; ++a) {
        double s = b[a];
        for (int64_t m = 0; m < a; ++m) s -= L[a * n + m] * b[m];
        b[a] = s / L[a * n + a];
    }
}
void solve_lower_t(const std::vector<double>& L, int64_t n, std::vector<double>& b) { // L^T y = b
    for (int64_t a = n - 1; a >= 0; --a) {
        double s = b[a];
        for (int64_t m = a + 1; m < n; ++m) s -= L[m * n + a] * b[m];
        b[a] = s / L[a * n + a];
    }
}

struct Pinned {
    void* p = nullptr;
    size_t bytes = 0;
    explicit Pinned(size_t n) : bytes((n + 4095) / 4096 * 4096) {
        p = HostPool::take(bytes, hipHostMallocDefault);
        if (!p) throw core_error("adelie_hip: hipHostMalloc failed");
    }
    ~Pinned() { HostPool::give(p, bytes, hipHostMallocDefault); }
};

template <class T>
struct CssSolver {
    adelie_hip_design* A;
    adelie_hip_css_result* res;
    int loss;
    int64_t p, lda;
    hipStream_t s;
    const T* Ad;
    T* Sr;
    DevBuf<T> beta, d, gathered;
    DevBuf<double> scores, v;
    DevBuf<uint8_t> mask;
    DevBuf<int64_t> sub;
    DevBuf<CssRec> rec;

    CssSolver(adelie_hip_design* A_, adelie_hip_css_result* r, int loss_) : A(A_), res(r), loss(loss_) {
        p = A->p;
        lda = A->ld;
        s = A->stream;
        Ad = static_cast<const T*>(A->X);
    }

    // k_host: the subset size whose k x k algebra runs on the host (swapping; 0 for greedy)
    void init(int64_t k, int64_t k_host) {
        Sr = reinterpret_cast<T*>(res->Sr.reserve(size_t(p) * size_t(p) * sizeof(T)));
        beta.reserve(p), d.reserve(p), scores.reserve(p), mask.reserve(p), rec.reserve(1);
        sub.reserve(std::max<int64_t>(k, 1)), v.reserve(std::max<int64_t>(k_host, 1));
        gathered.reserve(size_t(k_host) * k_host + k_host + 1);
        AHIP_CHECK(hipMemcpy2DAsync(Sr, size_t(p) * sizeof(T), Ad, size_t(lda) * sizeof(T), size_t(p) * sizeof(T), size_t(p),
                                    hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL((css_diag_kernel<T>), dim3(blocks_for(p, 256)), dim3(256), 0, s, Ad, lda, p, d.p);
        AHIP_CHECK(hipMemsetAsync(mask.p, 0, size_t(p), s));
        AHIP_CHECK(hipMemsetAsync(beta.p, 0, size_t(p) * sizeof(T), s));
        AHIP_CHECK(hipMemsetAsync(rec.p, 0, sizeof(CssRec), s));
        res->has_resid = true;
    }
    void prep_add(int64_t idx, int check_eps) {
        hipLaunchKernelGGL((css_prep_add_kernel<T>), dim3(blocks_for(p, 256)), dim3(256), 0, s, Sr, p, p, idx, check_eps, beta.p,
                           d.p, mask.p, rec.p);
    }
    template <int LOSS, bool SCORE>
    void pass_t() {
        const int64_t nb = std::min<int64_t>((p + kCssCols - 1) / kCssCols, int64_t(1) << 20);
        constexpr int V16 = 16 / int(sizeof(T));
        if (p % V16 == 0)
            hipLaunchKernelGGL((css_pass_kernel<T, LOSS, SCORE, V16>), dim3(unsigned(nb)), dim3(kCssThreads), 0, s, Sr, p, p, beta.p,
                               d.p, mask.p, rec.p, scores.p);
        else
            hipLaunchKernelGGL((css_pass_kernel<T, LOSS, SCORE, 1>), dim3(unsigned(nb)), dim3(kCssThreads), 0, s, Sr, p, p, beta.p,
                               d.p, mask.p, rec.p, scores.p);
    }
    // min_det's scores come from the diagonal alone (made in the arg-max kernel): its passes never score
    void pass(bool score) {
        if (!score || loss == CSS_MD) pass_t<CSS_MD, false>();
        else if (loss == CSS_LS) pass_t<CSS_LS, true>();
        else pass_t<CSS_SF, true>();
    }
    void argmax(int64_t j_swap, int64_t* slot, int64_t k_gather) {
        T* g = k_gather > 0 ? gathered.p : nullptr;
        if (loss == CSS_MD)
            hipLaunchKernelGGL((css_argmax_kernel<T, true>), dim3(1), dim3(kArgThreads), 0, s, scores.p, d.p, mask.p, p, j_swap,
                               rec.p, slot, Ad, lda, sub.p, k_gather, g);
        else
            hipLaunchKernelGGL((css_argmax_kernel<T, false>), dim3(1), dim3(kArgThreads), 0, s, scores.p, d.p, mask.p, p, j_swap,
                               rec.p, slot, Ad, lda, sub.p, k_gather, g);
    }
    void finish() {
        res->diag.resize(size_t(p) * sizeof(T));
        AHIP_CHECK(hipMemcpyAsync(res->diag.data(), d.p, size_t(p) * sizeof(T), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
        AHIP_CHECK(hipGetLastError());
    }

    // solve_greedy: enqueued without a host synchronisation inside the loop; the next update reads the winner from the record
    void greedy(int64_t k) {
        init(k, 0);
        if (k > 0) pass(true); // the scores of A itself (c = 0: nothing is written)
        for (int64_t t = 0; t < k; ++t) {
            argmax(-1, sub.p + t, 0);
            prep_add(-1, 0);
            pass(t + 1 < k);
            ++res->n_updates;
        }
        res->subset.resize(size_t(k));
        if (k) AHIP_CHECK(hipMemcpyAsync(res->subset.data(), sub.p, size_t(k) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        finish();
    }

    // solve_swapping: one device -> host read per attempt (the record and k + 1 entries of A)
    void swapping(const int64_t* subset0, int64_t k, int64_t max_iters) {
        std::vector<int64_t>& subset = res->subset;
        subset.assign(subset0, subset0 + k);
        if (k <= 0 || k >= p) return;
        constexpr double eps = 1e-10;
        init(k, k);
        Pinned up(size_t(k) * (sizeof(int64_t) + sizeof(double)));
        Pinned down(sizeof(CssRec) + (size_t(k) * k + k + 1) * sizeof(T));
        int64_t* h_sub = static_cast<int64_t*>(up.p);
        double* h_v = reinterpret_cast<double*>(h_sub + k);
        CssRec* h_rec = static_cast<CssRec*>(down.p);
        T* h_g = reinterpret_cast<T*>(h_rec + 1);

        // residual covariance w.r.t. T, with the independence check on the device (no host wait per column)
        for (int64_t jj = 0; jj < k; ++jj) {
            prep_add(subset[jj], 1);
            pass(false);
            ++res->n_updates;
        }
        std::memcpy(h_sub, subset.data(), size_t(k) * sizeof(int64_t));
        AHIP_CHECK(hipMemcpyAsync(sub.p, h_sub, size_t(k) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL((css_gather_kernel<T>), dim3(blocks_for(k, 256), unsigned(std::min<int64_t>(k, 65535))), dim3(256), 0, s,
                           Ad, lda, sub.p, k, gathered.p);
        AHIP_CHECK(hipMemcpyAsync(h_g, gathered.p, size_t(k) * k * sizeof(T), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipMemcpyAsync(h_rec, rec.p, sizeof(CssRec), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
        const char* dependent = "adelie_core: Initial subset are not linearly independent columns.";
        if (h_rec->err) {
            res->error = dependent;
            return finish();
        }
        // ST[a][b] = A(subset[a], subset[b]); kept on the host and patched when a swap happens
        std::vector<double> ST(size_t(k) * k), L_T, L_U(size_t(k - 1) * (k - 1)), x(size_t(k - 1)), w(size_t(k - 1));
        for (int64_t a = 0; a < k; ++a)
            for (int64_t b = 0; b <= a; ++b) ST[a * k + b] = ST[b * k + a] = double(h_g[a + b * k]);
        chol_lower(ST, k, L_T);
        auto store_LT = [&]() {
            res->L_T.assign(size_t(k) * k, 0.0);
            for (int64_t a = 0; a < k; ++a)
                for (int64_t b = 0; b <= a; ++b) res->L_T[a + b * k] = L_T[a * k + b];
        };
        store_LT();
        for (int64_t a = 0; a < k; ++a)
            if (L_T[a * k + a] <= eps) {
                res->error = dependent;
                return finish();
            }

        const int64_t n = k - 1;
        int64_t n_consec_keep = 0;
        for (int64_t it = 0; it < max_iters; ++it) {
            for (int64_t jj = 0; jj < k; ++jj) {
                // T = [subset[jj], ..., subset[k-1], subset[0], ..., subset[jj-1]], U = T[1:]
                const int64_t j = subset[jj];
                auto pos = [&](int64_t i) { return (jj + 1 + i) % k; }; // position in `subset` of U's i-th member
                // L_U from L_T: drop T's first member = a rank-one update of the trailing block with L_T's first column
                for (int64_t a = 0; a < n; ++a) {
                    for (int64_t b = 0; b < n; ++b) L_U[a * n + b] = b <= a ? L_T[(a + 1) * k + (b + 1)] : 0.0;
                    x[a] = L_T[(a + 1) * k];
                }
                chol_rank_one(L_U, n, x);
                // v = Sigma_U^-1 Sigma_{U, j}, scattered to the order of `subset`
                for (int64_t i = 0; i < n; ++i) w[i] = ST[pos(i) * k + jj];
                solve_lower(L_U, n, w);
                solve_lower_t(L_U, n, w);
                for (int64_t i = 0; i < n; ++i) h_v[pos(i)] = w[i];
                h_v[jj] = 0;
                std::memcpy(h_sub, subset.data(), size_t(k) * sizeof(int64_t));
                AHIP_CHECK(hipMemcpyAsync(sub.p, h_sub, size_t(k) * sizeof(int64_t), hipMemcpyHostToDevice, s));
                AHIP_CHECK(hipMemcpyAsync(v.p, h_v, size_t(k) * sizeof(double), hipMemcpyHostToDevice, s));
                hipLaunchKernelGGL((css_prep_remove_kernel<T>), dim3(blocks_for(p, 256)), dim3(256), 0, s, Ad, lda, p, j, sub.p, v.p,
                                   k, jj, beta.p, d.p, mask.p, rec.p);
                pass(true);
                argmax(j, nullptr, k);
                AHIP_CHECK(hipMemcpyAsync(h_rec, rec.p, sizeof(CssRec), hipMemcpyDeviceToHost, s));
                AHIP_CHECK(hipMemcpyAsync(h_g, gathered.p, size_t(k + 1) * sizeof(T), hipMemcpyDeviceToHost, s));
                AHIP_CHECK(hipStreamSynchronize(s)); // the one round trip of an attempt
                if (h_rec->stop) { // beta_j <= 0: numerically unstable, terminate (S_resid was not touched)
                    store_LT();
                    return finish();
                }
                ++res->n_updates;
                ++res->n_attempts;
                const bool early = h_rec->early != 0;
                res->early = early;
                if (h_rec->score_j < h_rec->score_star) {
                    const int64_t js = h_rec->winner;
                    subset[jj] = js;
                    for (int64_t m = 0; m < k; ++m)
                        if (m != jj) ST[m * k + jj] = ST[jj * k + m] = double(h_g[m]);
                    ST[jj * k + jj] = double(h_g[k]);
                    n_consec_keep = 0;
                    ++res->n_swaps;
                } else {
                    ++n_consec_keep;
                }
                // L_T of the rotated T = [U, subset[jj]]: L_U on top, a new last row
                for (int64_t i = 0; i < n; ++i) w[i] = ST[pos(i) * k + jj];
                solve_lower(L_U, n, w);
                double sq = 0;
                for (int64_t i = 0; i < n; ++i) sq += w[i] * w[i];
                std::fill(L_T.begin(), L_T.end(), 0.0);
                for (int64_t a = 0; a < n; ++a)
                    for (int64_t b = 0; b <= a; ++b) L_T[a * k + b] = L_U[a * n + b];
                for (int64_t i = 0; i < n; ++i) L_T[n * k + i] = w[i];
                const double last = std::sqrt(std::max(ST[jj * k + jj] - sq, 0.0));
                L_T[n * k + n] = last;
                // residual covariance w.r.t. the new T; it needs no scores, the next attempt starts with a remove
                prep_add(subset[jj], 0);
                pass(false);
                ++res->n_updates;
                if (n_consec_keep >= k || early || last <= eps) {
                    store_LT();
                    return finish();
                }
            }
        }
        store_LT();
        res->error = "adelie_core solver: Maximum swapping cycles reached!";
        finish();
    }
};

template <class T>
void css_run(adelie_hip_design* A, const adelie_hip_css_args* a, adelie_hip_css_result* res) {
    CssSolver<T> sv(A, res, a->loss);
    try {
        if (a->method == ADELIE_HIP_CSS_GREEDY) sv.greedy(a->subset_size);
        else sv.swapping(a->subset, a->n_subset, a->max_iters);
    } catch (...) {
        (void)hipStreamSynchronize(A->stream); // the buffers are parked by the destructors
        throw;
    }
}

} // namespace

extern "C" {

int adelie_hip_css_cov_solve(adelie_hip_design* A, const adelie_hip_css_args* a, adelie_hip_css_result** out) {
    adelie_hip_css_result* res = nullptr;
    try {
        if (!A || !a || !out) throw make_core_error("null argument.");
        if (!A->cov) throw make_core_error("S must be a covariance matrix (matrix.dense(method=\"cov\")).");
        if (A->cov_csc()) // (the solve keeps a dense (p, p) residual of S anyway)
            throw make_core_error("css_cov works on a dense covariance matrix: use matrix.sparse(..., method=\"cov\", resident=\"dense\").");
        // state_css_cov.ipp:15-57
        if (A->n != A->p) throw make_core_error("S must be (p, p).");
        if (a->subset_size < 0 || a->subset_size > A->p) throw make_core_error("subset_size must be <= p.");
        const bool swapping = a->method == ADELIE_HIP_CSS_SWAPPING;
        if (!swapping && a->method != ADELIE_HIP_CSS_GREEDY) throw make_core_error("method must be greedy or swapping.");
        if (a->loss < 0 || a->loss > 2) throw make_core_error("unknown loss.");
        if (a->n_subset < 0 || (a->n_subset && !a->subset)) throw make_core_error("null argument.");
        if (swapping && a->subset_size != a->n_subset)
            throw make_core_error("subset must be (subset_size,) if method is \"swapping\".");
        if (swapping)
            for (int64_t i = 0; i < a->n_subset; ++i)
                if (a->subset[i] < 0 || a->subset[i] >= A->p) throw make_core_error("subset must be in the range [0, p).");
        if (!swapping && a->n_subset) throw make_core_error("subset must be empty if method is \"greedy\".");
        if (a->n_threads < 1) throw make_core_error("n_threads must be >= 1.");
        AHIP_CHECK(hipSetDevice(A->device));
        res = new adelie_hip_css_result;
        res->dtype = A->dtype;
        res->device = A->device;
        res->p = A->p;
        res->k = a->subset_size;
        const auto t0 = std::chrono::steady_clock::now();
        DTYPE_DISPATCH(A, css_run<T>(A, a, res))
        res->total_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *out = res;
    } catch (const std::exception& e) {
        delete res;
        set_last_error(e.what());
        return 1;
    }
    return 0;
}

int adelie_hip_css_result_destroy(adelie_hip_css_result* r) {
    if (r) (void)hipSetDevice(r->device); // (its buffer is parked per device)
    delete r;
    return 0;
}

int64_t adelie_hip_css_result_size(const adelie_hip_css_result* r, int which) {
    if (!r) return -1;
    switch (which) {
        case ADELIE_HIP_CSS_SUBSET: return int64_t(r->subset.size());
        case ADELIE_HIP_CSS_S_RESID: return r->has_resid ? r->p * r->p : 0;
        case ADELIE_HIP_CSS_S_RESID_DIAG: return r->has_resid ? r->p : 0;
        case ADELIE_HIP_CSS_L_T: return int64_t(r->L_T.size());
    }
    return -1;
}

int adelie_hip_css_result_copy(const adelie_hip_css_result* r, int which, void* out, int64_t cap) {
    ABI_TRY
    const int64_t size = adelie_hip_css_result_size(r, which);
    if (size < 0 || !out) throw make_core_error("unknown result vector.");
    const size_t n = size_t(std::min(size, cap));
    const size_t es = r->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
    if (!n) return 0;
    switch (which) {
        case ADELIE_HIP_CSS_SUBSET: std::memcpy(out, r->subset.data(), n * sizeof(int64_t)); break;
        case ADELIE_HIP_CSS_S_RESID:
            AHIP_CHECK(hipSetDevice(r->device));
            AHIP_CHECK(hipMemcpy(out, r->Sr.p, n * es, hipMemcpyDeviceToHost));
            break;
        case ADELIE_HIP_CSS_S_RESID_DIAG: std::memcpy(out, r->diag.data(), n * es); break;
        case ADELIE_HIP_CSS_L_T: std::memcpy(out, r->L_T.data(), n * sizeof(double)); break;
    }
    ABI_CATCH
}

double adelie_hip_css_result_scalar(const adelie_hip_css_result* r, int which) {
    if (!r) return 0;
    switch (which) {
        case ADELIE_HIP_CSS_N_UPDATES: return double(r->n_updates);
        case ADELIE_HIP_CSS_N_SWAPS: return double(r->n_swaps);
        case ADELIE_HIP_CSS_N_ATTEMPTS: return double(r->n_attempts);
        case ADELIE_HIP_CSS_EARLY_EXIT: return double(r->early);
        case ADELIE_HIP_CSS_TOTAL_TIME: return r->total_time;
    }
    return 0;
}

const char* adelie_hip_css_result_error(const adelie_hip_css_result* r) { return r ? r->error.c_str() : ""; }

} // extern "C"
