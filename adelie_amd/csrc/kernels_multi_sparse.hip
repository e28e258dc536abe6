// kernels_multi_sparse.hip — the multi-response view [1 (x) I_K, X (x) I_K] over a design kept sparse (gfx950 / CDNA4).
//
// The reference composes MatrixNaiveKroneckerEye over MatrixNaiveSparse (matrix_naive_kronecker_eye.ipp over
// matrix_naive_sparse.ipp): every view column walks the base column's entries again.  Here the base's compressed columns and
// rows (CscView, kernels_sparse.hip) are read once per chunk of KT <= 8 responses; nothing of size nb x pb exists.  Vectors of
// nb K values are response-major as in kernels_multi.hip; extended feature u < icpt is the column of ones, which the base does
// not store: every kernel serves it in a code path of its own.
//
//   sweep   out[u K + l] = x_u . v_l.  The single-response sweep is bound by one gather per stored entry (kernels_sparse.hip), so
//           K gathers into K response-major vectors would cost what K sweeps cost.  The vectors are first interleaved per chunk,
//           vt[(q nb + i) KT + kk] = v[(q KT + kk) nb + i] (nb K values moved, against 12 bytes per stored entry), and the sweep
//           gathers ONE aligned KT-wide element per stored entry: index and value are read once, KT accumulators per lane.
//           16 lanes per (column, tile or row block) segment.  Tile height: the design's own tile-major copy is used where it
//           exists (CscView::nt > 0, th rows = 128 KB of ONE vector).  KT interleaved vectors of th rows are KT x 128 KB and do
//           not fit the 160 KB of LDS, and a shorter tile would need a second copy of the entries, so the tile of vt is left to
//           L2: th rows of a chunk are at most 1 MB of the 4 MB an XCD has, and workgroups are dispatched tile by tile
//           (blockIdx.y).  Without the copy the row blocks of CscView::bptr bound the gathered slice the same way.  Partial sums
//           per tile / row block, added in block order by the reduce kernel; the ones feature is sum_i v_l[i] in the order of
//           vec_sum_kernel.  No atomics.
//   step    phase (A)  r_l[row] -= x Delta[u, l]  over the stored entries of the changed features: one workgroup per feature slot
//           (multi_slots.hpp: the entries of one feature for several responses share one pass over its entries).  Two changed
//           features may share a row: phase (A) adds with hardware floating-point atomics on global memory, exactly as
//           csc_panel_update_kernel does, so runs agree to rounding and not bit for bit where that happens.  The ones feature is
//           a dense pass over all nb rows spread over the launch.
//           phase (B)  g[c] = sum_e x_e w_l[row_e] r_l[row_e]: one workgroup per feature slot of the block, the four wavefronts'
//           sums combined in a fixed order, straight into the block's gradient; the ones feature is a dense two-stage sum.
//   Gram    sum_i w_i x_ia x_ib over a block's distinct extended features by the LDS hash join of csc_block_gram_kernel, the
//           ones feature added: 1 w x_u = sum_e x_e w[row_e], 1 w 1 = sum w.  The result feeds launch_multi_expand unchanged.
//   axpy    out[:, l] += sign coef[m] x_u (rollback): coefficients scattered into a zeroed ((pb + icpt) K) vector, then one pass
//           over the compressed rows for all K responses; fixed order.
#include "kernels.hpp"
#include "wavered.hpp"
#include "multi_shape.hpp"
#include "multi_slots.hpp"

#include <algorithm>

namespace ahip {

namespace {

constexpr int MAXB = kMultiBlock; // entries of a panel block
constexpr int ONES_PARTS = 64;    // row chunks of the ones feature's gradient
static_assert(MAXB == 128, "the kernels below are written for this");

template <class T, int KT>
struct alignas(sizeof(T) * KT) VecK {
    T v[KT];
};

// ---- sweep --------------------------------------------------------------------------------------------------------------------
template <class T, int KT>
__global__ __launch_bounds__(256) void msp_interleave_kernel(const T* __restrict__ v, int64_t nb, int K, T* __restrict__ vt) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const int q = blockIdx.y;
    if (i >= nb) return;
    VecK<T, KT> x;
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
        const int l = q * KT + kk;
        x.v[kk] = l < K ? v[int64_t(l) * nb + i] : T(0);
    }
    reinterpret_cast<VecK<T, KT>*>(vt)[int64_t(q) * nb + i] = x;
}

// grid (groups of 16 base columns, tiles or row blocks, response chunks); TILE: the tile-major copy
template <class T, int KT, bool TILE>
__global__ __launch_bounds__(256) void msp_sweep_kernel(CscView<T> X, int K, int icpt, const T* __restrict__ vt, T* __restrict__ part) {
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int64_t c = (int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    const int y = blockIdx.y, q = blockIdx.z;
    const bool valid = c < X.p;
    int64_t b = 0, e = 0;
    if (valid) {
        if (TILE) {
            const int64_t* tp = X.tptr + int64_t(y) * (X.p + 1) + c;
            b = tp[0], e = tp[1];
        } else if (X.nb > 1) {
            const int64_t* bp = X.bptr + c * (X.nb + 1) + y;
            b = bp[0], e = bp[1];
        } else {
            b = X.cptr[c], e = X.cptr[c + 1];
        }
    }
    const VecK<T, KT>* vq = reinterpret_cast<const VecK<T, KT>*>(vt) + int64_t(q) * X.n;
    const int64_t row0 = TILE ? int64_t(y) * X.th : 0;
    T acc[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) acc[kk] = T(0);
#pragma unroll 2
    for (int64_t t = b + sub; t < e; t += 16) {
        const T x = TILE ? X.tval[t] : X.cval[t];
        const int64_t row = TILE ? row0 + int64_t(X.trow[t]) : int64_t(X.cidx[t]);
        const VecK<T, KT> s = vq[row];
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) acc[kk] = fma(x, s.v[kk], acc[kk]);
    }
    const int64_t nfeat = X.p + icpt;
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) { // fixed-order sum over the segment's 16 lanes
        T a = acc[kk];
        a += pdpp<0xB1>(a);  // quad_perm [1,0,3,2]
        a += pdpp<0x4E>(a);  // quad_perm [2,3,0,1]
        a += pdpp<0x141>(a); // row_half_mirror
        a += pdpp<0x140>(a); // row_mirror
        const int l = q * KT + kk;
        if (valid && sub == 0 && l < K) part[(int64_t(y) * nfeat + c + icpt) * K + l] = a;
    }
}

// sums[l * kVecSumScratch] = sum_i v_l[i] in the order of vec_sum_kernel (kernels_sparse.hip), one grid row per response
template <class T>
__global__ __launch_bounds__(256) void msp_vec_sum_kernel(const T* __restrict__ v, int64_t nb, T* __restrict__ sums, int stage) {
    __shared__ T sh[256];
    const T* vl = v + int64_t(blockIdx.y) * nb;
    T* out = sums + int64_t(blockIdx.y) * kVecSumScratch;
    T a = T(0);
    if (stage == 0) {
        const int64_t chunk = (nb + 255) / 256, b0 = int64_t(blockIdx.x) * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
        for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) a += vl[i];
    } else {
        a = out[8 + threadIdx.x];
    }
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (int(threadIdx.x) < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[stage == 0 ? 8 + blockIdx.x : 0] = sh[0];
}

template <class T>
__global__ __launch_bounds__(256) void msp_sweep_reduce_kernel(const T* __restrict__ part, int nparts, const T* __restrict__ sums,
                                                                int64_t nfeat, int K, int icpt, T* __restrict__ out) {
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= nfeat * K) return;
    if (k < int64_t(icpt) * K) {
        out[k] = sums[k * kVecSumScratch];
        return;
    }
    T acc = part[k];
    for (int b = 1; b < nparts; ++b) acc += part[int64_t(b) * nfeat * K + k];
    out[k] = acc;
}

// ---- panel step ---------------------------------------------------------------------------------------------------------------
// phase (A): grid (workgroups, response chunks); a workgroup takes every gridDim.x-th feature slot of the changed list
template <class T, int KT>
__global__ __launch_bounds__(256) void msp_update_kernel(CscView<T> X, int K, int icpt, const int32_t* __restrict__ dcol,
                                                         const T* __restrict__ dlt, const int32_t* __restrict__ nz_dev,
                                                         T* __restrict__ r) {
    __shared__ int featA[MAXB];
    __shared__ T dA[MAXB * KT];
    __shared__ int ns_sh;
    const int nz = min(nz_dev[0], MAXB);
    if (nz <= 0) return;
    const int tid = threadIdx.x, l0 = blockIdx.y * KT;
    for (int q = tid; q < MAXB * KT; q += 256) dA[q] = T(0);
    __syncthreads();
    if (tid < 64) {
        const int ns = build_slots(dcol, nz, K, featA, tid, [&](int m, int slot, int l) {
            if (l >= l0 && l < l0 + KT) dA[slot * KT + (l - l0)] = dlt[m];
        });
        if (tid == 0) ns_sh = ns;
    }
    __syncthreads();
    const int ns = ns_sh;
    const int64_t nb = X.n;
    for (int s = 0; s < ns; ++s) {
        const int u = featA[s];
        const bool ones = u < icpt;
        if (!ones && (s % int(gridDim.x)) != int(blockIdx.x)) continue;
        T d[KT];
        bool any = false;
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            d[kk] = dA[s * KT + kk];
            any = any || d[kk] != T(0);
        }
        if (!any) continue;
        if (ones) { // every row, spread over the launch
            for (int64_t i = int64_t(blockIdx.x) * 256 + tid; i < nb; i += int64_t(gridDim.x) * 256)
#pragma unroll
                for (int kk = 0; kk < KT; ++kk)
                    if (d[kk] != T(0)) unsafeAtomicAdd(r + int64_t(l0 + kk) * nb + i, -d[kk]);
            continue;
        }
        const int64_t c = u - icpt, e1 = X.cptr[c + 1];
        for (int64_t e = X.cptr[c] + tid; e < e1; e += 256) {
            const T x = X.cval[e];
            T* rr = r + X.cidx[e];
#pragma unroll
            for (int kk = 0; kk < KT; ++kk)
                if (d[kk] != T(0)) unsafeAtomicAdd(rr + int64_t(l0 + kk) * nb, -x * d[kk]);
        }
    }
}

// phase (B): grid (feature slots of the block, response chunks)
template <class T, int KT>
__global__ __launch_bounds__(256) void msp_grad_kernel(CscView<T> X, int K, int icpt, const T* __restrict__ w, const T* __restrict__ r,
                                                       const int32_t* __restrict__ cols, int nbc, T* __restrict__ gblk) {
    __shared__ int featB[2 * MAXB];
    __shared__ int valB[2 * MAXB * KT];
    __shared__ T red[4][KT];
    __shared__ int ns_sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l0 = blockIdx.y * KT;
    for (int q = tid; q < 2 * MAXB * KT; q += 256) valB[q] = -1;
    __syncthreads();
    if (tid < 64) {
        const int ns = build_slots(cols, nbc, K, featB, tid, [&](int m, int slot, int l) {
            if (l >= l0 && l < l0 + KT) valB[slot * KT + (l - l0)] = m;
        });
        if (tid == 0) ns_sh = ns;
    }
    __syncthreads();
    const int s = blockIdx.x;
    if (s >= ns_sh) return;
    const int u = featB[s];
    if (u < icpt) return; // (the ones feature: msp_ones_grad_kernel)
    int vb[KT];
    bool any = false;
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
        vb[kk] = valB[s * KT + kk];
        any = any || vb[kk] >= 0;
    }
    if (!any) return;
    const int64_t nb = X.n, c = u - icpt, e1 = X.cptr[c + 1];
    T acc[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) acc[kk] = T(0);
    for (int64_t e = X.cptr[c] + tid; e < e1; e += 256) {
        const T x = X.cval[e];
        const int64_t i = X.cidx[e];
#pragma unroll
        for (int kk = 0; kk < KT; ++kk)
            if (vb[kk] >= 0) {
                const int64_t q = int64_t(l0 + kk) * nb + i;
                acc[kk] = fma(x, w[q] * r[q], acc[kk]);
            }
    }
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
        const T a = wave_sum64(acc[kk]);
        if (lane == 0) red[wv][kk] = a;
    }
    __syncthreads();
    if (tid < KT && valB[s * KT + tid] >= 0) gblk[valB[s * KT + tid]] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// the ones feature's entries of the block: g[c] = sum_i w_l[i] r_l[i].  stage 0: grid (ONES_PARTS row chunks, response chunks)
// -> work[l * ONES_PARTS + chunk]; stage 1: grid (1, response chunks) adds the chunk sums in order.  Both find the entries
// themselves and return when the block has none.
template <class T, int KT>
__global__ __launch_bounds__(256) void msp_ones_grad_kernel(int64_t nb, int K, const T* __restrict__ w, const T* __restrict__ r,
                                                            const int32_t* __restrict__ cols, int nbc, T* __restrict__ work,
                                                            T* __restrict__ gblk, int stage) {
    __shared__ int pos[KT];
    __shared__ T sh[256];
    const int tid = threadIdx.x, l0 = blockIdx.y * KT;
    if (tid < KT) pos[tid] = -1;
    __syncthreads();
    for (int m = tid; m < nbc; m += 256) { // (u < icpt = 1: the view column is the response)
        const int c = cols[m];
        if (c < K && c >= l0 && c < l0 + KT) pos[c - l0] = m;
    }
    __syncthreads();
    for (int kk = 0; kk < KT; ++kk) {
        if (pos[kk] < 0) continue; // (uniform)
        const int l = l0 + kk;
        if (stage == 1) {
            if (tid == 0) {
                T a = work[int64_t(l) * ONES_PARTS];
                for (int b = 1; b < ONES_PARTS; ++b) a += work[int64_t(l) * ONES_PARTS + b];
                gblk[pos[kk]] = a;
            }
            continue;
        }
        const int64_t chunk = (nb + ONES_PARTS - 1) / ONES_PARTS, b0 = int64_t(blockIdx.x) * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
        T a = T(0);
        for (int64_t i = b0 + tid; i < b1; i += 256) a = fma(w[int64_t(l) * nb + i], r[int64_t(l) * nb + i], a);
        __syncthreads();
        sh[tid] = a;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h) sh[tid] += sh[tid + h];
            __syncthreads();
        }
        if (tid == 0) work[int64_t(l) * ONES_PARTS + blockIdx.x] = sh[0];
    }
}

// ---- Gram over a block's distinct extended features --------------------------------------------------------------------------------
// One workgroup per column b of the list (csc_block_gram_kernel's scheme): the stored entries of feature b go into an LDS hash
// table (row -> w[row] * value, long columns in chunks), every column a >= b probes it, one wavefront per column.  Against the
// ones feature nothing is joined: x_u' W 1 is the sum of w[row] * value over x_u's entries, 1' W 1 is wsum[0].
constexpr int HJ_SLOTS = 4096, HJ_CHUNK = 2560; // (load factor <= 0.625)
template <class T>
__global__ __launch_bounds__(256) void msp_gram_kernel(CscView<T> X, int icpt, const T* __restrict__ w, const int32_t* __restrict__ ucols,
                                                       int M, const T* __restrict__ wsum, T* __restrict__ C, int64_t ldc) {
    __shared__ int32_t keys[HJ_SLOTS];
    __shared__ T vals[HJ_SLOTS];
    __shared__ T accs[MAXB];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ub = ucols[b];
    if (tid < MAXB) accs[tid] = T(0);
    __syncthreads();
    // sum_e x_e w[row_e] over entries [e0, e1) of base column c, one wavefront, fixed order
    auto col_wsum = [&](int64_t c, int64_t e0, int64_t e1) {
        T acc = T(0);
        for (int64_t e = e0 + lane; e < e1; e += 64) acc = fma(X.cval[e], w[X.cidx[e]], acc);
        (void)c;
        return wave_sum64(acc);
    };
    if (ub < icpt) {
        for (int a = b + wv; a < M; a += 4) {
            const int ua = ucols[a];
            T v;
            if (ua < icpt) v = wsum[0];
            else v = col_wsum(ua - icpt, X.cptr[ua - icpt], X.cptr[ua - icpt + 1]);
            if (lane == 0) accs[a] = v;
        }
    } else {
        const int64_t cb = ub - icpt, eb0 = X.cptr[cb], eb1 = X.cptr[cb + 1];
        for (int64_t c0 = eb0; c0 < eb1; c0 += HJ_CHUNK) {
            __syncthreads();
            for (int k = tid; k < HJ_SLOTS; k += 256) keys[k] = -1;
            __syncthreads();
            const int64_t c1 = c0 + HJ_CHUNK < eb1 ? c0 + HJ_CHUNK : eb1;
            for (int64_t e = c0 + tid; e < c1; e += 256) {
                const int32_t row = X.cidx[e];
                unsigned slot = (unsigned(row) * 2654435761u) >> 20;
                while (atomicCAS(&keys[slot], -1, row) != -1) slot = (slot + 1) & (HJ_SLOTS - 1);
                vals[slot] = w[row] * X.cval[e];
            }
            __syncthreads();
            for (int a = b + wv; a < M; a += 4) {
                const int ua = ucols[a];
                T acc;
                if (ua < icpt) {
                    acc = col_wsum(cb, c0, c1);
                } else {
                    acc = T(0);
                    const int64_t ca = ua - icpt, ea1 = X.cptr[ca + 1];
                    for (int64_t e = X.cptr[ca] + lane; e < ea1; e += 64) {
                        const int32_t row = X.cidx[e];
                        unsigned slot = (unsigned(row) * 2654435761u) >> 20;
                        int32_t k;
                        while ((k = keys[slot]) != -1) {
                            if (k == row) { acc = fma(X.cval[e], vals[slot], acc); break; }
                            slot = (slot + 1) & (HJ_SLOTS - 1);
                        }
                    }
                    acc = wave_sum64(acc);
                }
                if (lane == 0) accs[a] += acc; // (column a belongs to this wavefront in every chunk)
            }
        }
    }
    __syncthreads();
    for (int a = b + tid; a < M; a += 256) {
        const T v = accs[a];
        C[a + int64_t(b) * ldc] = v;
        C[b + int64_t(a) * ldc] = v;
    }
}

// ---- axpy -----------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void msp_scatter_kernel(const int32_t* __restrict__ cols, const T* __restrict__ coef,
                                                          const int32_t* __restrict__ cnt_dev, bool clear, T* __restrict__ delta) {
    const int32_t cnt = cnt_dev[0];
    for (int32_t m = blockIdx.x * 256 + threadIdx.x; m < cnt; m += gridDim.x * 256) delta[cols[m]] = clear ? T(0) : coef[m];
}
// out[l nb + i] += sign (delta[l] (ones) + sum_t rval[t] delta[(rcol[t] + icpt) K + l]): 8 lanes per row, KT responses each
template <class T, int KT>
__global__ __launch_bounds__(256) void msp_axpy_kernel(CscView<T> X, int K, int icpt, const T* __restrict__ delta,
                                                       const int32_t* __restrict__ cnt_dev, T sign, T* __restrict__ out) {
    if (cnt_dev[0] <= 0) return;
    const int sub = threadIdx.x & 7, l0 = blockIdx.y * KT;
    const int64_t i = (int64_t(blockIdx.x) * 256 + threadIdx.x) >> 3;
    T acc[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) acc[kk] = T(0);
    if (i < X.n) {
        const int64_t b = X.rptr[i], e = X.rptr[i + 1];
        for (int64_t t = b + sub; t < e; t += 8) {
            const T x = X.rval[t];
            const T* dp = delta + (int64_t(X.rcol[t]) + icpt) * K + l0;
#pragma unroll
            for (int kk = 0; kk < KT; ++kk)
                if (l0 + kk < K) acc[kk] = fma(x, dp[kk], acc[kk]);
        }
    }
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
        acc[kk] += __shfl_xor(acc[kk], 1, 64);
        acc[kk] += __shfl_xor(acc[kk], 2, 64);
        acc[kk] += __shfl_xor(acc[kk], 4, 64);
    }
    if (i < X.n && sub == 0) {
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            const int l = l0 + kk;
            if (l >= K) continue;
            const T a = icpt ? acc[kk] + delta[l] : acc[kk];
            if (a != T(0)) out[int64_t(l) * X.n + i] = fma(sign, a, out[int64_t(l) * X.n + i]);
        }
    }
}

inline unsigned blocks_for(int64_t items, int per_block) {
    return unsigned(std::max<int64_t>(1, (items + per_block - 1) / per_block));
}
template <class T>
inline int parts_of(const CscView<T>& X) { return X.nt > 0 ? X.nt : std::max(X.nb, 1); }
// work of the sweep: the interleaved vectors, the per-tile partials, the K sums of the ones feature
template <class T>
struct SweepWork {
    int64_t vt, part, sums;
    explicit SweepWork(const MultiView<T>& X) {
        const int KT = kt_of(X.K);
        const int64_t kchunks = (X.K + KT - 1) / KT;
        vt = ((kchunks * X.nb * KT + 63) / 64) * 64;
        part = int64_t(parts_of(X.csc)) * (X.pb + X.icpt) * X.K;
        sums = int64_t(X.K) * kVecSumScratch;
    }
};

} // namespace

template <class T>
int64_t multi_sweep_work_elems_csc(const MultiView<T>& X) {
    const SweepWork<T> wk(X);
    return wk.vt + wk.part + wk.sums;
}

template <class T>
void launch_multi_sweep_csc(const MultiView<T>& X, const T* v, T* out, T* work, hipStream_t s) {
    if (X.pb + X.icpt <= 0 || X.K <= 0) return;
    const CscView<T>& B = X.csc;
    const int K = X.K, icpt = X.icpt, KT = kt_of(K), kchunks = (K + KT - 1) / KT, parts = parts_of(B);
    const SweepWork<T> wk(X);
    T *vt = work, *part = work + wk.vt, *sums = part + wk.part;
    const dim3 gi(blocks_for(X.nb, 256), unsigned(kchunks)), gs(blocks_for(B.p, 16), unsigned(parts), unsigned(kchunks));
#define AHIP_MSP_SWEEP(KK)                                                                                                       \
    do {                                                                                                                         \
        hipLaunchKernelGGL((msp_interleave_kernel<T, KK>), gi, dim3(256), 0, s, v, X.nb, K, vt);                                 \
        if (B.nt > 0) hipLaunchKernelGGL((msp_sweep_kernel<T, KK, true>), gs, dim3(256), 0, s, B, K, icpt, vt, part);            \
        else hipLaunchKernelGGL((msp_sweep_kernel<T, KK, false>), gs, dim3(256), 0, s, B, K, icpt, vt, part);                    \
    } while (0)
    if (KT == 8) AHIP_MSP_SWEEP(8); else if (KT == 4) AHIP_MSP_SWEEP(4); else AHIP_MSP_SWEEP(2);
#undef AHIP_MSP_SWEEP
    if (icpt) {
        hipLaunchKernelGGL((msp_vec_sum_kernel<T>), dim3(256, unsigned(K)), dim3(256), 0, s, v, X.nb, sums, 0);
        hipLaunchKernelGGL((msp_vec_sum_kernel<T>), dim3(1, unsigned(K)), dim3(256), 0, s, v, X.nb, sums, 1);
    }
    const int64_t nfeat = X.pb + icpt;
    hipLaunchKernelGGL((msp_sweep_reduce_kernel<T>), dim3(blocks_for(nfeat * K, 256)), dim3(256), 0, s, part, parts, sums, nfeat, K, icpt,
                       out);
}

int64_t multi_step_work_elems_csc(int K) { return int64_t(K) * ONES_PARTS; }

template <class T>
int launch_multi_panel_step_csc(const MultiView<T>& X, const T* w, T* r, const int32_t* dcol, const T* dlt, const int32_t* nz_dev,
                                const int32_t* cols, int nb_cols, T* gblk, T* work, hipStream_t s) {
    const CscView<T>& B = X.csc;
    const int K = X.K, icpt = X.icpt, KT = kt_of(K);
    const unsigned kchunks = unsigned((K + KT - 1) / KT);
    nb_cols = std::min(nb_cols, 2 * MAXB);
#define AHIP_MSP_STEP(KK)                                                                                                        \
    do {                                                                                                                         \
        hipLaunchKernelGGL((msp_update_kernel<T, KK>), dim3(MAXB, kchunks), dim3(256), 0, s, B, K, icpt, dcol, dlt, nz_dev, r);  \
        if (nb_cols > 0) {                                                                                                       \
            hipLaunchKernelGGL((msp_grad_kernel<T, KK>), dim3(unsigned(nb_cols), kchunks), dim3(256), 0, s, B, K, icpt, w, r, cols, \
                               nb_cols, gblk);                                                                                   \
            if (icpt) {                                                                                                          \
                hipLaunchKernelGGL((msp_ones_grad_kernel<T, KK>), dim3(ONES_PARTS, kchunks), dim3(256), 0, s, X.nb, K, w, r, cols, \
                                   nb_cols, work, gblk, 0);                                                                      \
                hipLaunchKernelGGL((msp_ones_grad_kernel<T, KK>), dim3(1, kchunks), dim3(256), 0, s, X.nb, K, w, r, cols, nb_cols, \
                                   work, gblk, 1);                                                                               \
            }                                                                                                                    \
        }                                                                                                                        \
    } while (0)
    if (KT == 8) AHIP_MSP_STEP(8); else if (KT == 4) AHIP_MSP_STEP(4); else AHIP_MSP_STEP(2);
#undef AHIP_MSP_STEP
    return 0; // (no slice partials: the gradient is in gblk)
}

template <class T>
void launch_syrk_multi_csc(const MultiView<T>& X, const T* w, const int32_t* ucols, int32_t M, T* C, int64_t ldc, T* work,
                           hipStream_t s) {
    if (M <= 0) return;
    if (X.icpt) launch_vec_sum<T>(w, X.nb, work, s);
    {
        BuildLaunchInfo r;
        r.kind = BuildLaunchInfo::BLOCK_GRAM_CSC; r.nsplit = 1; r.tile = M;
        last_build_launch() = r;
    }
    hipLaunchKernelGGL((msp_gram_kernel<T>), dim3(unsigned(std::min<int32_t>(M, MAXB))), dim3(256), 0, s, X.csc, int(X.icpt), w, ucols,
                       int(std::min<int32_t>(M, MAXB)), work, C, ldc);
}

template <class T>
void launch_multi_axpy_cols_csc(const MultiView<T>& X, const int32_t* cols, const T* coef, const int32_t* cnt_dev, T sign, T* out,
                                T* delta_zeroed, hipStream_t s) {
    const int K = X.K, KT = kt_of(K);
    const dim3 grid(blocks_for(X.nb * 8, 256), unsigned((K + KT - 1) / KT));
    hipLaunchKernelGGL((msp_scatter_kernel<T>), dim3(64), dim3(256), 0, s, cols, coef, cnt_dev, false, delta_zeroed);
#define AHIP_MSP_AXPY(KK) \
    hipLaunchKernelGGL((msp_axpy_kernel<T, KK>), grid, dim3(256), 0, s, X.csc, K, int(X.icpt), delta_zeroed, cnt_dev, sign, out)
    if (KT == 8) AHIP_MSP_AXPY(8); else if (KT == 4) AHIP_MSP_AXPY(4); else AHIP_MSP_AXPY(2);
#undef AHIP_MSP_AXPY
    hipLaunchKernelGGL((msp_scatter_kernel<T>), dim3(64), dim3(256), 0, s, cols, coef, cnt_dev, true, delta_zeroed);
}

#define INST(T)                                                                                                                  \
    template int64_t multi_sweep_work_elems_csc<T>(const MultiView<T>&);                                                         \
    template void launch_multi_sweep_csc<T>(const MultiView<T>&, const T*, T*, T*, hipStream_t);                                 \
    template int launch_multi_panel_step_csc<T>(const MultiView<T>&, const T*, T*, const int32_t*, const T*, const int32_t*,     \
                                                const int32_t*, int, T*, T*, hipStream_t);                                       \
    template void launch_syrk_multi_csc<T>(const MultiView<T>&, const T*, const int32_t*, int32_t, T*, int64_t, T*, hipStream_t); \
    template void launch_multi_axpy_cols_csc<T>(const MultiView<T>&, const int32_t*, const T*, const int32_t*, T, T*, T*, hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
