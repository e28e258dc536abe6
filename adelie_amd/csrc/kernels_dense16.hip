// kernels_dense16.hip — sweep, Gram, axpy_cols and sp_tmul over a dense design stored as IEEE half or bfloat16 (gfx950 / CDNA4).
//
// The matrix stays 2 bytes a value in HBM, column- or row-major, exactly as the caller laid it out (adelie_hip_design_create_dense16 /
// _adopt_dense16_dev); every value is converted to float32 in registers and all arithmetic is float32, so the design IS the float32
// design of those values.  bfloat16 -> float32 is a 16-bit shift into the float32 pattern; half -> float32 is v_cvt_f32_f16, which
// keeps subnormals, signed zeros, infinities and NaN.  Format and order are template parameters; what the host chooses at run time
// is the load width of the kernels that read columns in place (AL below).
//
//   sweep, column-major   A workgroup owns 8 columns and one row split and walks it in tiles of 2048 rows.  Column j starts at byte
//       2 (j ld) of the matrix, so with ld not a multiple of 8 (or an adopted slice) every column has its own offset to the next
//       16-byte boundary.  Lane t of a tile therefore owns, per column, the ALIGNED vector of 8 values whose rows are
//       [t0 + 8 t - e, t0 + 8 t - e + 8), e = the column's offset in elements: one 16-byte load when all 8 rows lie in the split,
//       otherwise (only the lanes at the two ends of a split: a column's head and tail) guarded 2-byte loads of the rows that do.
//       No 16-byte load is misaligned and nothing outside the split's rows of the column is read.  The 8 loads of a lane's columns
//       are issued before the first conversion.  v is shared by the columns but shifted by e against each: the tile's 2048 + 8
//       values go through LDS once per tile, stored "transposed by 8" (row x at (x mod 8) * 264 + x / 8), so that the lanes of a
//       wave read consecutive words whatever the shift (read straight, a stride of 8 words would be a 16-way bank conflict; the
//       stride 264 = 8 mod 32 keeps the stores conflict-free as well).  One float32 accumulator per column and lane takes
//       rows_per_split / 256 terms, as the float32 dense sweep's does; lanes, waves and row splits are then added in the fixed order
//       of sweep_common.hpp.  No atomics.
//   sweep, row-major   A lane owns a column and reads it with 2-byte loads that are contiguous over the wave (128 B per
//       instruction), v[i] is uniform.  Eight accumulators per lane (row mod 8), at most 256 terms each.
//   axpy_cols / sp_tmul   A lane owns 8 rows of the output and walks the columns four at a time.  Rows start at multiples of 8, so
//       the loads are as wide as base pointer and leading dimension allow for every column at once: AL = 8, 4, 2 or 1 values per
//       load, chosen on the host (row-major: 2-byte loads a row apart).
//   Gram   C = X_M^T diag(w) X_N on v_mfma_f32_16x16x4_f32, the instruction of the float32 dense Gram: w is float32 and w x is
//       not a 16-bit value, so the 16-bit MFMA formats do not fit.  A workgroup owns a 64 x 64 tile and one K-split, four waves of
//       32 x 32 each.  The 16-bit operand halves the LDS bytes of a stage, and that goes into depth: a stage is 64 rows (the dense
//       kernel: 32) of 128 columns kept 16-bit in LDS (20 KB with the padding), one barrier pair per 64 rows.  Rows within a block
//       of 16 are dealt to the MFMA's k index as fk * 4 + u, so a lane reads its four values of a column as one 8-byte word and
//       converts them in registers; columns are padded to 40 words, which makes those reads conflict-free.  The next stage's global
//       loads are in flight during the MFMAs.  K-split partials are summed in a fixed order by a second kernel that centres and,
//       for the symmetric calls of the solver, mirrors -- the contract of launch_gram.
#include "sweep_common.hpp"
#include "gram_common.hpp"
#include <algorithm>

namespace ahip {

namespace {

typedef unsigned u2v_t __attribute__((ext_vector_type(2)));

// the float32 value of the 16-bit pattern in the low / high half of a word
template <int FMT>
__device__ __forceinline__ float cvt_lo(unsigned w) {
    if constexpr (FMT == kFmtBF16) return __uint_as_float(w << 16);
    else {
        const unsigned short h = (unsigned short)(w & 0xffffu);
        _Float16 x;
        __builtin_memcpy(&x, &h, 2);
        return float(x);
    }
}
template <int FMT>
__device__ __forceinline__ float cvt_hi(unsigned w) {
    if constexpr (FMT == kFmtBF16) return __uint_as_float(w & 0xffff0000u);
    else return cvt_lo<FMT>(w >> 16);
}
// value e (0..7) of four packed words
template <int FMT>
__device__ __forceinline__ float cvt_at(const unsigned (&w)[4], int e) {
    return (e & 1) ? cvt_hi<FMT>(w[e >> 1]) : cvt_lo<FMT>(w[e >> 1]);
}

// ---- sweep, column-major ---------------------------------------------------------------------------------------------------
constexpr int kCB16 = 8;                 // columns per workgroup
constexpr int kTile16 = kThreads * 8;    // rows per tile
constexpr int kLdv16 = 264;              // words per residue class of the transposed v tile: >= kTile16 / 8 + 1, = 8 mod 32
static_assert(kLdv16 >= kTile16 / 8 + 1 && kLdv16 % 32 == 8, "the v tile's layout");

// the rows of [r0, r1) among the 8 from i_lo on, one 2-byte load each (a split's head and tail)
__device__ __noinline__ u4v_t load8_guarded(const unsigned short* __restrict__ col, int64_t i_lo, int64_t r0, int64_t r1) {
    u4v_t x = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int64_t i = i_lo + u;
        if (i >= r0 && i < r1) x[u >> 1] |= unsigned(col[i]) << (16 * (u & 1));
    }
    return x;
}

template <int FMT, bool SQ>
__global__ __launch_bounds__(kThreads) void sweep16_cm_kernel(const unsigned short* __restrict__ X, int64_t ld, int64_t n,
                                                              const float* __restrict__ v, float* __restrict__ out, int64_t c0,
                                                              int64_t ncols, const int32_t* __restrict__ cols,
                                                              int64_t rows_per_split, int nsplit,
                                                              const float* __restrict__ sub_scale,
                                                              const float* __restrict__ sub_vec) {
    __shared__ float vs[8 * kLdv16];
    __shared__ float red[kThreads / 64][kCB16];
    const int tid = threadIdx.x;
    const int64_t cb = blockIdx.x;
    const int split = blockIdx.y;
    const int64_t r0 = int64_t(split) * rows_per_split; // (a multiple of kTile16)
    const int64_t r1 = min(n, r0 + rows_per_split);

    const unsigned short* cp[kCB16];
    int sh[kCB16]; // 8 - e: where the lane's first row stands in the v tile, minus 8 t
#pragma unroll
    for (int k = 0; k < kCB16; ++k) {
        int64_t c = cb * kCB16 + k;
        if (c >= ncols) c = ncols - 1; // duplicate work on the tail panel, discarded in the epilogue
        const int64_t j = cols ? int64_t(cols[c]) : c0 + c;
        cp[k] = X + j * ld;
        sh[k] = 8 - int((reinterpret_cast<uintptr_t>(cp[k]) >> 1) & 7);
    }
    float acc[kCB16];
#pragma unroll
    for (int k = 0; k < kCB16; ++k) acc[k] = 0.f;

    // a column's row i stands in the tile with t0 <= i + e < t0 + kTile16, e <= 7: the last tile may hold a tail only
    for (int64_t t0 = r0; t0 < r1 + 8; t0 += kTile16) {
        __syncthreads(); // the previous tile's v is consumed
        // v[t0 - 8 + x] for x < kTile16 + 8, zero outside the split
        for (int x = tid; x < kTile16 + 8; x += kThreads) {
            const int64_t i = t0 - 8 + x;
            vs[(x & 7) * kLdv16 + (x >> 3)] = (i >= r0 && i < r1) ? v[i] : 0.f;
        }
        __syncthreads();
        u4v_t xx[kCB16];
#pragma unroll
        for (int k = 0; k < kCB16; ++k) {
            const int64_t i_lo = t0 + 8 * tid + (sh[k] - 8);
            if (i_lo >= r0 && i_lo + 8 <= r1) xx[k] = __builtin_nontemporal_load(reinterpret_cast<const u4v_t*>(cp[k] + i_lo));
            else if (i_lo + 8 <= r0 || i_lo >= r1) xx[k] = u4v_t{0u, 0u, 0u, 0u};
            else xx[k] = load8_guarded(cp[k], i_lo, r0, r1);
        }
#pragma unroll
        for (int k = 0; k < kCB16; ++k) {
            const unsigned w[4] = {xx[k][0], xx[k][1], xx[k][2], xx[k][3]};
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = sh[k] + u; // tile position 8 t + q, q in [1, 15]
                const float vi = vs[(q & 7) * kLdv16 + tid + (q >> 3)];
                const float x0 = cvt_at<FMT>(w, u);
                acc[k] = fmaf(SQ ? x0 * x0 : x0, vi, acc[k]);
            }
        }
    }
    panel_epilogue<false>(acc, red, cb, ncols, c0, cols, nullptr, out, split, nsplit, sub_scale, sub_vec);
}

// ---- sweep, row-major ------------------------------------------------------------------------------------------------------
template <int FMT, bool SQ>
__global__ __launch_bounds__(kThreads) void sweep16_rm_kernel(const unsigned short* __restrict__ X, int64_t ld, int64_t n,
                                                              const float* __restrict__ v, float* __restrict__ out, int64_t c0,
                                                              int64_t ncols, const int32_t* __restrict__ cols,
                                                              int64_t rows_per_split, int nsplit,
                                                              const float* __restrict__ sub_scale,
                                                              const float* __restrict__ sub_vec) {
    const int split = blockIdx.y;
    const int64_t r0 = int64_t(split) * rows_per_split;
    const int64_t r1 = min(n, r0 + rows_per_split);
    int64_t c = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    const bool live = c < ncols;
    if (!live) c = ncols - 1;
    const int64_t j = cols ? int64_t(cols[c]) : c0 + c;
    const unsigned short* p = X + j;
    float acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.f;
    for (int64_t i = r0; i < r1; i += 8) {
        unsigned h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) h[u] = (i + u < r1) ? unsigned(p[(i + u) * ld]) : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float x0 = cvt_lo<FMT>(h[u]);
            const float vi = (i + u < r1) ? v[i + u] : 0.f;
            acc[u] = fmaf(SQ ? x0 * x0 : x0, vi, acc[u]);
        }
    }
    if (!live) return;
    const float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    store_sum(s, out, c, j, split, nsplit, ncols, sub_scale, sub_vec);
}

// row splits of the row-major sweep: about 2048 workgroups, at most 2048 rows (256 terms per accumulator) per split
inline void sweep16_rm_shape(int64_t n, int64_t ncols, int64_t& blocks_c, int& nsplit, int64_t& rps) {
    blocks_c = (ncols + kThreads - 1) / kThreads;
    const int64_t want = std::max<int64_t>(1, (2048 + blocks_c - 1) / blocks_c);
    rps = (n + want - 1) / want;
    rps = std::min<int64_t>(((rps + 63) / 64) * 64, 2048);
    while ((n + rps - 1) / rps > 65535) rps *= 2;
    nsplit = int((n + rps - 1) / rps);
}

// ---- 8 rows of one column, in place (axpy_cols, sp_tmul, the Gram's stages) ---------------------------------------------------
// Rows [i0, i0 + 8) of column j as four packed words, a row at or beyond `nlim` (<= n) giving 0.  i0 is a multiple of 8.
// Column-major: AL values per load, every column start being a multiple of AL values from a 2 AL-byte boundary (the host's
// choice: dense16_al).  Row-major: 2-byte loads ld values apart.
template <bool RM, int AL>
__device__ __forceinline__ void load8(const unsigned short* __restrict__ X, int64_t ld, int64_t nlim, int64_t j, int64_t i0,
                                      unsigned (&w)[4]) {
    if constexpr (RM) {
        const unsigned short* p = X + j;
        unsigned h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) h[u] = (i0 + u < nlim) ? unsigned(p[(i0 + u) * ld]) : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = h[2 * u] | (h[2 * u + 1] << 16);
    } else {
        const unsigned short* p = X + j * ld + i0;
        if (AL > 1 && i0 + 8 <= nlim) {
            if constexpr (AL == 8) {
                const u4v_t x = *reinterpret_cast<const u4v_t*>(p);
                w[0] = x[0], w[1] = x[1], w[2] = x[2], w[3] = x[3];
            } else if constexpr (AL == 4) {
                const u2v_t x = *reinterpret_cast<const u2v_t*>(p), y = *reinterpret_cast<const u2v_t*>(p + 4);
                w[0] = x[0], w[1] = x[1], w[2] = y[0], w[3] = y[1];
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const unsigned*>(p + 2 * u);
            }
        } else {
            unsigned h[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) h[u] = (i0 + u < nlim) ? unsigned(p[u]) : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = h[2 * u] | (h[2 * u + 1] << 16);
        }
    }
}

// acc[e] += sum over k in [k0, k1) of coef[k] X[i0 + e, idx[k]], k ascending, four columns' loads in flight
template <int FMT, bool RM, int AL, class I>
__device__ __forceinline__ void accum8(const unsigned short* __restrict__ X, int64_t ld, int64_t n, int64_t i0,
                                       const I* __restrict__ idx, const float* __restrict__ coef, int64_t k0, int64_t k1,
                                       float (&acc)[8]) {
    int64_t k = k0;
    for (; k + 4 <= k1; k += 4) {
        unsigned w[4][4];
        float cf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            cf[u] = coef[k + u];
            load8<RM, AL>(X, ld, n, int64_t(idx[k + u]), i0, w[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(cf[u], cvt_at<FMT>(w[u], e), acc[e]);
    }
    for (; k < k1; ++k) {
        unsigned w[4];
        const float cf = coef[k];
        load8<RM, AL>(X, ld, n, int64_t(idx[k]), i0, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(cf, cvt_at<FMT>(w, e), acc[e]);
    }
}

template <int FMT, bool RM, int AL>
__global__ __launch_bounds__(kThreads) void axpy16_kernel(const unsigned short* __restrict__ X, int64_t ld, int64_t n,
                                                          const int32_t* __restrict__ cols, const float* __restrict__ coef,
                                                          const int32_t* __restrict__ count_dev, int32_t count, float sign,
                                                          float* __restrict__ out) {
    const int K = count_dev ? count_dev[0] : count;
    if (K <= 0) return;
    const int64_t i0 = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * 8;
    if (i0 >= n) return;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    accum8<FMT, RM, AL, int32_t>(X, ld, n, i0, cols, coef, 0, K, acc);
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (i0 + e < n) out[i0 + e] += sign * acc[e];
}

template <int FMT, bool RM, int AL>
__global__ __launch_bounds__(kThreads) void sp_tmul16_kernel(const unsigned short* __restrict__ X, int64_t ld, int64_t n,
                                                             const int64_t* __restrict__ indptr,
                                                             const int64_t* __restrict__ indices,
                                                             const float* __restrict__ values, float* __restrict__ out) {
    const int64_t l = blockIdx.y;
    const int64_t i0 = (int64_t(blockIdx.x) * kThreads + threadIdx.x) * 8;
    if (i0 >= n) return;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    accum8<FMT, RM, AL, int64_t>(X, ld, n, i0, indices, values, indptr[l], indptr[l + 1], acc);
    float* o = out + l * n;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (i0 + e < n) o[i0 + e] = acc[e];
}

// ---- Gram ------------------------------------------------------------------------------------------------------------------
constexpr int G16_B = 64;    // tile edge
constexpr int G16_KT = 64;   // rows per stage
constexpr int G16_LDW = 40;  // words per staged column (32 of data): = 8 mod 32, and whole 16-byte units
static_assert(kGramKT % 8 == 0, "a K-split starts on a multiple of 8 rows (load8)");

template <int FMT, bool RM, int AL>
__global__ __launch_bounds__(256, 2) void gram16_kernel(const unsigned short* __restrict__ X, int64_t ld, int64_t n,
                                                        const float* __restrict__ w, const int32_t* __restrict__ mcols, int32_t M,
                                                        const int32_t* __restrict__ ncols, int32_t N, int64_t kchunk,
                                                        float* __restrict__ part, int64_t Mpad, int64_t Npad, int32_t Nt) {
    __shared__ u4v_t S4[2 * G16_B * G16_LDW / 4]; // columns 0..63: the M side, 64..127: the N side
    __shared__ f4v_t W4[G16_KT / 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int bm = blockIdx.x / Nt, bn = blockIdx.x % Nt, sp = blockIdx.y;
    const int64_t k0 = int64_t(sp) * kchunk; // (a multiple of kGramKT)
    const int64_t kend = min(n, k0 + kchunk);

    // staging role: 32 rows of one of the 128 columns
    const int sc = tid >> 1, sr = (tid & 1) * 32;
    const int ci = sc < G16_B ? bm * G16_B + sc : bn * G16_B + (sc - G16_B);
    const bool ok = sc < G16_B ? ci < M : ci < N;
    const int64_t j = ok ? int64_t(sc < G16_B ? mcols[ci] : ncols[ci]) : 0;

    f4v_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f4v_t{0.f, 0.f, 0.f, 0.f};

    unsigned rg[4][4];
    float rw = 0.f;
    auto fetch = [&](int64_t k) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (ok) load8<RM, AL>(X, ld, kend, j, k + sr + 8 * m, rg[m]);
            else rg[m][0] = rg[m][1] = rg[m][2] = rg[m][3] = 0u;
        }
        if (tid < G16_KT) rw = (k + tid < kend) ? w[k + tid] : 0.f;
    };
    if (k0 < kend) fetch(k0);
    const int fr = lane & 15, fk = lane >> 4;
    const u2v_t* S2 = reinterpret_cast<const u2v_t*>(S4);
    float* Ws = reinterpret_cast<float*>(W4);
    for (int64_t k = k0; k < kend; k += G16_KT) {
        __syncthreads(); // the previous stage is consumed
#pragma unroll
        for (int m = 0; m < 4; ++m) S4[(sc * G16_LDW + sr / 2) / 4 + m] = u4v_t{rg[m][0], rg[m][1], rg[m][2], rg[m][3]};
        if (tid < G16_KT) Ws[tid] = rw;
        __syncthreads();
        if (k + G16_KT < kend) fetch(k + G16_KT); // in flight while the MFMAs run
#pragma unroll
        for (int kb = 0; kb < G16_KT / 16; ++kb) {
            const f4v_t wq = W4[kb * 4 + fk]; // the weights of rows kb * 16 + fk * 4 + u
            u2v_t a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = S2[((wm * 32 + t * 16 + fr) * G16_LDW + kb * 8 + fk * 2) / 2];
                b[t] = S2[((G16_B + wn * 32 + t * 16 + fr) * G16_LDW + kb * 8 + fk * 2) / 2];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float af[2], bf[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    af[t] = (u & 1) ? cvt_hi<FMT>(a[t][u >> 1]) : cvt_lo<FMT>(a[t][u >> 1]);
                    bf[t] = ((u & 1) ? cvt_hi<FMT>(b[t][u >> 1]) : cvt_lo<FMT>(b[t][u >> 1])) * wq[u];
                }
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                    for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = Mfma<float>::run(af[ta], bf[tb], acc[ta][tb]);
            }
        }
    }
    // partial tile -> part[sp][col][row] (col = N index, row = M index), padded to whole tiles
    float* P = part + int64_t(sp) * Mpad * Npad;
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = bm * G16_B + wm * 32 + ta * 16 + Mfma<float>::row(lane, e);
                const int col = bn * G16_B + wn * 32 + tb * 16 + (lane & 15);
                P[int64_t(col) * Mpad + row] = acc[ta][tb][e];
            }
}

// The K-split partials of C[m_pos0 + a, n_pos0 + b] in four interleaved groups added in a fixed order, centred; a symmetric call
// (launch_gram's rule) takes every pair inside the new x new square from its lower-triangle entry and writes the mirror too.
__global__ __launch_bounds__(256) void gram16_reduce_kernel(const float* __restrict__ part, int nsplit, int64_t Mpad, int64_t Npad,
                                                            int32_t M, int32_t N, const int32_t* __restrict__ mcols,
                                                            const int32_t* __restrict__ ncols, int32_t m_pos0, int32_t n_pos0,
                                                            const float* __restrict__ xm, int center, int symmetric,
                                                            float* __restrict__ C, int64_t ldc) {
    __shared__ float red[4][64];
    const int ta = threadIdx.x & 63, tg = threadIdx.x >> 6;
    const int a = blockIdx.x * 64 + ta, b = blockIdx.y;
    const int64_t rp = int64_t(m_pos0) + a, cp = int64_t(n_pos0) + b;
    const bool skip = !(a < M && b < N) || (symmetric && rp >= n_pos0 && rp < cp);
    float s = 0.f;
    if (!skip) {
        const int64_t stride = Mpad * Npad;
        const float* base = part + int64_t(b) * Mpad + a;
        for (int sp = tg; sp < nsplit; sp += 4) s += base[int64_t(sp) * stride];
    }
    red[tg][ta] = s;
    __syncthreads();
    if (tg != 0 || skip) return;
    s = (red[0][ta] + red[1][ta]) + (red[2][ta] + red[3][ta]);
    if (center) s -= xm[mcols[a]] * xm[ncols[b]];
    C[rp + cp * ldc] = s;
    if (symmetric) C[cp + rp * ldc] = s;
}

// values per load that every column start allows (column-major; a row offset is a multiple of 8 values)
inline int dense16_al(const Dense16View& X) {
    if (X.row_major) return 1;
    const uintptr_t at = reinterpret_cast<uintptr_t>(X.X);
    for (int al = 8; al > 1; al /= 2)
        if (at % (2 * al) == 0 && X.ld % al == 0) return al;
    return 1;
}

// KERNEL<FMT, RM, AL> for the view's format, order and load width
#define DENSE16_PICK(KERNEL, X, kernel)                                                                                     \
    do {                                                                                                                    \
        const int al_ = dense16_al(X);                                                                                      \
        if ((X).fmt == kFmtBF16) {                                                                                          \
            kernel = (X).row_major ? KERNEL<kFmtBF16, true, 1>                                                              \
                   : al_ == 8 ? KERNEL<kFmtBF16, false, 8> : al_ == 4 ? KERNEL<kFmtBF16, false, 4>                          \
                   : al_ == 2 ? KERNEL<kFmtBF16, false, 2> : KERNEL<kFmtBF16, false, 1>;                                    \
        } else {                                                                                                            \
            kernel = (X).row_major ? KERNEL<kFmtF16, true, 1>                                                               \
                   : al_ == 8 ? KERNEL<kFmtF16, false, 8> : al_ == 4 ? KERNEL<kFmtF16, false, 4>                            \
                   : al_ == 2 ? KERNEL<kFmtF16, false, 2> : KERNEL<kFmtF16, false, 1>;                                      \
        }                                                                                                                   \
    } while (0)

} // namespace

// ---- launchers (kernels.hpp) -------------------------------------------------------------------------------------------------
int64_t sweep_work_elems_dense16(const Dense16View& X, int64_t ncols) {
    if (ncols <= 0) return 0;
    int64_t blocks_c, rps;
    int ns;
    if (X.row_major) sweep16_rm_shape(X.n, ncols, blocks_c, ns, rps);
    else sweep_shape(X.n, ncols, 8, blocks_c, ns, rps, kCB16);
    return int64_t(ns) * ncols + 16;
}

void launch_sweep_dense16(const Dense16View& X, const float* v, float* out, int64_t c0, int64_t ncols, const int32_t* cols,
                          const float* sub_scale, const float* sub_vec, bool square, float* work, hipStream_t s) {
    if (ncols <= 0) return;
    const bool bf = X.fmt == kFmtBF16;
    int64_t blocks_c, rps;
    int ns;
    auto kernel = sweep16_cm_kernel<kFmtF16, false>;
    if (X.row_major) {
        sweep16_rm_shape(X.n, ncols, blocks_c, ns, rps);
        kernel = bf ? (square ? sweep16_rm_kernel<kFmtBF16, true> : sweep16_rm_kernel<kFmtBF16, false>)
                    : (square ? sweep16_rm_kernel<kFmtF16, true> : sweep16_rm_kernel<kFmtF16, false>);
    } else {
        sweep_shape(X.n, ncols, 8, blocks_c, ns, rps, kCB16); // (rows per split: whole tiles of kTile16 rows)
        kernel = bf ? (square ? sweep16_cm_kernel<kFmtBF16, true> : sweep16_cm_kernel<kFmtBF16, false>)
                    : (square ? sweep16_cm_kernel<kFmtF16, true> : sweep16_cm_kernel<kFmtF16, false>);
    }
    float* dst = ns == 1 ? out : work;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks_c, (unsigned)ns), dim3(kThreads), 0, s, X.X, X.ld, X.n, v, dst, c0, ncols, cols,
                       rps, ns, sub_scale, sub_vec);
    if (ns > 1) launch_sweep_reduce<float>(work, out, ncols, ns, c0, cols, sub_scale, sub_vec, s);
}

void launch_axpy_cols_dense16(const Dense16View& X, const int32_t* cols, const float* coef, const int32_t* count_dev, int32_t count,
                              float sign, float* out, hipStream_t s) {
    if (X.n <= 0 || (!count_dev && count <= 0)) return;
    auto kernel = axpy16_kernel<kFmtF16, false, 1>;
    DENSE16_PICK(axpy16_kernel, X, kernel);
    const int64_t rows = int64_t(kThreads) * 8;
    hipLaunchKernelGGL(kernel, dim3(unsigned((X.n + rows - 1) / rows)), dim3(kThreads), 0, s, X.X, X.ld, X.n, cols, coef, count_dev,
                       count, sign, out);
}

void launch_sp_tmul_dense16(const Dense16View& X, int64_t L, const int64_t* indptr, const int64_t* indices, const float* values,
                            float* out, hipStream_t s) {
    if (L <= 0 || X.n <= 0) return;
    auto kernel = sp_tmul16_kernel<kFmtF16, false, 1>;
    DENSE16_PICK(sp_tmul16_kernel, X, kernel);
    const int64_t rows = int64_t(kThreads) * 8;
    for (int64_t l0 = 0; l0 < L; l0 += 65535) {
        const unsigned ly = unsigned(L - l0 < 65535 ? L - l0 : 65535);
        hipLaunchKernelGGL(kernel, dim3(unsigned((X.n + rows - 1) / rows), ly), dim3(kThreads), 0, s, X.X, X.ld, X.n, indptr + l0,
                           indices, values, out + l0 * X.n);
    }
}

// (the K-splits of gram_shape, whose partial buffer -- 128-row tiles -- covers this one's 64-row tiles)
void launch_gram_dense16(const Dense16View& X, const float* w, const int32_t* mcols, int32_t M, int32_t m_pos0, const int32_t* ncols,
                         int32_t N, int32_t n_pos0, const float* xm_by_col, bool center, float* C, int64_t ldc, float* work,
                         hipStream_t s) {
    if (M <= 0 || N <= 0) return;
    const GramShape g = gram_shape(X.n, M, N);
    const int64_t Mt = (M + G16_B - 1) / G16_B, Nt = (N + G16_B - 1) / G16_B;
    const int64_t Mpad = Mt * G16_B, Npad = Nt * G16_B;
    const int symmetric = (mcols + (n_pos0 - m_pos0) == ncols && m_pos0 + M == n_pos0 + N && n_pos0 >= m_pos0) ? 1 : 0;
    auto kernel = gram16_kernel<kFmtF16, false, 1>;
    DENSE16_PICK(gram16_kernel, X, kernel);
    hipLaunchKernelGGL(kernel, dim3(unsigned(Mt * Nt), unsigned(g.nsplit)), dim3(256), 0, s, X.X, X.ld, X.n, w, mcols, M, ncols, N,
                       g.kchunk, work, Mpad, Npad, int32_t(Nt));
    hipLaunchKernelGGL(gram16_reduce_kernel, dim3(unsigned((M + 63) / 64), unsigned(N)), dim3(256), 0, s, work, g.nsplit, Mpad, Npad,
                       M, N, mcols, ncols, m_pos0, n_pos0, xm_by_col, center ? 1 : 0, symmetric, C, ldc);
}

} // namespace ahip
