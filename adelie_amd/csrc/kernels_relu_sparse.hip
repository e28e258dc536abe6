// kernels_relu_sparse.hip — gated / signed convex-ReLU designs over a SPARSE base matrix Z, kept sparse (gfx950 / CDNA4, wave64).
//
// The design (reference MatrixNaiveConvexReluSparse / MatrixNaiveConvexGatedReluSparse, matrix_naive_convex_relu.ipp,
// matrix_naive_convex_gated_relu.ipp) has (gated ? 1 : 2) m d columns; column sgn (m d) + j_m d + j_d stores +-Z[i, j_d] at the
// rows i where Z stores an entry and mask[i, j_m] is set.  Input: Z's column- and row-compressed arrays in canonical form and
// the mask packed to words of 32 gates per row, all on the device.  Output: the six arrays of a CscView in canonical form
// (rows ascending inside a column, columns ascending inside a row, no explicit zeros), so that every kernel of
// kernels_sparse.hip runs on the result.  No n x P array is formed and nothing is sorted.
//
//   relu_sp_pack        bits[w n + i] = the gates 32 w .. 32 w + 31 of row i, from the column-major mask bytes
//   relu_sp_col_count   one wavefront per (column j_d of Z, row tile t, word w): the entries of the segment 64 at a time; the
//                       ballot of the lanes whose row has gate g set counts them -> col_cnt[(j_m d + j_d) nt + t]
//   relu_sp_row_count   one thread per row: (gated ? 1 : 2) popcount(mask row) nnz(Z row)
//   (the caller turns the counts into cptr, the start of every (column, tile) segment and rptr by prefix sums)
//   relu_sp_col_fill    the walk of the count again: segment start + entries of the earlier steps + the lower lanes of the
//                       ballot place an entry; a column keeps the order of Z's column
//   relu_sp_row_fill    one wavefront per row: sgn-major, then the set gates ascending, then Z's row entries in their order
//   relu_sp_sweep       the structured full sweep: one wavefront per (j_d, t, w) reads its segment of Z 64 entries at a time,
//                       gathers v and ONE mask word per entry and keeps the sums of the word's gates in registers; a butterfly
//                       adds the lanes.  nnz(Z) entries are read instead of the about m / 2 times as many of the expansion.
//   relu_sp_reduce      adds the tiles' partial sums in tile order, applies the epilogue of the other sweeps per column and writes
//                       the negated sum into the signed half
//
// Every position comes from a count and a prefix sum, none from an atomic's return value, and every sum is added in a fixed
// order without floating-point atomics: two builds give identical arrays, two sweeps identical bits.
#include "kernels.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace ahip {

namespace {

constexpr int kWB = kReluSpWordBits;
constexpr int kRowThreads = 256;
constexpr int kRowWaves = 4; // rows (one wavefront each) per workgroup of relu_sp_row_fill

__global__ __launch_bounds__(kRowThreads) void relu_sp_pack_kernel(const uint8_t* __restrict__ mask, int64_t n, int64_t m,
                                                                   uint32_t* __restrict__ bits) {
    const int64_t i = int64_t(blockIdx.x) * kRowThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t w = blockIdx.y;
    uint32_t b = 0;
    for (int g = 0; g < kWB; ++g) {
        const int64_t jm = w * kWB + g;
        if (jm < m && mask[i + jm * n] != 0) b |= uint32_t(1) << g;
    }
    bits[w * n + i] = b;
}

// what identifies a wavefront's work: column j of Z, tile t, word w and the segment [k0, k1) of Z's entries
struct Seg {
    int64_t j, k0, k1;
    int t, w;
};
template <class T>
__device__ __forceinline__ Seg relu_sp_seg(const ReluCscView<T>& F) {
    Seg s;
    s.j = int64_t(blockIdx.x) / F.nt;
    s.t = int(int64_t(blockIdx.x) % F.nt);
    s.w = int(blockIdx.y);
    const int64_t* sp = F.seg + s.j * (F.nt + 1) + s.t;
    s.k0 = sp[0];
    s.k1 = sp[1];
    return s;
}

template <class T>
__global__ __launch_bounds__(64) void relu_sp_col_count_kernel(ReluCscView<T> F, int32_t* __restrict__ col_cnt) {
    const int lane = threadIdx.x;
    const Seg sg = relu_sp_seg(F);
    const uint32_t* __restrict__ bw = F.bits + int64_t(sg.w) * F.n;
    int32_t mine = 0; // lane g ends up with the count of gate g
    for (int64_t kb = sg.k0; kb < sg.k1; kb += 64) { // (uniform over the wave)
        const int64_t k = kb + lane;
        const uint32_t word = k < sg.k1 ? bw[F.zidx[k]] : 0u;
#pragma unroll
        for (int g = 0; g < kWB; ++g) {
            const int32_t c = int32_t(__popcll(__ballot((word >> g) & 1u)));
            if (lane == g) mine += c;
        }
    }
    const int64_t jm = int64_t(sg.w) * kWB + lane;
    if (lane < kWB && jm < F.m) col_cnt[(jm * F.d + sg.j) * F.nt + sg.t] = mine;
}

__global__ __launch_bounds__(kRowThreads) void relu_sp_row_count_kernel(const uint32_t* __restrict__ bits, const int64_t* __restrict__ zrptr,
                                                                        int64_t n, int64_t words, int gated,
                                                                        int64_t* __restrict__ row_cnt) {
    const int64_t i = int64_t(blockIdx.x) * kRowThreads + threadIdx.x;
    if (i >= n) return;
    int64_t pc = 0;
    for (int64_t w = 0; w < words; ++w) pc += __popc(bits[w * n + i]);
    row_cnt[i] = (gated ? 1 : 2) * pc * (zrptr[i + 1] - zrptr[i]);
}

template <class T>
__global__ __launch_bounds__(64) void relu_sp_col_fill_kernel(ReluCscView<T> F, const int64_t* __restrict__ col_pos,
                                                              int32_t* __restrict__ cidx, T* __restrict__ cval) {
    const int lane = threadIdx.x;
    const Seg sg = relu_sp_seg(F);
    const uint32_t* __restrict__ bw = F.bits + int64_t(sg.w) * F.n;
    const int64_t md = F.m * F.d;
    // lane g: where the segment of gate g starts in the unsigned half, and how far the signed half's lies behind it
    const int64_t jm_l = int64_t(sg.w) * kWB + lane;
    const bool gate_l = lane < kWB && jm_l < F.m;
    const int64_t c_l = gate_l ? jm_l * F.d + sg.j : 0;
    int64_t pos_l = gate_l ? col_pos[c_l * F.nt + sg.t] : 0;
    const int64_t neg_l = (gate_l && !F.gated) ? col_pos[(md + c_l) * F.nt + sg.t] - pos_l : 0;
    const unsigned long long lower = (1ull << lane) - 1;
    for (int64_t kb = sg.k0; kb < sg.k1; kb += 64) { // (uniform over the wave)
        const int64_t k = kb + lane;
        const bool in = k < sg.k1;
        const int32_t i = in ? F.zidx[k] : 0;
        const T z = in ? F.zval[k] : T(0);
        const uint32_t word = in ? bw[i] : 0u;
#pragma unroll
        for (int g = 0; g < kWB; ++g) {
            const bool hit = (word >> g) & 1u;
            const unsigned long long b = __ballot(hit);
            if (!b) continue; // (uniform)
            const int64_t start = __shfl(pos_l, g);
            const int64_t neg = __shfl(neg_l, g);
            if (hit) {
                const int64_t at = start + __popcll(b & lower);
                cidx[at] = i;
                cval[at] = z;
                if (!F.gated) {
                    cidx[at + neg] = i;
                    cval[at + neg] = -z;
                }
            }
            if (lane == g) pos_l += __popcll(b);
        }
    }
}

template <class T>
__global__ __launch_bounds__(64 * kRowWaves) void relu_sp_row_fill_kernel(ReluCscView<T> F, const int64_t* __restrict__ zrptr,
                                                                         const int32_t* __restrict__ zrcol, const T* __restrict__ zrval,
                                                                         const int64_t* __restrict__ rptr, int32_t* __restrict__ rcol,
                                                                         T* __restrict__ rval, int64_t words) {
    const int lane = threadIdx.x & 63;
    const int64_t i = int64_t(blockIdx.x) * kRowWaves + (threadIdx.x >> 6);
    if (i >= F.n) return;
    const int64_t k0 = zrptr[i], nz = zrptr[i + 1] - k0;
    if (nz == 0) return;
    int64_t pc = 0;
    for (int64_t w = 0; w < words; ++w) pc += __popc(F.bits[w * F.n + i]);
    const int64_t base = rptr[i], md = F.m * F.d;
    int64_t rank = 0; // set gates before this one
    for (int64_t w = 0; w < words; ++w) {
        uint32_t word = F.bits[w * F.n + i]; // (uniform over the wave)
        while (word) {
            const int g = __ffs(int(word)) - 1;
            word &= word - 1;
            const int64_t c0 = (w * kWB + g) * F.d;
            int32_t* oc = rcol + base + rank * nz;
            T* ov = rval + base + rank * nz;
            for (int64_t k = lane; k < nz; k += 64) {
                const int32_t c = zrcol[k0 + k];
                const T z = zrval[k0 + k];
                oc[k] = int32_t(c0 + c);
                ov[k] = z;
                if (!F.gated) {
                    oc[pc * nz + k] = int32_t(md + c0 + c);
                    ov[pc * nz + k] = -z;
                }
            }
            ++rank;
        }
    }
}

// NG gates of the word are summed (NG = 8 when the whole mask has no more): lane l of step s holds entry k0 + 64 s + l.
template <class T, int NG>
__global__ __launch_bounds__(64) void relu_sp_sweep_kernel(ReluCscView<T> F, const T* __restrict__ v, T* __restrict__ part) {
    const int lane = threadIdx.x;
    const Seg sg = relu_sp_seg(F);
    const uint32_t* __restrict__ bw = F.bits + int64_t(sg.w) * F.n;
    T acc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = T(0);
    for (int64_t k = sg.k0 + lane; k < sg.k1; k += 64) {
        const int32_t i = F.zidx[k];
        const T zv = F.zval[k] * v[i];
        const uint32_t word = bw[i];
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] += ((word >> g) & 1u) ? zv : T(0); // a select: a masked-out entry is not stored
    }
    // The lanes' sums in a fixed order, as a transposing butterfly: at distance 32, 16, ... a lane keeps one half of its gates and
    // hands the other half to its partner, so the exchanges halve with every step (NG - 1 in all, not 6 NG); the distances
    // left once one gate remains are plain butterfly steps.  Lane l ends with the sum of gate l >> kRest.
    constexpr int kRest = 6 - (NG == 32 ? 5 : NG == 16 ? 4 : NG == 8 ? 3 : -100);
    static_assert(kRest >= 0, "NG is 8, 16 or 32");
    int off = 32;
#pragma unroll
    for (int half = NG / 2; half >= 1; half >>= 1) {
        const bool hi = (lane & off) != 0;
#pragma unroll
        for (int g = 0; g < half; ++g) {
            const T send = hi ? acc[g] : acc[g + half];
            const T keep = hi ? acc[g + half] : acc[g];
            acc[g] = keep + __shfl_xor(send, off);
        }
        off >>= 1;
    }
    T mine = acc[0];
#pragma unroll
    for (int r = 0; r < kRest; ++r) {
        mine += __shfl_xor(mine, off);
        off >>= 1;
    }
    const int64_t jm = int64_t(sg.w) * kWB + (lane >> kRest);
    if ((lane & ((1 << kRest) - 1)) == 0 && jm < F.m) part[int64_t(sg.t) * (F.m * F.d) + jm * F.d + sg.j] = mine;
}

template <class T>
__global__ __launch_bounds__(256) void relu_sp_reduce_kernel(const T* __restrict__ part, T* __restrict__ out, int64_t md, int nt, int gated,
                                                             const T* __restrict__ sub_scale, const T* __restrict__ sub_vec) {
    const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (c >= md) return;
    T s = part[c];
    for (int t = 1; t < nt; ++t) s += part[int64_t(t) * md + c];
    T pos = s, neg = -s;
    if (sub_vec) {
        pos -= sub_scale[0] * sub_vec[c];
        if (!gated) neg -= sub_scale[0] * sub_vec[md + c];
    }
    out[c] = pos;
    if (!gated) out[md + c] = neg;
}

// one wavefront per (column of Z, tile) in x and per word in y
template <class T>
dim3 seg_grid(const ReluCscView<T>& F) {
    const int64_t gx = F.d * int64_t(F.nt), words = (F.m + kWB - 1) / kWB;
    if (gx >= (int64_t(1) << 31) || words > 65535)
        throw std::runtime_error("adelie_hip: convex_relu(): too many (column of Z, row tile) pairs or mask words for one launch.");
    return dim3(unsigned(gx), unsigned(words));
}

inline unsigned row_blocks(int64_t n, int per) { return unsigned((n + per - 1) / per); }

} // namespace

void launch_relu_sparse_pack(const uint8_t* mask, int64_t n, int64_t m, uint32_t* bits, hipStream_t s) {
    const int64_t words = (m + kWB - 1) / kWB;
    if (n <= 0 || words <= 0) return;
    if (words > 65535) throw std::runtime_error("adelie_hip: convex_relu(): too many mask words for one launch.");
    hipLaunchKernelGGL(relu_sp_pack_kernel, dim3(row_blocks(n, kRowThreads), unsigned(words)), dim3(kRowThreads), 0, s, mask, n, m, bits);
}

template <class T>
void launch_relu_sparse_count(const ReluCscView<T>& F, const int64_t* zrptr, int32_t* col_cnt, int64_t* row_cnt, hipStream_t s) {
    if (F.n <= 0 || F.d <= 0 || F.m <= 0) return;
    hipLaunchKernelGGL((relu_sp_col_count_kernel<T>), seg_grid(F), dim3(64), 0, s, F, col_cnt);
    hipLaunchKernelGGL(relu_sp_row_count_kernel, dim3(row_blocks(F.n, kRowThreads)), dim3(kRowThreads), 0, s, F.bits, zrptr, F.n,
                       (F.m + kWB - 1) / kWB, F.gated, row_cnt);
}

template <class T>
void launch_relu_sparse_fill(const ReluCscView<T>& F, const int64_t* zrptr, const int32_t* zrcol, const T* zrval, const int64_t* col_pos,
                             const int64_t* rptr, int32_t* cidx, T* cval, int32_t* rcol, T* rval, hipStream_t s) {
    if (F.n <= 0 || F.d <= 0 || F.m <= 0) return;
    hipLaunchKernelGGL((relu_sp_col_fill_kernel<T>), seg_grid(F), dim3(64), 0, s, F, col_pos, cidx, cval);
    hipLaunchKernelGGL((relu_sp_row_fill_kernel<T>), dim3(row_blocks(F.n, kRowWaves)), dim3(64 * kRowWaves), 0, s, F, zrptr, zrcol, zrval,
                       rptr, rcol, rval, (F.m + kWB - 1) / kWB);
}

template <class T>
void launch_sweep_relu_sparse(const ReluCscView<T>& F, const T* v, T* out, const T* sub_scale, const T* sub_vec, T* work, hipStream_t s) {
    if (F.d <= 0 || F.m <= 0) return;
    const int64_t md = F.m * F.d;
    const dim3 grid = seg_grid(F);
    if (F.m <= 8) hipLaunchKernelGGL((relu_sp_sweep_kernel<T, 8>), grid, dim3(64), 0, s, F, v, work);
    else hipLaunchKernelGGL((relu_sp_sweep_kernel<T, kWB>), grid, dim3(64), 0, s, F, v, work);
    hipLaunchKernelGGL((relu_sp_reduce_kernel<T>), dim3(row_blocks(md, 256)), dim3(256), 0, s, work, out, md, F.nt, F.gated, sub_scale,
                       sub_vec);
}

#define INST(T)                                                                                                                      \
    template void launch_relu_sparse_count<T>(const ReluCscView<T>&, const int64_t*, int32_t*, int64_t*, hipStream_t);               \
    template void launch_relu_sparse_fill<T>(const ReluCscView<T>&, const int64_t*, const int32_t*, const T*, const int64_t*,        \
                                             const int64_t*, int32_t*, T*, int32_t*, T*, hipStream_t);                               \
    template void launch_sweep_relu_sparse<T>(const ReluCscView<T>&, const T*, T*, const T*, const T*, T*, hipStream_t);
INST(double)
INST(float)
#undef INST

} // namespace ahip
