// accessors.hpp — column accessors shared by the streaming and Gram kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "pieces_host.hpp"

namespace ahip {

typedef double d2_t __attribute__((ext_vector_type(2)));
typedef float f4_t __attribute__((ext_vector_type(4)));
template <class T> struct VecOf;
template <> struct VecOf<double> { using type = d2_t; static constexpr int N = 2; };
template <> struct VecOf<float> { using type = f4_t; static constexpr int N = 4; };

template <class T, int VEC> struct Pack { T v[VEC]; };

// ---- column accessors ---------------------------------------------------------------------------
template <class T>
struct DenseAcc {
    const T* X;
    int64_t ld;
    __device__ __forceinline__ const T* colptr(int64_t j) const { return X + j * ld; }
    template <int VEC>
    __device__ __forceinline__ Pack<T, VEC> load(const T* col, int64_t i, int64_t /*j*/) const {
        Pack<T, VEC> r;
        if constexpr (VEC == 1) {
            r.v[0] = col[i];
        } else {
            using V = typename VecOf<T>::type;
            V x = __builtin_nontemporal_load(reinterpret_cast<const V*>(col + i));
#pragma unroll
            for (int e = 0; e < VEC; ++e) r.v[e] = x[e];
        }
        return r;
    }
};

// Dense design preceded by `shift` (0 or 1) columns of ones: the "extended features" of the multi-response view
// [1 (x) I_K, X (x) I_K] (kernels_multi.hip).  Same interface as DenseAcc, so the MFMA syrk kernel takes it unchanged.
template <class T>
struct DenseOnesAcc {
    const T* X;
    int64_t ld;
    const T* ones;
    int64_t shift;
    __device__ __forceinline__ const T* colptr(int64_t u) const { return u < shift ? ones : X + (u - shift) * ld; }
    template <int VEC>
    __device__ __forceinline__ Pack<T, VEC> load(const T* col, int64_t i, int64_t /*j*/) const {
        Pack<T, VEC> r;
        if constexpr (VEC == 1) {
            r.v[0] = col[i];
        } else {
            using V = typename VecOf<T>::type;
            V x = __builtin_nontemporal_load(reinterpret_cast<const V*>(col + i));
#pragma unroll
            for (int e = 0; e < VEC; ++e) r.v[e] = x[e];
        }
        return r;
    }
};

// 2-bit SNP calls: value = code<3 ? code : impute[j]   (matrix_naive_snp_unphased.ipp:8-22 semantics)
// VEC calls of one column from row i on (VEC == 2: i even, VEC == 4: i a multiple of 4), a missing call giving `imp`
template <class T, int VEC>
__device__ __forceinline__ Pack<T, VEC> snp_decode(const uint8_t* col, int64_t i, T imp) {
    Pack<T, VEC> r;
    if constexpr (VEC == 1) {
        const unsigned c = (col[i >> 2] >> (2 * (i & 3))) & 3u;
        r.v[0] = c == 3u ? imp : T(c);
    } else if constexpr (VEC == 2) {
        const unsigned byte = col[i >> 2] >> (2 * (i & 3)); // i even
#pragma unroll
        for (int k = 0; k < 2; ++k) { const unsigned c = (byte >> (2 * k)) & 3u; r.v[k] = c == 3u ? imp : T(c); }
    } else {
        const unsigned byte = col[i >> 2]; // i multiple of 4
#pragma unroll
        for (int k = 0; k < 4; ++k) { const unsigned c = (byte >> (2 * k)) & 3u; r.v[k] = c == 3u ? imp : T(c); }
    }
    return r;
}
template <class T>
struct SnpAcc {
    const uint8_t* bits;
    int64_t ldb;
    const T* impute;
    __device__ __forceinline__ const uint8_t* colptr(int64_t j) const { return bits + j * ldb; }
    template <int VEC>
    __device__ __forceinline__ Pack<T, VEC> load(const uint8_t* col, int64_t i, int64_t j) const {
        return snp_decode<T, VEC>(col, i, impute[j]);
    }
};

// 2-bit SNP design preceded by `shift` (0 or 1) columns of ones: the extended features of the multi-response view over an
// SNP base.  Same interface as SnpAcc (the K-wide sweep and the MFMA Gram kernels take it unchanged); the ones columns are
// never dereferenced.
template <class T>
struct SnpOnesAcc {
    const uint8_t* bits;
    int64_t ldb;
    const T* impute;
    int64_t shift;
    __device__ __forceinline__ const uint8_t* colptr(int64_t u) const { return u < shift ? bits : bits + (u - shift) * ldb; }
    template <int VEC>
    __device__ __forceinline__ Pack<T, VEC> load(const uint8_t* col, int64_t i, int64_t u) const {
        if (u < shift) {
            Pack<T, VEC> r;
#pragma unroll
            for (int e = 0; e < VEC; ++e) r.v[e] = T(1);
            return r;
        }
        return SnpAcc<T>{bits, ldb, impute}.template load<VEC>(col, i, u - shift);
    }
};

// A design made of up to kMaxPieces column blocks, each a dense or a 2-bit design that stays as it is (pieces_host.hpp;
// adelie_hip_design_create_pieces).  The table travels by value in the kernel arguments.  colptr finds the piece of a column
// with a scan of the first columns -- every slot is read at a fixed index and chosen by compares, so nothing is indexed at run
// time -- and returns the column's base with where its impute value stands (null: a dense piece); load then runs DenseAcc's or
// SnpAcc's code.  In the sweep, axpy and sp_tmul kernels a column is the same for every lane of a load, so the branch is
// uniform; in the MFMA Gram kernels neighbouring lanes may hold columns of both kinds and diverge.
template <class T>
struct PiecesAcc {
    const void* base[kMaxPieces];  // dense: T*, leading dimension ld elements; 2-bit: the calls, ld bytes per column
    int64_t ld[kMaxPieces];
    const T* impute[kMaxPieces];   // 2-bit pieces: (p_piece,) values of a missing call; dense pieces: null
    int32_t first[kMaxPieces + 1]; // first column of each piece; unused slots hold INT32_MAX
    struct Col {
        const void* p;
        const T* imp;
    };
    // (a recursion over the slot with every slot read before it is chosen: the indices are constants and the reads
    // unconditional, so the by-value table is read where the kernel arguments stand -- a loop, or a read under the compare, had
    // the compiler copy the table to 200 bytes of scratch per lane and index it there)
    template <int M>
    __device__ __forceinline__ void pick(int64_t j, const void*& b, int64_t& l, const T*& im, int64_t& f) const {
        if constexpr (M < kMaxPieces) {
            const void* bm = base[M];
            const int64_t lm = ld[M], fm = first[M];
            const T* imm = impute[M];
            const bool at = j >= fm;
            b = at ? bm : b, l = at ? lm : l, im = at ? imm : im, f = at ? fm : f;
            pick<M + 1>(j, b, l, im, f);
        }
    }
    __device__ __forceinline__ Col colptr(int64_t j) const {
        const void* b = base[0];
        int64_t l = ld[0], f = 0;
        const T* im = impute[0];
        pick<1>(j, b, l, im, f);
        const int64_t jl = j - f;
        if (im) return Col{static_cast<const uint8_t*>(b) + jl * l, im + jl};
        return Col{static_cast<const T*>(b) + jl * l, nullptr};
    }
    template <int VEC>
    __device__ __forceinline__ Pack<T, VEC> load(const Col& c, int64_t i, int64_t /*j*/) const {
        if (c.imp) return snp_decode<T, VEC>(static_cast<const uint8_t*>(c.p), i, *c.imp);
        return DenseAcc<T>{nullptr, 0}.template load<VEC>(static_cast<const T*>(c.p), i, 0);
    }
};
// the accessor of a PiecesView (kernels.hpp), whose tables it copies
template <class T, class View>
inline PiecesAcc<T> pieces_acc(const View& X) {
    PiecesAcc<T> a;
    for (int m = 0; m < kMaxPieces; ++m) a.base[m] = X.base[m], a.ld[m] = X.ld[m], a.impute[m] = X.impute[m];
    for (int m = 0; m <= kMaxPieces; ++m) a.first[m] = X.first[m];
    return a;
}

} // namespace ahip
