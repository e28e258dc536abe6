// kernels.hpp — launch interface of the gfx950 kernels (implemented in kernels_*.hip).
// Everything here works on DEVICE pointers and enqueues on the given HIP stream; no host sync.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gram_shape.hpp"
#include "multi_shape.hpp"
#include "relu_shape.hpp"
#include "relu_sparse_shape.hpp"
#include "shadow_kind_host.hpp"
#include "pieces_host.hpp"

namespace ahip {

// Dense column-major design in HBM: element (i,j) at X[i + j*ld].
template <class T>
struct DenseView {
    const T* X;
    int64_t n, p, ld;
};
// SNP design: 2-bit calls, column-major, 4 calls per byte (row i of column j in byte (i>>2) of
// the column, bits 2*(i&3)); code 0 -> 0, 1 -> 1, 2 -> 2, 3 -> missing (impute[j]).
struct SnpView {
    const uint8_t* bits;
    int64_t n, p, ldb; // ldb = bytes per column (padded)
};

// Design made of k <= kMaxPieces column blocks that stay as they are (pieces_host.hpp): piece m holds columns
// [first[m], first[m + 1]) and is a dense design (impute[m] null; X = base[m], leading dimension ld[m]) or a 2-bit design (bits =
// base[m], ldb = ld[m], impute[m] its (p_m,) values).  Unused slots: base / impute null, first INT32_MAX.
template <class T>
struct PiecesView {
    const void* base[kMaxPieces];
    int64_t ld[kMaxPieces];
    const T* impute[kMaxPieces];
    int32_t first[kMaxPieces + 1];
    int k;
    int64_t n, p;
    bool is_snp(int m) const { return impute[m] != nullptr; }
    int64_t cols_of(int m) const { return int64_t(first[m + 1]) - int64_t(first[m]); }
    DenseView<T> dense_piece(int m) const { return DenseView<T>{static_cast<const T*>(base[m]), n, cols_of(m), ld[m]}; }
    SnpView snp_piece(int m) const { return SnpView{static_cast<const uint8_t*>(base[m]), n, cols_of(m), ld[m]}; }
    // whether the kernels over PiecesAcc may read 16 bytes at a time (pieces_host.hpp: pieces_vec_ok)
    bool vec_ok() const {
        int kind[kMaxPieces];
        uintptr_t at[kMaxPieces];
        for (int m = 0; m < k; ++m) kind[m] = is_snp(m) ? kPieceSnp : kPieceDense, at[m] = reinterpret_cast<uintptr_t>(base[m]);
        return pieces_vec_ok(kind, at, ld, k, int(16 / sizeof(T)));
    }
};

// Sparse design kept sparse (kernels_sparse.hip): the same matrix column-compressed (cptr / cidx / cval, row indices ascending
// inside a column) and row-compressed (rptr / rcol / rval).
template <class T>
struct CscView {
    const int64_t* cptr;
    const int32_t* cidx;
    const T* cval;
    const int64_t* rptr;
    const int32_t* rcol;
    const T* rval;
    int64_t n, p, nnz;
    // row blocks of rb rows for the sweeps (nb > 1): bptr[c * (nb + 1) + b] = first entry of column c with row >= b * rb
    const int64_t* bptr;
    int nb;
    int64_t rb;
    // standardized view (both null: the plain matrix): the design is (x_ij - center[j]) * inv_scale[j], entries untouched
    const T* center;
    const T* inv_scale;
    // tile-major copy for the full sweeps (nt > 0): the entries of row tile t (th rows) stand together, by column;
    // tptr[t * (p + 1) + c] = first entry of (tile t, column c), trow = row inside the tile, tval = value
    const int64_t* tptr;
    const uint16_t* trow;
    const T* tval;
    int nt;
    int64_t th;
};

// ---- vector helpers -------------------------------------------------------------------------
// out[i] = a[i] * b[i]
template <class T> void launch_vmul(const T* a, const T* b, T* out, int64_t n, hipStream_t s);
template <class T> void launch_fill(T* out, T value, int64_t n, hipStream_t s);

// ---- sweep: out[c] = sum_i X[i, col(c)] * v[i]  (col(c) = cols ? cols[c] : c0 + c) --------------
// epilogue: out[c] -= sub_scale[0] * sub_vec[col(c)] when sub_vec != nullptr (sub_scale is a DEVICE scalar)
// square: use X^2 instead of X (sq_mul).  `work` must hold sweep_work_elems(n, ncols) elements.
template <class T>
void launch_sweep(const DenseView<T>& X, const T* v, T* out, int64_t c0, int64_t ncols, const int32_t* cols,
                  const T* sub_scale, const T* sub_vec, bool square, T* work, hipStream_t s);
template <class T>
void launch_sweep_snp(const SnpView& X, const T* impute, const T* v, T* out, int64_t c0, int64_t ncols,
                      const int32_t* cols, const T* sub_scale, const T* sub_vec, bool square, T* work, hipStream_t s);
int64_t sweep_work_elems(int64_t n, int64_t ncols);
// The same operations on a design made of pieces (kernels_sweep.hip, kernels_gram.hip).  A sweep over a column range
// (cols == nullptr) is issued piece by piece with launch_sweep / launch_sweep_snp on the piece's part of the range: every block
// runs at the rate its storage has and a column's value is what its piece alone gives.  A sweep over a column list, Gram, axpy
// and sp_tmul run the kernels above over PiecesAcc (accessors.hpp).  `work` holds sweep_work_elems_pieces(X, c0, ncols) elements.
template <class T>
void launch_sweep_pieces(const PiecesView<T>& X, const T* v, T* out, int64_t c0, int64_t ncols, const int32_t* cols,
                         const T* sub_scale, const T* sub_vec, bool square, T* work, hipStream_t s);
template <class T> int64_t sweep_work_elems_pieces(const PiecesView<T>& X, int64_t c0, int64_t ncols);
template <class T>
void launch_axpy_cols_pieces(const PiecesView<T>& X, const int32_t* cols, const T* coef, const int32_t* count_dev, int32_t count,
                             T sign, T* out, hipStream_t s);
template <class T>
void launch_sp_tmul_pieces(const PiecesView<T>& X, int64_t L, const int64_t* indptr, const int64_t* indices, const T* values,
                           T* out, hipStream_t s);
// launch_gram below on a design made of pieces; `work` holds gram_work_elems(n, M, N) elements
template <class T>
void launch_gram_pieces(const PiecesView<T>& X, const T* w, const int32_t* mcols, int32_t M, int32_t m_pos0, const int32_t* ncols,
                        int32_t N, int32_t n_pos0, const T* xm_by_col, bool center, T* C, int64_t ldc, T* work, hipStream_t s);

// ---- filtered invariance sweep (kernels_filter.hip): a float32 shadow of a dense f64 design ----------------------------------
// Xs: the columns rounded to float32 (column-major, ld a multiple of 4); err[j] = ||x_j - xs_j||_2, nrm[j] = ||xs_j||_2 (both
// rounded up).  |x_j.v - xs_j.v| as the two sweeps compute them differ by at most (err[j] + fp_term() * nrm[j]) * ||v||_2.
// kind kShadowQ15 (shadow_kind_host.hpp): X holds int16 q_ij = rint(x_ij * (32767 / max_i |x_ij|)) clamped to +-32767 (column-major, ld
// a multiple of 64, pad rows 0) and scale[j] = max_i |x_ij| / 32767; xs_j = scale[j] q_j in the two definitions above.
struct ShadowView {
    const void* X; // float (kShadowF32) or int16_t (kShadowQ15)
    int64_t n, p, ld;
    const double* err;
    const double* nrm;
    int kind = kShadowF32;
    const double* scale = nullptr; // (p,) q15 only
    // float32: 4 n 2^-53, both accumulations' rounding.  q15: (4 n + 8) 2^-53, derived at ShadowQ15 (kernels_filter.hip).
    double fp_term() const { return (4.0 * double(n) + (kind == kShadowQ15 ? 8.0 : 0.0)) * 1.1102230246251565e-16; }
    double elem_bytes() const { return kind == kShadowQ15 ? 2.0 : 4.0; }
};
// makes the copy and measures err / nrm; *bad |= 1 when an entry is not finite or beyond FLT_MAX
void launch_shadow_build(const DenseView<double>& X, float* Xs, int64_t lds, double* err, double* nrm, int32_t* bad, hipStream_t s);
// the q15 copy: lds = shadow_q15_ld(n); *bad |= 1 when an entry is not finite (any finite entry can be held)
int64_t shadow_q15_ld(int64_t n);
void launch_shadow_build_q15(const DenseView<double>& X, int16_t* Xq, int64_t lds, double* scale, double* err, double* nrm,
                             int32_t* bad, hipStream_t s);
// how many fixed-order partial sums of (w o r)^2 one filtered sweep leaves in sq_part
int filter_norm_parts(int64_t n);
// One filtered invariance sweep, all device pointers.  In order on one stream:
//   v = w o r and the partial sums of its squares;
//   one launch that sweeps the shadow over all columns into grad and, in workgroups of its own, sweeps in f64 the columns
//   that are exact whatever the shadow says (screen_cols, then pen0_cols: the groups without a penalty) into staging;
//   the classification: ||v||, the staged columns reduced, compared with their shadow values and stored, and the columns of
//   the groups that tstar cannot place listed (kernels_filter.hip, filter_classify_kernel, also for meta_i / meta_d);
//   the f64 sweep of the listed columns.
// Every f64 value is the bits launch_sweep over all X.p columns gives that column.
struct FilteredSweep {
    const double *w, *r;
    double* v;                          // n
    double* grad;                       // p
    const double *sub_scale, *sub_vec;  // grad[c] -= sub_scale[0] * sub_vec[c] (sub_vec == nullptr: no such term)
    const int32_t* screen_cols;
    int64_t n_screen_cols;
    const int32_t* pen0_cols;
    int64_t n_pen0_cols;
    const int64_t *groups, *group_sizes;
    int64_t G;
    const int32_t* slot;                // per group: >= 0 in the screen set
    const double* penalty;
    double tstar;
    double* sq_part;                    // filter_norm_parts(n)
    int32_t* list;                      // cap
    int64_t cap;
    int32_t* meta_i;                    // 4
    double* meta_d;                     // 2
    double* work;                       // filtered_sweep_work_elems(n, p, n_screen_cols + n_pen0_cols, cap)
};
int64_t filtered_sweep_work_elems(int64_t n, int64_t p, int64_t n_before, int64_t cap);
void enqueue_filtered_sweep(const DenseView<double>& X, const ShadowView& S, const FilteredSweep& a, hipStream_t s);
// sparse design: one wavefront per (column, row block) over its stored entries; `work` holds sweep_work_elems_csc(X.nb, ncols)
int64_t sweep_work_elems_csc(int nb, int64_t ncols);
template <class T>
void launch_sweep_csc(const CscView<T>& X, const T* v, T* out, int64_t c0, int64_t ncols, const int32_t* cols,
                      const T* sub_scale, const T* sub_vec, bool square, T* work, hipStream_t s);
// Pieces of the standardized view (x_ij - center[j]) * inv_scale[j] over ANY base design (kernels_sparse.hip): the solver composes
// the base design's raw sweep / Gram / axpy with them.
// out[0] = sum_i v[i], fixed order; `out` holds kVecSumScratch elements (the result, then the chunk sums)
constexpr int kVecSumScratch = 8 + 256;
template <class T> void launch_vec_sum(const T* v, int64_t n, T* out, hipStream_t s);
template <class T>
void launch_std_sweep_epilogue(const T* center, const T* inv_scale, const T* raw, const T* raw_plain, const T* vsum, bool square,
                               T* out, int64_t c0, int64_t ncols, const int32_t* cols, const T* sub_scale, const T* sub_vec,
                               hipStream_t s);
template <class T>
void launch_std_gram_fix(const T* center, const T* inv_scale, T* C, int64_t ldc, int32_t M, int32_t pos0, int32_t N,
                         const int32_t* vcol, const T* m, const T* wsum, const T* xm, bool centered, hipStream_t s);
template <class T>
void launch_std_scale_coef(const T* center, const T* inv_scale, const int32_t* cols, const T* coef, const int32_t* count_dev,
                           int32_t count, T* coef2, T* kappa, hipStream_t s);
template <class T> void launch_vec_shift(T* out, int64_t n, const T* kappa, T sign, const int32_t* count_dev, hipStream_t s);
// panel engine on a standardized view: a block's gradient from the raw sums, a batch of diagonal blocks from the raw X' W X
template <class T>
void launch_std_fix_gblk(T* gblk, const int32_t* cols, int nb, const T* center, const T* inv_scale, const T* rsum_dev,
                         const T* xm_view_or_null, hipStream_t s);
struct SyrkBatch;
template <class T>
void launch_std_block_fix(T* D0, const SyrkBatch& sb, const int32_t* cols_base, int ldb, const T* center, const T* inv_scale,
                          const T* xm_view, const T* wsum_dev, bool centered, hipStream_t s);
// tile-major copy of a sparse design (see CscView): from the per-column tile pointers colptr[c * (nt + 1) + t] (what
// launch_csc_block_ptr gives with rb = th) and the tile-major offsets tptr, the entries are copied to their places
template <class T>
void launch_csc_tile_scatter(const int64_t* colptr, const int32_t* cidx, const T* cval, int64_t p, int nt, int64_t th,
                             const int64_t* tptr, uint16_t* trow, T* tval, hipStream_t s);
constexpr int64_t kCscTileBytes = 128 * 1024; // a tile of v in LDS
// row-block layout of a sparse design with n rows (blocks whose slice of an n-vector is about 1 MB, at most 64 of them) and
// the per-column block pointers
void csc_block_layout(int64_t n, size_t value_size, int* nb, int64_t* rb);
void launch_csc_block_ptr(const int64_t* cptr, const int32_t* cidx, int64_t p, int nb, int64_t rb, int64_t* bptr, hipStream_t s);
// launch_gram on a sparse design; `work` holds gram_work_elems_csc(n, M, N, X.nb) elements
int64_t gram_work_elems_csc(int64_t n, int64_t M, int64_t N, int nb);
template <class T>
void launch_gram_csc(const CscView<T>& X, const T* w, const int32_t* mcols, int32_t M, int32_t m_pos0, const int32_t* ncols,
                     int32_t N, int32_t n_pos0, const T* xm_by_col, bool center, T* C, int64_t ldc, T* work, hipStream_t s);
// launch_axpy_cols on a sparse design (cols must be distinct); `delta_zeroed`: p + 8 elements, the first p all zero on entry and on exit
template <class T>
void launch_axpy_cols_csc(const CscView<T>& X, const int32_t* cols, const T* coef, const int32_t* count_dev, int32_t count,
                          T sign, T* out, T* delta_zeroed, hipStream_t s);
// launch_sp_tmul on a sparse design; `work` holds sp_tmul_work_elems_csc(p) elements
int64_t sp_tmul_work_elems_csc(int64_t p);
template <class T>
void launch_sp_tmul_csc(const CscView<T>& X, int64_t L, const int64_t* indptr, const int64_t* indices, const T* values, T* out,
                        T* work, hipStream_t s);

// ---- panel axpy: out[i] += sign * sum_k coef[k] * X[i, cols[k]],  k < *count_dev (or count if count_dev null)
template <class T>
void launch_axpy_cols(const DenseView<T>& X, const int32_t* cols, const T* coef, const int32_t* count_dev,
                      int32_t count, T sign, T* out, hipStream_t s);
template <class T>
void launch_axpy_cols_snp(const SnpView& X, const T* impute, const int32_t* cols, const T* coef,
                          const int32_t* count_dev, int32_t count, T sign, T* out, hipStream_t s);
// batched variant for sp_tmul: out (L,n) row-major, CSR (indptr,indices,values) on device
template <class T>
void launch_sp_tmul(const DenseView<T>& X, int64_t L, const int64_t* indptr, const int64_t* indices, const T* values,
                    T* out, hipStream_t s);
template <class T>
void launch_sp_tmul_snp(const SnpView& X, const T* impute, int64_t L, const int64_t* indptr, const int64_t* indices,
                        const T* values, T* out, hipStream_t s);

// ---- product of two column-major matrices over their common rows (kernels_pinball.hip, plain LDS tiles):
//   C[r + c*ldc] = sum_{i<K} P[i + pcol(r)*ldp] * Q[i + qcol(c)*ldq],  r < M, c < N,  pcol(r) = pcols ? pcols[r] : r
template <class T>
void launch_ptq(const T* P, int64_t ldp, const int32_t* pcols, int32_t M, const T* Q, int64_t ldq, const int32_t* qcols, int32_t N,
                int64_t K, T* C, int64_t ldc, hipStream_t s);
// The same products where the (d, m) matrix A' is kept sparse (kernels_pinball_sparse.hip), a row of A being compressed column
// col of A (entries e, stored indices ascending); every element is one ascending sum in one accumulator, as in launch_ptq:
//   AS[r + c*ld]  = sum_e val_e ST[r + idx_e*d],    r < d = A.n, c < N, col = cols ? cols[c] : c    (ST: S' column-major)
//   C[r + c*ldc]  = sum_e val_e Q[idx_e + c*ldq],   r < M, c < N,       col = pcols ? pcols[r] : r
template <class T>
void launch_csc_rows_dense(const CscView<T>& A, const int32_t* cols, int64_t N, const T* ST, T* AS, int64_t ld, hipStream_t s);
template <class T>
void launch_csc_rows_cols(const CscView<T>& A, const int32_t* pcols, int64_t M, const T* Q, int64_t ldq, int64_t N, T* C,
                          int64_t ldc, hipStream_t s);
// out[c + r*d] = in[r + c*d]: the transposed copy of a (d, d) column-major matrix
template <class T> void launch_transpose_square(const T* in, int64_t d, T* out, hipStream_t s);

// ---- Gram (MFMA): for a in [0,M), b in [0,N):
//   C[rowpos[a] + colpos[b]*ldc] = sum_i w[i] X[i,mcols[a]] X[i,ncols[b]]  - (center ? xm[mcols[a]]*xm[ncols[b]] : 0)
// where rowpos[a] = m_pos0 + a, colpos[b] = n_pos0 + b.  The mirror entry C[colpos[b] + rowpos[a]*ldc] gets the same value when
// ncols is the tail of mcols at the same positions (the symmetric append); launch_gram_csc writes it on every call.
// `work` holds gram_work_elems(...) elements.
template <class T>
void launch_gram(const DenseView<T>& X, const T* w, const int32_t* mcols, int32_t M, int32_t m_pos0,
                 const int32_t* ncols, int32_t N, int32_t n_pos0, const T* xm_by_col, bool center, T* C, int64_t ldc,
                 T* work, hipStream_t s);
template <class T>
void launch_gram_snp(const SnpView& X, const T* impute, const T* w, const int32_t* mcols, int32_t M, int32_t m_pos0,
                     const int32_t* ncols, int32_t N, int32_t n_pos0, const T* xm_by_col, bool center, T* C,
                     int64_t ldc, T* work, hipStream_t s);
// gram_work_elems(n, M, N): gram_shape.hpp, like every *_work_elems of the MFMA block builds below
// What the last block build launched by this host thread ran (the kernel-level test entry reports it).
BuildLaunchInfo& last_build_launch();
// symmetric diagonal block of M <= 128 columns: C[a + b*ldc] = C[b + a*ldc] = sum_i w_i X[i,cols[a]] X[i,cols[b]] (- xm xm^T);
// only the lower-triangle MFMA tiles are computed.  `work` holds syrk_work_elems(n, M) elements.
// Several diagonal blocks per launch (syrk_batch_kernel): block y of the batch has the nb[y] columns cols_base[off[y]...] and
// goes to C_base + dst[y] (leading dimension ldc).  `work` holds syrk_batch_work_elems(n, count) elements.
struct SyrkBatch {
    static constexpr int MAX = 16;
    int32_t off[MAX];
    int32_t nb[MAX];
    int64_t dst[MAX];
    int32_t count;
};
// the panel engine over compressed columns (kernels_sparse.hip): the panel step (phase (A) as launch_panel_step; the block's gradient straight
// into gblk, centring included: no reduce launch) and the diagonal blocks of a batch (both triangles, leading dimension ldb)
template <class T>
void launch_panel_step_csc(const CscView<T>& X, const T* w, T* r, const int32_t* dcol, const T* dlt, const int32_t* nz_dev,
                           const int32_t* cols, int nb, const T* rsum_dev, const T* xm_by_col, T* gblk, hipStream_t s);
template <class T>
void launch_block_gram_csc(const CscView<T>& X, const T* w, const int32_t* cols_base, const SyrkBatch& sb, const T* xm_by_col,
                           bool center, T* D0, int ldb, hipStream_t s);
// Several rectangular blocks of at most 128 x 128 per launch (gram_batch_kernel; the cross blocks of the look-ahead passes):
// block y = rows cols_base[moff[y] ...] (m[y] of them) x columns cols_base[noff[y] ...] (nn[y]), X_rows^T W X_cols -
// xm_rows xm_cols^T into C_base + dst[y] (leading dimension ldc).  `work` holds gram_batch_work_elems(n, count) elements.
struct GramBatch {
    static constexpr int MAX = 16;
    int32_t moff[MAX], m[MAX], noff[MAX], nn[MAX];
    int64_t dst[MAX];
    int32_t count;
};
template <class T>
void launch_gram_batch(const DenseView<T>& X, const T* w, const int32_t* cols_base, const GramBatch& b, const T* xm_by_col,
                       bool center, T* C_base, int64_t ldc, T* work, hipStream_t s);
template <class T>
void launch_gram_batch_snp(const SnpView& X, const T* impute, const T* w, const int32_t* cols_base, const GramBatch& b,
                           const T* xm_by_col, bool center, T* C_base, int64_t ldc, T* work, hipStream_t s);
// The new rows of a panel block (kernels_strip.hip): strip y = the m[y] <= 64 columns cols_base[voff[y] ...] against the c0n[y]
// columns cols_base[c0off[y] ...] of the previous block and the c1n[y] columns cols_base[c1off[y] ...] of the block itself
// (c0n + c1n <= 256; the new columns are the last m[y] of the own block, i.e. its members [row0, row0 + m)):
//   X_base[dstX[y] + (row0 + r) + c ldc]            = v_r^T W x_c - xm xm     c <  c0n   (rows of the cross block)
//   D_base[dstD[y] + (row0 + r) + c' ldc] and mirror = v_r^T W x_c' - xm xm   c' < c1n   (rows / columns of the diagonal block)
struct StripBatch {
    static constexpr int MAX = 8;
    int32_t voff[MAX], m[MAX], c0off[MAX], c0n[MAX], c1off[MAX], c1n[MAX], row0[MAX];
    int64_t dstX[MAX], dstD[MAX];
    int32_t count;
};
void set_strip_workgroups(int wgs);         // spread of the next strip builds launched by this host thread (default kStripWgsDefault = 192, at most kStripWgsMax)
void set_strip_lds(bool on);                // f64: fragments through the wave-private LDS transpose (default) or straight from HBM
template <class T>
void launch_strip_batch(const DenseView<T>& X, const T* w, const int32_t* cols_base, const StripBatch& b, const T* xm_by_col,
                        bool center, T* D_base, T* X_base, int64_t ldc, T* work, hipStream_t s);
template <class T>
void launch_syrk_batch(const DenseView<T>& X, const T* w, const int32_t* cols_base, const SyrkBatch& b, const T* xm_by_col,
                       bool center, T* C_base, int64_t ldc, T* work, hipStream_t s);
template <class T>
void launch_syrk_batch_snp(const SnpView& X, const T* impute, const T* w, const int32_t* cols_base, const SyrkBatch& b,
                           const T* xm_by_col, bool center, T* C_base, int64_t ldc, T* work, hipStream_t s);
template <class T>
void launch_syrk(const DenseView<T>& X, const T* w, const int32_t* cols, int32_t M, const T* xm_by_col, bool center, T* C,
                   int64_t ldc, T* work, hipStream_t s);
template <class T>
void launch_syrk_snp(const SnpView& X, const T* impute, const T* w, const int32_t* cols, int32_t M, const T* xm_by_col,
                       bool center, T* C, int64_t ldc, T* work, hipStream_t s);

// ---- abs_grad (solver_base.hpp:20-110) --------------------------------------------------------
// abs_grad[g] = || grad[groups[g] : +gs] - regul_g * beta_slot ||,  regul_g = (1-alpha)*lmda*penalty[g] for screen
// groups (slot[g] >= 0 gives the value offset into screen_beta), plain norm otherwise.
template <class T>
void launch_abs_grad(const T* grad, const int64_t* groups, const int64_t* group_sizes, int64_t G, const int32_t* slot,
                     const T* screen_beta, const T* penalty, T one_minus_alpha_lmda, T* abs_grad, hipStream_t s);
// the same when some groups of one coefficient carry box constraints clo[g] <= beta <= chi[g] (+-inf: none); cmu: the
// multipliers of the screen values, mu_out (G,): every group's multiplier afterwards
template <class T>
void launch_abs_grad_cons(const T* grad, const int64_t* groups, const int64_t* group_sizes, int64_t G, const int32_t* slot, const T* screen_beta,
                          const T* penalty, T one_minus_alpha_lmda, const T* clo, const T* chi, const T* cmu, T* abs_grad,
                          T* mu_out, hipStream_t s);

// ---- coordinate descent (pin solver) ----------------------------------------------------------
enum CdStatus : int32_t {
    CD_OK = 0, CD_MAX_CDS = 1, CD_MAX_ACTIVE = 2, CD_NEWTON = 3,
    // constraint objects solved on the device (kernels_cons.hip): the errors of constraint/utils.hpp:24-243 and its sub-solvers
    CD_CONS_PN = 4, CD_CONS_QP_BOX = 5, CD_CONS_QP_NNQP = 6, CD_CONS_UNEXPECTED = 7
};
// adelie_hip_grpnet_args::constraint_native
constexpr int32_t ADELIE_HIP_NATIVE_BOX = 4, ADELIE_HIP_NATIVE_ONE_SIDED = 5, ADELIE_HIP_NATIVE_LINEAR = 6;

template <class T>
struct CdScalars { // one instance in device memory, read back by the host after the kernel
    T rsq;
    T resid_sum;
    int64_t iters;
    int64_t n_visits_screen, n_visits_active, n_updates, n_passes_screen, n_passes_active;
    int32_t active_size;
    int32_t status;
    int32_t n_delta; // number of (col, delta) entries produced for the residual update
    int32_t _pad;
    int64_t dbg[8];  // cycle counters of the kernel's phases (only filled when built with -DAHIP_CD_PROFILE)
};

template <class T>
struct CdParams {
    int32_t nv, ns;          // screen values / screen groups
    const int32_t* sbegin;   // [ns]
    const int32_t* ssize;    // [ns]
    const T* spen;           // [ns] penalty per screen group
    const T* spen2 = nullptr; // [ns] or nullptr (= spen): factors of the quadratic part (adelie_hip_grpnet_args::penalty_l2, scalars only)
    const T* C;              // centred Gram, screen-value order
    int64_t ldc;
    const T* vars;           // [nv]
    const T* xmean;          // [nv]
    const T* V;              // concatenated (q,q) col-major eigenvector blocks
    const int64_t* voff;     // [ns]
    T* beta;                 // [nv] in/out
    T* g;                    // [nv] in/out: gradient x_a^T W r - xmean_a * resid_sum at the current beta
    int8_t* is_active;       // [ns]
    int32_t* active_set;     // [>= ns]
    T lmda, alpha, tol, newton_tol, dbeta_tol;
    int32_t newton_max_iters, max_active_size, intercept, all_scalar;
    int64_t max_iters;
    CdScalars<T>* sc;        // in: rsq, resid_sum, active_size; out: everything
    // residual-update list produced at exit: delta = beta - beta0 per changed value
    const T* beta0;          // [nv] snapshot of beta at fit entry
    const int32_t* vcol;     // [nv] design column of each screen value
    int32_t* dcols;          // [nv] out
    T* dvals;                // [nv] out
    int32_t max_group_size;
};
template <class T> void launch_cd(const CdParams<T>& p, hipStream_t s);

// ---- block Gauss-Seidel form of a lasso CD pass (kernels_cd_block.hip) ---------------------------
template <class T>
struct CdBlkState { // device-resident scalars carried from block to block and read by the host once per pass
    T rsq, resid_sum, cm;
    int64_t n_updates;
    int32_t active_size, status, nz, _pad;
};
template <class T>
struct CdBlkParams {
    int32_t nv;
    const T* C;
    int64_t ldc;
    const T* vars;
    const T* xmean;
    const T* spen;
    const T* spen2 = nullptr; // factors of the quadratic part, or nullptr (= spen): adelie_hip_grpnet_args::penalty_l2
    T* beta;
    T* g;
    int8_t* is_active;
    int32_t* active_set;
    T l1, l2;
    int32_t max_active_size;
    T* Dbuf;          // 2 * BLK * BLK
    T* dlt;           // BLK
    int32_t* didx;    // BLK
    CdBlkState<T>* st;
    const int32_t* list; // visiting list of the pass (nullptr: screen order 0..count-1)
    int32_t count;
    int32_t mark;
    int32_t bsz;         // visits per block, <= cd_block_size() (the D slot keeps leading dimension cd_block_size())
    // end-of-pass report straight into host-mapped memory (no stream synchronisation on the host side): the solve of block
    // `report_j` copies the state to host_st and then publishes `report_seq` in host_seq (system-scope release)
    CdBlkState<T>* host_st;
    int32_t* host_seq;
    int32_t report_j, report_seq;
    // panel (residual-based) variant, kernels_cd_panel.hip: gradient of the block from the panel step, diagonal block
    // from the cache, changed design columns out for the residual update
    const T* gblk;       // [BLK] gradient of the block's coordinates (list order)
    const T* Dptr;       // BLK x BLK block (ld = BLK)
    const int32_t* vcol; // screen value -> design column
    int32_t* dcol;       // [BLK] out: design columns of the changed coordinates (same order as dlt)
    // look-ahead form of the panel passes (solver.hip::run_panel_passes): gblk was computed from a residual that does not
    // contain the previous block's changes yet; the solve first subtracts Cprev[:, ppos[m]] * pdlt[m], m < *pnz, where
    // Cprev = X_b^T W X_prev - xbar_b xbar_prev^T (BLK x BLK, ld BLK, rows = this block).  Outputs for the next block /
    // the next panel step: block-local positions of the changed coordinates, their count, resid_sum after this block.
    const T* Cprev;
    const T* pdlt;
    const int32_t* ppos;
    const int32_t* pnz;
    int32_t* dpos;
    int32_t* nz_out;
    T* rsum_out;
    // `part` != nullptr: the gradient of the block is not in gblk yet but still in the slice partials of the panel step that
    // ran in the PREVIOUS launch (part[c * part_ld + k], k < part_n): the solve sums them itself in its prologue — in a fixed
    // order — and applies the intercept term  - part_rsum[0] * xbar_c  (what panel_reduce_kernel does as a launch of its own)
    const T* part;
    int64_t part_ld;
    int32_t part_n;
    const T* part_rsum; // nullptr: no intercept term
    // dense form of the changes, for the one-round-trip prologue of the fused look-ahead launch (blk_solve_la_body): every
    // solve of a look-ahead pass leaves  dd[i] = new - old  of its BLK coordinates (0 where nothing changed / beyond the block),
    // the next one reads the previous block's through pdd and forms the correction as Cprev * pdd without index loads
    const T* pdd;
    T* dd;
    // one-coefficient constraints (blk_solve_body<T, true>): bounds per screen value (-inf / +inf where there is none)
    // and, out, the multiplier mu_+ - mu_- of every constrained coordinate the block visited
    const T* clo;
    const T* chi;
    T* cmu;
};
// One visit of a group whose box / one-sided constraint object is solved on the device (kernels_cons.hip): the group is a block
// of its own; pointers are already offset to the group (its screen begin `b`, its first design column `col0`).
template <class T>
struct ConsVisitParams {
    int32_t q, ss, b, col0, native;       // group size, screen position, screen begin, first design column, NATIVE_BOX / _ONE_SIDED
    const T* gsrc;                        // [q] gradient of the group (panel reduce output, or the Gram engines' g + b)
    T* beta;                              // [q] screen_beta + b
    const T* vars;                        // [q] eigenvalues
    const T* V;                           // [q * q] eigenbasis, column-major (ignored for q = 1)
    const T* sxm;                         // [q] screen_X_means + b, or nullptr
    int8_t* is_active;                    // (whole array, indexed by ss)
    int32_t* active_set;
    CdBlkState<T>* st;
    double l1, l2, dbeta_tol;
    int32_t mark, first_of_pass, gram, max_active_size;
    int32_t* dcol; T* dlt;                // [q] out: the changes for the next residual update / Gram update
    const T* va; const T* vb;             // [q] box: lower, upper; one-sided: sgn, b
    T* mu;                                // [q] in/out: the object's multipliers
    double cfg[5];                        // max_iters, tol, pinball / nnqp max_iters, its tol, slack
    CdBlkState<T>* host_st; int32_t* host_seq; int32_t report_seq; // end-of-pass report (report_seq = 0: none)
    int64_t* n_visits;                    // device counter or nullptr
};
size_t cons_visit_lds(int q);
template <class T>
void launch_grp_cons_visit(const ConsVisitParams<T>& p, hipStream_t s);
// abs_grad (and, outside the screen set, the solve_zero multipliers) of the `count` groups in `list` with device constraint objects
template <class T>
void launch_cons_abs_grad(const int32_t* list, int count, const int32_t* native, const int64_t* groups, const int64_t* gsizes,
                          const int32_t* slot, const T* grad, const T* beta, const T* penalty, T regul_scale,
                          const T* va, const T* vb, T* mu, T* abs_grad, hipStream_t s);

// group (q > 1) variant: a block = consecutive groups of the visiting list with <= 128 values in total
template <class T>
struct CdGrpBlkParams {
    int32_t nv;
    const T* C;
    int64_t ldc;
    const T* vars;
    const T* xmean;
    T* beta;
    T* g;
    int8_t* is_active;
    int32_t* active_set;
    T l1, l2, newton_tol, dbeta_tol;
    int32_t newton_max_iters, max_active_size, mark;
    const T* V;
    const int64_t* voff;
    const T* spen;
    const int32_t* sbegin;
    const int32_t* ssize;
    const int32_t* blk_g0; // [nblk+1] first list position of each block
    const int32_t* list;   // visiting list of screen-group indices (nullptr: 0..)
    int32_t nblk;
    T* Dbuf;
    T* dlt;
    int32_t* didx;
    CdBlkState<T>* st;
    // panel (residual-based) variant: see CdBlkParams
    const T* gblk;       // [128] gradient of the block's values (block-local order)
    const T* Dptr;       // 128 x 128 slot, block-local order
    const int32_t* vcol; // screen value -> design column
    int32_t* dcol;       // [128] out: design columns of the changed values
    CdBlkState<T>* host_st;
    int32_t* host_seq;
    int32_t report_j, report_seq;
    int64_t* dbg;        // 8 cycle counters, only written by builds with -DAHIP_GRP_PROFILE
    // look-ahead form, see CdBlkParams (positions are block-local value indices)
    const T* Cprev;
    const T* pdlt;
    const int32_t* ppos;
    const int32_t* pnz;
    int32_t* dpos;
    int32_t* nz_out;
    T* rsum_out;
    // rot: 1 on every panel (residual-based) launch, 0 on the full-Gram engine's.  Panel launches: Dptr holds the block in the
    // eigen-coordinates of its groups, R^T D R with R = blockdiag(V_g) (launch_grp_block_rotate, applied once per build): the sequential loop then works on rotated
    // gradients / coefficients throughout and the per-visit rotations of pin_naive:123-157 happen once per block and value,
    // lane-parallel, in the prologue and the epilogue of the solve
    int32_t rot;
    // panel launches: per-block layout descriptors of the pass (launch_grp_layout, GDESC_* below: the value / group tables that
    // block_layout would otherwise derive through a chain of dependent global loads in every solve's prologue), and the
    // look-ahead correction in dense form: dd (out) / pdd (previous block's, in) = change of every value of the block by
    // block-local position (0 where unchanged or beyond the block), so that the correction is Cprev * pdd with no index loads
    const int32_t* desc;
    const T* pdd;
    T* dd;
    // fused look-ahead launch: the block's gradient is still in the slice partials the previous launch's step left
    // (slice-major, part[k * 128 + c], k < part_n) and the solve sums them itself in the second round trip of its prologue,
    // in a fixed order, then applies the intercept term  - part_rsum[0] * xbar  (as CdBlkParams::part)
    const T* part;
    int32_t part_n;
    const T* part_rsum;
    // fused look-ahead launch: the LAST step workgroup to finish sums the slice partials of the next block (slice-major) in a
    // fixed order, applies  - tail_rsum[0] * tail_xm[col]  and leaves the block's gradient in tail_g — in the shadow of the
    // solve, which outlasts the step in a group launch — instead of a panel_reduce launch between two fused launches.
    // tail_counter: two int32 that are 0 between launches (arrivals; finished tail workgroups: the last of those resets both); nullptr: off.
    int32_t* tail_counter;
    T* tail_g;
    const T* tail_rsum;
    const T* tail_xm; // nullptr: no intercept term
    // one-coefficient constraints of groups of size one (see CdBlkParams): per screen value, +-inf where there is none
    const T* clo;
    const T* chi;
    T* cmu;
    // Fused look-ahead launch: the look-ahead correction of the NEXT block is formed by THIS solve's otherwise idle
    // waves — they fetch the cross block Cnext = C_{j+1,j} while the visiting wave runs, multiply it with this block's dense
    // changes when those exist and leave the 128 sums in corr_out; the next solve then reads corr_in (1 KB) instead of pulling
    // 128 KB of cross block through its own CU at the head of its prologue.  Same products, same order of summation.
    const T* Cnext;   // nullptr: the next solve forms the correction itself from Cprev / pdd
    T* corr_out;
    const T* corr_in; // nullptr: as before
};
// layout descriptor of one block (int32 words)
constexpr int GDESC_VMAP = 0;    // [128] screen-value index of block value i
constexpr int GDESC_VGRP = 128;  // [128] group (of the block) of value i
constexpr int GDESC_VSS = 256;   // [128] screen-group index of value i
constexpr int GDESC_GOFF = 384;  // [129] first value of group k; [ng] = nval
constexpr int GDESC_GQ = 520;    // [128] size of group k
constexpr int GDESC_GSS = 648;   // [128] screen-group index of group k
constexpr int GDESC_NG = 776, GDESC_NVAL = 777;
constexpr int GDESC_VOFF = 784;  // [128] offset of the eigenbasis of value i's group in CdGrpBlkParams::V
constexpr int GDESC_VPOS = 912;  // [128] position of value i inside its group
constexpr int GDESC_VQ = 1040;   // [128] size of value i's group
constexpr int GDESC_STRIDE = 1168;
// descriptors of blocks 0..nblk-1 of the pass described by p (blk_g0, list, sbegin, ssize) into desc
template <class T> void launch_grp_layout(const CdGrpBlkParams<T>& p, int nblk, int32_t* desc, hipStream_t s);
// Dptr <- R^T Dsrc R for one 128 x 128 slot (ld 128; Dsrc == Dptr: in place): `ng` groups, group k = block values [goff[k], goff[k+1]) with eigenbasis
// (q, q) column-major at V + voff[k] (ignored for q == 1).  `scratch` holds 128 * 128 elements, private to the stream.
// Footprint, nval = goff[ng]: all 128 rows of the first nval columns of Dsrc are read.  In place, nothing outside the leading
// nval x nval entries changes.  Dsrc != Dptr: the leading nval x nval entries are written, and when no group is wider than 16 and
// nval is odd also row nval of the first nval columns (the paired store), with Dsrc's entries there; every other entry of Dptr
// keeps what it held.  Entries whose row and column groups both have q == 1 are copied bit for bit.  The result is symmetric
// only up to rounding: the solves read it below the diagonal only.
struct GrpRotArgs {
    int32_t ng;
    int32_t goff[129];
    int64_t voff[128];
};
template <class T> void launch_grp_block_rotate(T* Dptr, const T* Dsrc, const T* V, const GrpRotArgs& a, T* scratch, hipStream_t s);
template <class T> void launch_cd_group_block_pass(const CdGrpBlkParams<T>& p, hipStream_t s);
template <class T> void launch_cd_group_block_range(const CdGrpBlkParams<T>& p, int j0, int j1, hipStream_t s);
template <class T> void launch_cd_group_block_update(const CdGrpBlkParams<T>& p, int j, hipStream_t s);
// the visits of block j against p.gblk / p.Dptr (one workgroup)
template <class T> void launch_cd_group_panel_solve(const CdGrpBlkParams<T>& p, int j, hipStream_t s);
int cd_block_size();
// enqueues one whole pass (gather, then solve/update per block); the host reads st afterwards
template <class T> void launch_cd_block_pass(const CdBlkParams<T>& p, hipStream_t s);
// ---- panel form (kernels_cd_panel.hip): residual-based block passes ------------------------------------------------
// step: r -= sum_{m < *nz_dev} dlt[m] X[:, dcol[m]]; then part[c][slice] = X[slice, cols[c]] . (w*r)[slice] for c < nb.
// Returns the number of row slices.  `part` holds panel_part_elems(n) elements.
template <class T>
int launch_panel_step(const DenseView<T>& X, const T* w, T* r, const int32_t* dcol, const T* dlt, const int32_t* nz_dev,
                      const int32_t* cols, int nb, T* part, hipStream_t s);
// `tail` (2-bit designs, the one-word-per-lane kernel only; *tailed says whether it was used): the step sums its own partials
// -- the last eight workgroups to finish take eight columns each once every workgroup's partials are out -- and leaves the
// block's gradient in tail->g (what panel_reduce would: - rsum[0] * xm[cols[c]] applied): no reduce launch behind the step.
// `counter` counts finished workgroups monotonically over the launches of one solver; `base` = its value before this launch.
template <class T>
struct StepTail {
    int32_t* counter;
    int32_t base;
    T* g;
    const T* rsum;
    const T* xm; // by design column, or nullptr (no intercept term)
};
template <class T>
int launch_panel_step_snp(const SnpView& X, const T* impute, const T* w, T* r, const int32_t* dcol, const T* dlt,
                          const int32_t* nz_dev, const int32_t* cols, int nb, T* part, hipStream_t s,
                          const StepTail<T>* tail = nullptr, bool* tailed = nullptr);
int64_t panel_part_elems(int64_t n);
// Opening of a look-ahead pass whose block-0 gradient already exists: g[c] = grad[cols[c]] (c < nb) out of the full gradient
// the invariance sweep left for the same residual, and both look-ahead residual-sum slots <- rsum_src[0] (nullptr: skip).
template <class T>
void launch_la_open_from_grad(const T* grad, const int32_t* cols, int nb, T* g, const T* rsum_src, T* rsum_out, hipStream_t s);
// gblk[c] = sum_slices part[c][.] - (xm_by_col ? rsum_dev[0] * xm_by_col[cols[c]] : 0)
template <class T>
void launch_panel_reduce(const T* part, int nslices, int nb, const int32_t* cols, const T* rsum_dev, const T* xm_by_col,
                         T* gblk, hipStream_t s);
template <class T>
void launch_panel_reduce_ld(const T* part, int64_t part_ld, int nslices, int nb, const int32_t* cols, const T* rsum_dev,
                            const T* xm_by_col, T* gblk, hipStream_t s);
// fused look-ahead step: the solve of block j (sp, as launch_cd_panel_solve) and a panel step in ONE launch; returns the
// leading dimension of `part` (>= number of row slices; use launch_panel_reduce_ld).  `part` holds 2*panel_part_elems(n).
// `tr`: slice-major partials part[k * 128 + c] (for a solve that sums them itself, CdBlkParams::part with part_ld == 0);
// the return value is then the number of partials per column.
template <class T>
int launch_panel_fused(const CdBlkParams<T>& sp, int j, const DenseView<T>& X, const T* w, T* r, const int32_t* dcol,
                       const T* dlt, const int32_t* nz_dev, const int32_t* cols, int nb, T* part, bool tr, hipStream_t s);
template <class T>
int launch_panel_fused_snp(const CdBlkParams<T>& sp, int j, const SnpView& X, const T* impute, const T* w, T* r,
                           const int32_t* dcol, const T* dlt, const int32_t* nz_dev, const int32_t* cols, int nb, T* part,
                           bool tr, hipStream_t s);
template <class T>
int launch_panel_fused_grp(const CdGrpBlkParams<T>& sp, int j, const DenseView<T>& X, const T* w, T* r, const int32_t* dcol,
                           const T* dlt, const int32_t* nz_dev, const int32_t* cols, int nb, T* part, bool tr, hipStream_t s);
template <class T>
int launch_panel_fused_grp_snp(const CdGrpBlkParams<T>& sp, int j, const SnpView& X, const T* impute, const T* w, T* r,
                               const int32_t* dcol, const T* dlt, const int32_t* nz_dev, const int32_t* cols, int nb,
                               T* part, bool tr, hipStream_t s);
// the visits of block j of the pass (one workgroup); p.gblk / p.Dptr / p.vcol / p.dcol must be set
template <class T> void launch_cd_panel_solve(const CdBlkParams<T>& p, int j, hipStream_t s);
template <class T> void launch_center_vars(T* vars, const T* xm, int cnt, bool center, hipStream_t s);
void launch_gather_i32(const int32_t* src, const int32_t* idx, int cnt, int32_t* out, hipStream_t s);
template <class T>
void launch_cd_compact(const T* beta, const T* beta0, const int32_t* vcol, int nv, int32_t* dcols, T* dvals,
                       int32_t* n_delta, hipStream_t s);

// ---- multi-response view (kernels_multi.hip) -------------------------------------------------------------------------
// The design [1 (x) I_K, X (x) I_K] (first block iff icpt) over a dense base X (nb x pb), never materialised.  Column
// j = u*K + l is (extended feature u, response l); u < icpt is the column of ones, u - icpt the base column otherwise.
// Row vectors (residual, weights) live on the device RESPONSE-MAJOR: element (i, l) at [l*nb + i] (K contiguous vectors of
// length nb), so that every kernel reads a slice of a column of X once and applies it to all K responses with unit-stride
// vector accesses; the C ABI's (n, K) row-major vectors are transposed once on the way in and out.
template <class T>
struct MultiView {
    const T* X;
    int64_t nb, pb, ld;
    const T* ones; // nb ones
    int32_t K, icpt;
    // 2-bit SNP base (matrix_naive_kronecker_eye.ipp over matrix_naive_snp_unphased.ipp): bits != nullptr, X unused — the
    // K-wide kernels decode the calls of a column once for all K responses (accessors.hpp::SnpOnesAcc)
    const uint8_t* bits = nullptr;
    int64_t ldb = 0;
    const T* impute = nullptr;
};
// out[u*K + l] = sum_i xcol(u)[i] * v[l*nb + i]  for every u in [0, pb + icpt): X is read ONCE for all K responses.
template <class T> void launch_multi_sweep(const MultiView<T>& X, const T* v, T* out, T* work, hipStream_t s);
template <class T> int64_t multi_sweep_work_elems(const MultiView<T>& X);
// what launch_multi_sweep runs for this view and this v (multi_shape.hpp); rows per load of the panel steps (the type's vector
// width, or 1 when the base does not take vector loads)
template <class T> MSweepPlan multi_sweep_plan(const MultiView<T>& X, const T* v);
template <class T> int multi_step_vec(const MultiView<T>& X);
// the same over a 2-bit SNP design: out[u*K + l] = x_u . v[l*n + :]; work sized as for the view {nb = n, pb = p, icpt = 0, K}
template <class T>
void launch_multi_sweep_snp(const SnpView& X, const T* impute, int K, const T* v, T* out, T* work, hipStream_t s);
// panel step on view columns (same contract as launch_panel_step; returns the row slices = leading dimension of `part`,
// mstep_slices(nb, multi_step_vec(X)); `part` holds nb_cols times that many elements; at most 128 changes, 256 columns):
//   r -= sum_{m < *nz_dev} dlt[m] X'[:, dcol[m]];   part[c][slice] = X'[slice, cols[c]] . (w*r)[slice]  for c < nb_cols
// entries that share an extended feature (the K responses of a group) are served by one load of the column slice.
template <class T>
int launch_multi_panel_step(const MultiView<T>& X, const T* w, T* r, const int32_t* dcol, const T* dlt,
                            const int32_t* nz_dev, const int32_t* cols, int nb_cols, T* part, hipStream_t s);
// out[:, response] += sign * coef[m] * xcol(feature)  for m < *cnt_dev   (rollback path)
template <class T>
void launch_multi_axpy_cols(const MultiView<T>& X, const int32_t* cols, const T* coef, const int32_t* cnt_dev, T sign,
                            T* out, hipStream_t s);
// symmetric M x M block over extended features ucols (MFMA syrk of kernels_gram.hip with the ones-aware accessor)
template <class T>
void launch_syrk_multi(const MultiView<T>& X, const T* w, const int32_t* ucols, int32_t M, T* C, int64_t ldc, T* work,
                       hipStream_t s);
// D[a + b*ldd] = (resp[a] == resp[b] && (lsel < 0 || resp[a] == lsel)) ? C[slot[a] + slot[b]*ldc] : (lsel <= 0 ? 0 : keep)
// for a, b < nv: expands a Gram block over extended features into the block over view columns (X (x) I_K has no entries
// between different responses).  lsel < 0: one weight vector for all responses; otherwise the call for response lsel.
template <class T>
void launch_multi_expand(const T* C, int64_t ldc, const int32_t* slot, const int32_t* resp, int nv, int lsel, T* D,
                         int64_t ldd, hipStream_t s);
// distinct extended features of a block's view columns (order of first appearance) -> ulist; per column its slot in
// ulist and its response.  nv <= 128.
void launch_multi_block_lists(const int32_t* cols, int nv, int K, int32_t* ulist, int32_t* slot, int32_t* resp,
                              hipStream_t s);
// fused look-ahead launch on the view: group solve of block j + multi-response step (nb_cols <= 128); returns the leading
// dimension of part, mfused_part_ld(nb, multi_step_vec(X))
template <class T>
int launch_multi_panel_fused(const CdGrpBlkParams<T>& sp, int j, const MultiView<T>& X, const T* w, T* r,
                             const int32_t* dcol, const T* dlt, const int32_t* nz_dev, const int32_t* cols, int nb_cols,
                             T* part, hipStream_t s);
template <class T>
void launch_gram_multi(const MultiView<T>& X, const T* w, const int32_t* mcols, int32_t M, const int32_t* ncols, int32_t N,
                       T* C, int64_t ldc, T* work, hipStream_t s);
// C[a + b*ldc] = (resp_r[a] == resp_c[b]) ? G[slot_r[a] + slot_c[b]*ldg] : 0   for a < nr, b < nc
template <class T>
void launch_multi_expand_cross(const T* G, int64_t ldg, const int32_t* slot_r, const int32_t* resp_r, int nr,
                               const int32_t* slot_c, const int32_t* resp_c, int nc, T* C, int64_t ldc, hipStream_t s);
template <class T>
void launch_batch_pick(const T* src, int64_t nfeat, int K, int slot, const T* sub_scale, const T* sub_vec, T* out,
                       hipStream_t s);
// (n, K) row-major <-> response-major
template <class T> void launch_multi_to_major(const T* src, int64_t nb, int K, T* dst, hipStream_t s);
template <class T> void launch_multi_from_major(const T* src, int64_t nb, int K, T* dst, hipStream_t s);

// ---- GLM elementwise (solver_glm_naive.hpp:336-348, 439-449; glm_*.ipp) --------------------------
template <class T>
struct IrlsScalars {
    T hess_sum, y_mean, y_var, resid_sum, conv, loss;
};
// step 1: hess/irls_resid from (eta, resid); partial sums
// (implemented in kernels_glm.hip; declared there to keep this header small)
// the losses of eta = base + b0 + off under two weight vectors (design.hip's path losses; kernels_glm.hip)
template <class T>
void launch_glm_loss2(int kind, const T* y, const T* wa, const T* wb, const T* base, T b0, const T* off, int64_t n, T* sums,
                      hipStream_t s);
template <class T>
void launch_multi_loss2(int kind, const T* y, const T* wa, const T* wb, const T* base, const T* b0, const T* off, int64_t nb,
                        int K, T* sums, hipStream_t s);

// ---- misc -------------------------------------------------------------------------------------
// copy a (rows x cols) block between column-major matrices with different leading dimensions
// covariance-method matrix (kernels_cov.hip)
template <class T>
void launch_cov_gather(const T* S, int64_t lda, int tr, const int32_t* vcol, int32_t nv, int32_t pos0, int32_t N, T* C,
                       int64_t ldc, hipStream_t s);
template <class T>
void launch_cov_bmul(const T* S, int64_t lda, int tr, const int64_t* subset, int64_t ns, const int64_t* indices,
                     const T* values, int64_t ni, T* out, hipStream_t s);
template <class T>
void launch_cov_mul(const T* S, int64_t lda, int64_t p, const int64_t* indices, const T* values, int64_t ni, T* out,
                    hipStream_t s);
template <class T>
void launch_cov_grad(const T* S, int64_t lda, int64_t p, const T* v, const int32_t* cols, const T* coef, const int32_t* cnt,
                     T* grad, hipStream_t s);
// covariance-method matrix kept sparse (kernels_cov_sparse.hip): the column-compressed form of the symmetric (p, p) matrix;
// `lanes` (4, 16 or 64; cov_csc_host.hpp) is the group that walks one column
template <class T>
struct CovCscView {
    const int64_t* cptr;
    const int32_t* cidx;
    const T* cval;
    int64_t p;
    int lanes;
};
// w (p,) = 0, then w[cols[k]] = coef[k] for k < *cnt (read on the device; at most max_cnt, distinct columns)
template <class T>
void launch_cov_csc_fill_w(const int32_t* cols, const T* coef, const int32_t* cnt, int64_t max_cnt, T* w, int64_t p, hipStream_t s);
// out[jj] = (base ? base[j] - dot : dot), dot = sum over the stored entries of column j of cval[e] * w[cidx[e]], j = subset ?
// subset[jj] : jj, for jj < ncols
template <class T>
void launch_cov_csc_coldot(const CovCscView<T>& A, const int64_t* subset, int64_t ncols, const T* w, const T* base, T* out,
                           hipStream_t s);
// launch_cov_gather's cells from the stored entries; `pos` is a (p,) scratch the launcher fills itself
template <class T>
void launch_cov_csc_gather(const CovCscView<T>& A, const int32_t* vcol, int32_t nv, int32_t pos0, int32_t N, T* C, int64_t ldc,
                           int32_t* pos, hipStream_t s);
// out (q, q) column-major on the device = A[i:i+q, i:i+q]
template <class T>
void launch_cov_csc_to_dense(const CovCscView<T>& A, int64_t i, int64_t q, T* out, hipStream_t s);

// Lambda-batched v - A beta_l (adelie_hip_design_cov_mul_batch; cov_batch_host.hpp has the batch width, the chunking and the
// dense plan).  Dense storage: the rows [0, rows) of a chunk in one launch, out (rows, p) with rows contiguous, v null for the
// product alone.  Kept sparse: one batch of rows <= kCovBatchLb per launch; fill_w_batch zeroes the (p, kCovBatchLb) block w and
// writes the batch's rows into it (indptr: the batch's rows + 1 pointers, ebase: the position of the uploaded chunk's first
// entry; max_row: the longest of the batch's rows).
template <class T>
void launch_cov_mul_batch(const T* S, int64_t lda, int64_t p, const int64_t* uptr, const int32_t* ucols, const T* coef, const T* v,
                          int64_t rows, T* out, hipStream_t s);
template <class T>
void launch_cov_csc_fill_w_batch(const int64_t* indptr, const int64_t* indices, const T* values, int64_t ebase, int rows,
                                 int64_t max_row, T* w, int64_t p, hipStream_t s);
template <class T>
void launch_cov_csc_coldot_batch(const CovCscView<T>& A, const T* w, const T* base, int rows, T* out, hipStream_t s);
template <class T> void launch_copy2d(const T* src, int64_t lds, T* dst, int64_t ldd, int64_t rows, int64_t cols, hipStream_t s);
// vars[pos0 + a] = max(C[(pos0+a)*(ldc+1)], 0) for a < cnt   (gs == 1 groups)
// Appending new screen groups to the device mirrors (solver.hip::device_append_screen): ONE packed upload + one scatter
// launch instead of seven to ten small copies per lambda.  Packed image (8-byte aligned throughout):
//   T      pen[Ng], beta[Nv], (lo[Nv], hi[Nv], mu[Nv] when `cons`)
//   int32  begin[Ng], size[Ng], isact[Ng], group[Ng], vcol[Nv]
template <class T>
struct AppendDst {
    T* spen; T* beta; T* clo; T* chi; T* cmu;
    int32_t* sbegin; int32_t* ssize; int8_t* isact; int32_t* slot; int32_t* vcol;
    int32_t ns_old, nv_old, Ng, Nv, cons;
};
template <class T>
struct AppendImage { // offsets (bytes) of the arrays inside the packed image
    size_t pen, beta, lo, hi, mu, begin, size, isact, group, vcol, total;
    __host__ __device__ AppendImage(int Ng, int Nv, bool cons) {
        size_t o = 0;
        pen = o; o += sizeof(T) * size_t(Ng);
        beta = o; o += sizeof(T) * size_t(Nv);
        lo = hi = mu = o;
        if (cons) { lo = o; o += sizeof(T) * size_t(Nv); hi = o; o += sizeof(T) * size_t(Nv); mu = o; o += sizeof(T) * size_t(Nv); }
        o = (o + 7) & ~size_t(7);
        begin = o; o += 4 * size_t(Ng);
        size = o; o += 4 * size_t(Ng);
        isact = o; o += 4 * size_t(Ng);
        group = o; o += 4 * size_t(Ng);
        vcol = o; o += 4 * size_t(Nv);
        total = (o + 7) & ~size_t(7);
    }
};
template <class T> void launch_screen_append(const void* image_dev, const AppendDst<T>& d, hipStream_t s);
// Eigen-decomposition of new screen groups' Gram blocks on the device (kernels_eig.hip): group `i` of the launch reads the
// (q, q) block at src_base + src (leading dimension ld), writes its eigenvalues (ascending, clamped at 0) to
// vars[vars_pos .. + q) and its eigenvectors (column-major, in the columns) to V[v_off .. + q*q).  q == 1: the variance only.
struct EigDesc { int64_t src; int64_t vars_pos; int64_t v_off; int32_t ld; int32_t q; };
constexpr int kEigMaxQ = 96; // 2 * q * q doubles of LDS
template <class T>
void launch_grp_eig(const T* src_base, const EigDesc* desc_dev, int count, int max_q, T* vars, T* V, hipStream_t s);
template <class T> void launch_diag_vars(const T* C, int64_t ldc, int32_t pos0, int32_t cnt, T* vars, hipStream_t s);
// the diagonals of the blocks of a build batch into vars (by screen position; list == nullptr: positions base + off + i)
template <class T>
void launch_block_diag_vars(const T* D0, const SyrkBatch& sb, int ldb, int32_t base, const int32_t* list, T* vars, hipStream_t s);
// transpose row-major (n,p) into column-major with leading dimension ld
template <class T> void launch_transpose(const T* src, int64_t n, int64_t p, T* dst, int64_t ld, hipStream_t s);
// rows / columns of a 2-bit design re-packed as a 2-bit design (dst: pout columns of ldb_dst bytes)
void launch_snp_subset(const SnpView& X, int64_t nout, int64_t pout, const int64_t* rows, const int64_t* cols, uint8_t* dst,
                       int64_t ldb_dst, hipStream_t s);
template <class T> void launch_gather_cols(const T* src, const int64_t* cols, int64_t pout, T* out, hipStream_t s);
// dst (zeroed, column-major, leading dimension ld) += the entries of a CSC matrix
template <class T>
void launch_csc_scatter(const int64_t* indptr, const int32_t* indices, const T* values, int64_t n, int64_t p, T* dst,
                        int64_t ld, hipStream_t s);
// new dense matrix from a resident design: optional row / column gather, optional per-column centre and scale
template <class T>
void launch_derive_dense(const DenseView<T>& X, int64_t nout, int64_t pout, const int64_t* rows, const int64_t* cols,
                         const T* centers, const T* scales, T* dst, int64_t ldd, hipStream_t s);
template <class T>
void launch_derive_dense_snp(const SnpView& X, const T* impute, int64_t nout, int64_t pout, const int64_t* rows,
                             const int64_t* cols, const T* centers, const T* scales, T* dst, int64_t ldd, hipStream_t s);
// pack int8 calldata (n,p col-major) into 2-bit codes
void launch_pack_snp(const int8_t* calldata, int64_t n, int64_t p, uint8_t* bits, int64_t ldb, hipStream_t s);
// PLINK .bed records (p records of stride_in bytes, device memory) -> 2-bit codes; column means of the non-missing calls
void launch_bed_transcode(const uint8_t* bed, int64_t n, int64_t p, int64_t stride_in, uint8_t* bits, int64_t ldb,
                          hipStream_t s);
template <class T> void launch_snp_impute(const uint8_t* bits, int64_t n, int64_t p, int64_t ldb, T* impute, hipStream_t s);

// ---- factor designs (kernels_factor.hip): one-hot / pairwise-interaction expansions of a table Z --------------------------
// A block is the outer product A * B of two small bases over one or two columns of Z, A's columns running fastest
// (matrix_naive_interaction.ipp:78-200, matrix_naive_one_hot.ipp).  The basis of a continuous column is [1, z] (l = 2), of a
// discrete one [z == 0, ..., z == l - 1]; a one-hot block has no B (l1 = 1, B = [1]).  Column t of the block is the
// product's column g = t + shift, k0 = g % l0, k1 = g / l0; `shift` = 1 drops the constant column of two continuous bases
// and of the one-hot block of a continuous column.
constexpr int kFactorChunk = 16; // columns of one block a workgroup of the sweep / the expansion owns
struct FactorBlock {
    int32_t col0, ncols; // first column in the expanded design, number of columns
    int32_t i0, i1;      // columns of Z (i1 = i0 when B is absent)
    int32_t l0, l1;      // sizes of the two bases (continuous: 2; absent B: 1)
    int32_t shift;
    int32_t flags;       // bit 0: A discrete, bit 1: B discrete, bit 2: B absent
};
struct FactorChunk {
    int32_t blk, t0, cnt, pad; // columns [t0, t0 + cnt) of block blk, cnt <= kFactorChunk
};
template <class T>
struct FactorView {
    const T* Z;         // column-major copy of the d columns of Z, leading dimension ldz
    int64_t n, ldz, p;  // rows, leading dimension of Z, columns of the expanded design
    const FactorBlock* blk;
    const FactorChunk* chunk;
    int64_t nchunk;
};
// X (column-major, leading dimension ld, rows >= n untouched) = the expanded design
template <class T> void launch_factor_expand(const FactorView<T>& F, T* X, int64_t ld, hipStream_t s);
// The full sweep out[c] = sum_i X[i, c] v[i] - (sub_vec ? sub_scale[0] * sub_vec[c] : 0) over all p columns, read off Z
// and v alone; fixed summation order (row-slice partials in `work`, factor_sweep_work_elems(n, p, nchunk) elements).
int64_t factor_sweep_work_elems(int64_t n, int64_t p, int64_t nchunk);
template <class T>
void launch_sweep_factor(const FactorView<T>& F, const T* v, T* out, const T* sub_scale, const T* sub_vec, T* work,
                         hipStream_t s);

// ---- convex-relu designs (kernels_relu.hip): gated / signed ReLU expansions of a base matrix Z and a boolean mask ------------
// Column j = sgn (m d) + j_m d + j_d of the (n, P) design holds mask[i, j_m] ? Z[i, j_d] : 0, negated for sgn = 1
// (matrix_naive_convex_relu.ipp:10-30); a gated design has no sgn half (matrix_naive_convex_gated_relu.ipp), P = m d or 2 m d.
template <class T>
struct ReluView {
    const T* Z;          // column-major copy of the d columns of Z, leading dimension ldz, rows n .. ldz - 1 zero
    int64_t n, ldz;
    const uint8_t* mask; // column-major (n, m) bytes, leading dimension ldm, rows n .. ldm - 1 zero
    int64_t ldm, d, m;
    int gated;
    int64_t p() const { return (gated ? 1 : 2) * m * d; }
};
// X (column-major, leading dimension ld, rows >= n untouched) = the expanded design
template <class T> void launch_relu_expand(const ReluView<T>& F, T* X, int64_t ld, hipStream_t s);
// The full sweep out[c] = sum_i X[i, c] v[i] - (sub_vec ? sub_scale[0] * sub_vec[c] : 0) over all P columns as the (d, m) matrix
// product Z^T (mask o v) on the matrix cores, read off Z, the mask and v alone; fixed summation order (row-slice partials in
// `work`, relu_sweep_work_elems(n, d, m) elements, relu_shape.hpp).  Z must be finite: a non-finite value in a masked-out row
// is a zero of the expanded design but poisons the product.
template <class T>
void launch_sweep_relu(const ReluView<T>& F, const T* v, T* out, const T* sub_scale, const T* sub_vec, T* work, hipStream_t s);

// ---- convex-relu designs over a sparse base matrix, kept sparse (kernels_relu_sparse.hip) -----------------------------------------
// The same matrix as above with Z held by compressed columns: column sgn (m d) + j_m d + j_d stores +-Z[i, j_d] at the rows where
// Z stores an entry and mask[i, j_m] is set.  Rows are cut into the tiles of relu_sparse_shape(n, m), gates into words of
// kReluSpWordBits bits; one wavefront owns a (column of Z, tile, word).
template <class T>
struct ReluCscView {
    const int64_t* seg;   // (d, nt + 1): seg[j (nt + 1) + t] = first entry of Z's column j in tile t, [.. + nt] = the column's end
    const int32_t* zidx;  // Z's row indices, rows ascending inside a column
    const T* zval;        // Z's values
    const uint32_t* bits; // the mask packed by row: bit g of bits[w n + i] = mask[i, 32 w + g]; bits beyond m are zero
    int64_t n, d, m;
    int gated;
    int64_t tile_rows;
    int nt;
};
// bits (words * n words, word-major) from the column-major (n, m) mask bytes on the device
void launch_relu_sparse_pack(const uint8_t* mask, int64_t n, int64_t m, uint32_t* bits, hipStream_t s);
// col_cnt[(j_m d + j_d) nt + t] = stored entries of column j_m d + j_d of the unsigned half in tile t (m d nt counts);
// row_cnt[i] = stored entries of row i of the whole design.  zrptr: Z's row pointers.
template <class T>
void launch_relu_sparse_count(const ReluCscView<T>& F, const int64_t* zrptr, int32_t* col_cnt, int64_t* row_cnt, hipStream_t s);
// col_pos (P nt, the exclusive prefix sum of the counts of all P columns in (column, tile) order) and rptr (that of row_cnt)
// place every entry: fills cidx / cval and rcol / rval in canonical form.  Z's row-compressed arrays are read for the rows.
template <class T>
void launch_relu_sparse_fill(const ReluCscView<T>& F, const int64_t* zrptr, const int32_t* zrcol, const T* zrval, const int64_t* col_pos,
                             const int64_t* rptr, int32_t* cidx, T* cval, int32_t* rcol, T* rval, hipStream_t s);
// The full sweep out[c] = sum_i X[i, c] v[i] - (sub_vec ? sub_scale[0] * sub_vec[c] : 0) over all P columns read off Z's nnz(Z)
// entries, the mask words and v; fixed summation order (tile partials in `work`, relu_sparse_sweep_work_elems(n, d, m)
// elements), the signed half the negation of the first.  A masked-out entry is skipped by a select, whatever Z and v hold.
template <class T>
void launch_sweep_relu_sparse(const ReluCscView<T>& F, const T* v, T* out, const T* sub_scale, const T* sub_vec, T* work, hipStream_t s);

// ---- phased-ancestry SNP designs (kernels_phased.hip): the arrays of a CscView built from the (n, 2 s) code table -------------
// `code` is the column-major uint8 table of phased_decode_host.hpp (ancestry of a mutation, or 255); the design has s A columns,
// column j A + a counting the haplotypes of SNP j mutated with ancestry a.  Rows are cut into phased_tiles(n) tiles of
// kPhasedTileRows; the caller keeps s * phased_tiles(n) below 2^31 (one workgroup each).
int phased_tiles(int64_t n);
// col_cnt[(j A + a) nt + t] = stored entries of column j A + a in tile t; row_cnt[i] = stored entries of row i
void launch_phased_count(const uint8_t* code, int64_t n, int64_t s, int A, int32_t* col_cnt, int64_t* row_cnt, hipStream_t st);
// col_pos = the exclusive prefix sum of col_cnt in its own order (so cptr[c] = col_pos[c nt]), rptr that of row_cnt: fills
// cidx / cval and rcol / rval in canonical form (rows ascending in a column, columns ascending in a row, one entry of value 2
// where both haplotypes carry the same ancestry).  Positions come from the counts alone: two calls write identical arrays.
template <class T>
void launch_phased_fill(const uint8_t* code, int64_t n, int64_t s, int A, const int64_t* col_pos, const int64_t* rptr, int32_t* cidx,
                        T* cval, int32_t* rcol, T* rval, hipStream_t st);

} // namespace ahip
