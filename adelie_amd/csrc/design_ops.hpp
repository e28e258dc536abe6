// design_ops.hpp — the raw operations on a resident design (sweep, Gram, axpy, sp_tmul), dispatched over its storage kind in
// one place, and the two reads of a covariance-method matrix (dense or kept sparse) at the end.  Host only: design.hip and
// solver.hip include it, no kernel file does.
// "Raw" is what the stored matrix gives.  A standardized view of a dense / 2-bit design composes its epilogues around these
// calls (solver_screen.hpp: sweep / gram / axpy_cols); one over compressed columns is handled inside the csc kernels, whose
// CscView carries the centers and scales.  The multi-response view has K-wide kernels of its own (the solver calls them) and
// is refused here.  A design made of pieces (kPieces) is the fourth branch of each: a sweep over a column range goes piece by
// piece through the dense / 2-bit launches, everything else through the same kernels over PiecesAcc.  Every work buffer is the caller's: the solver and the matrix operations keep different scratch, and a
// caller may hold live data in one buffer while an operation works in another, so nothing here reserves memory.
#pragma once
#include "common.hpp"

namespace ahip {

inline core_error multi_view_error() {
    return make_core_error("this entry point is not offered on a multi-response view; use the base design.");
}
// A design made of pieces has neither a dense nor a 2-bit view of its own.  Every two-way branch `dense ? ... : ...snp...` of
// the solver and of the design entry points calls this in front of it, so that no launch is ever handed a null view; the
// solver keeps such a design off the panel engines (solver_path.hpp), which is what makes those branches unreachable.
inline void no_pieces(const adelie_hip_design& d, const char* where) {
    if (d.is_pieces())
        throw make_core_error(std::string(where) + " is not offered on a design made of pieces (concatenate(..., resident=\"pieces\")); "
                              "resident=\"auto\" gives one design, on which everything works.");
}
template <class T>
const T* snp_impute(const adelie_hip_design& d) { return static_cast<const T*>(d.impute); }

// ---- sweep: out[k] = x_col(k) . v (kernels.hpp: launch_sweep) -----------------------------------------------------------------
// Whether a sweep takes the structured kernel of a one-hot / interaction design (kernels_factor.hip) or of a convex-relu design
// (kernels_relu.hip; kept sparse: kernels_relu_sparse.hip), which only do the plain full sweep.  `hooks`: the ADELIE_HIP_FACTOR_SWEEP / ADELIE_HIP_RELU_SWEEP values
// the caller goes by (a solve reads them once when it starts, the matrix operations at the call).
inline bool raw_sweep_structured(const adelie_hip_design& d, int64_t c0, int64_t ncols, const int32_t* cols, bool square,
                                 const SweepHooks& hooks) {
    if (cols || c0 != 0 || ncols != d.p || square) return false;
    // a convex-relu design kept sparse (kernels_relu_sparse.hip); a standardized view of one sweeps its compressed columns
    if (d.is_csc()) return d.relu_csc() && !d.std_center && relu_sparse_sweep_on(hooks.relu);
    if (!d.is_dense() || d.is_std_view()) return false;
    return (d.factor() && factor_sweep_on(hooks.factor)) || (d.relu() && relu_sweep_on(hooks.relu));
}
// (c0: the first column of a sweep over a column range; only a design made of pieces sizes its work by where the range lies)
inline int64_t raw_sweep_work_elems(const adelie_hip_design& d, int64_t ncols, bool structured, int64_t c0 = 0) {
    if (d.is_pieces())
        return d.dtype == ADELIE_HIP_F64 ? sweep_work_elems_pieces<double>(d.pieces<double>(), c0, ncols)
                                         : sweep_work_elems_pieces<float>(d.pieces<float>(), c0, ncols);
    if (structured && d.relu_csc()) return relu_sparse_sweep_work_elems(d.n, d.r_d, d.r_m);
    if (structured && d.relu()) return relu_sweep_work_elems(d.n, d.r_d, d.r_m);
    if (structured) return factor_sweep_work_elems(d.n, d.p, d.f_nchunk);
    return d.is_csc() ? sweep_work_elems_csc(d.sp_parts(), ncols) : sweep_work_elems(d.n, ncols);
}
template <class T>
void raw_sweep(const adelie_hip_design& d, const T* v, T* out, int64_t c0, int64_t ncols, const int32_t* cols, const T* sub_scale,
               const T* sub_vec, bool square, bool structured, T* work, hipStream_t s) {
    if (structured && d.relu_csc()) launch_sweep_relu_sparse<T>(d.relu_csc_view<T>(), v, out, sub_scale, sub_vec, work, s);
    else if (structured && d.relu()) launch_sweep_relu<T>(d.relu_view<T>(), v, out, sub_scale, sub_vec, work, s);
    else if (structured) launch_sweep_factor<T>(d.factor_view<T>(), v, out, sub_scale, sub_vec, work, s);
    else if (d.is_dense()) launch_sweep<T>(d.dense<T>(), v, out, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
    else if (d.is_snp()) launch_sweep_snp<T>(d.snp(), snp_impute<T>(d), v, out, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
    else if (d.is_csc()) launch_sweep_csc<T>(d.csc<T>(), v, out, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
    else if (d.is_pieces()) launch_sweep_pieces<T>(d.pieces<T>(), v, out, c0, ncols, cols, sub_scale, sub_vec, square, work, s);
    else throw multi_view_error();
}

// ---- Gram: C[m_pos0 + a, n_pos0 + b] = x_mcols[a]^T W x_ncols[b] (kernels.hpp: launch_gram) -----------------------------------
inline int64_t raw_gram_work_elems(const adelie_hip_design& d, int64_t n, int64_t M, int64_t N) {
    return d.is_csc() ? gram_work_elems_csc(n, M, N, d.sp_parts()) : gram_work_elems(n, M, N);
}
template <class T>
void raw_gram(const adelie_hip_design& d, const T* w, const int32_t* mcols, int32_t M, int32_t m_pos0, const int32_t* ncols, int32_t N,
              int32_t n_pos0, const T* xm, bool center, T* C, int64_t ldc, T* work, hipStream_t s) {
    if (d.is_dense()) launch_gram<T>(d.dense<T>(), w, mcols, M, m_pos0, ncols, N, n_pos0, xm, center, C, ldc, work, s);
    else if (d.is_snp()) launch_gram_snp<T>(d.snp(), snp_impute<T>(d), w, mcols, M, m_pos0, ncols, N, n_pos0, xm, center, C, ldc, work, s);
    else if (d.is_csc()) launch_gram_csc<T>(d.csc<T>(), w, mcols, M, m_pos0, ncols, N, n_pos0, xm, center, C, ldc, work, s);
    else if (d.is_pieces()) launch_gram_pieces<T>(d.pieces<T>(), w, mcols, M, m_pos0, ncols, N, n_pos0, xm, center, C, ldc, work, s);
    else throw multi_view_error();
}

// ---- axpy: out += sign * sum_k coef[k] x_cols[k] (kernels.hpp: launch_axpy_cols) ----------------------------------------------
// `delta_zeroed` is only read on compressed columns and may be null otherwise.  There it is the caller's p + 8 elements, all
// zero on entry; the kernels scatter the coefficients into it and leave it all zero again, so a caller zeroes it once.
template <class T>
void raw_axpy_cols(const adelie_hip_design& d, const int32_t* cols, const T* coef, const int32_t* count_dev, int32_t count, T sign,
                   T* out, T* delta_zeroed, hipStream_t s) {
    if (d.is_dense()) launch_axpy_cols<T>(d.dense<T>(), cols, coef, count_dev, count, sign, out, s);
    else if (d.is_snp()) launch_axpy_cols_snp<T>(d.snp(), snp_impute<T>(d), cols, coef, count_dev, count, sign, out, s);
    else if (d.is_csc()) launch_axpy_cols_csc<T>(d.csc<T>(), cols, coef, count_dev, count, sign, out, delta_zeroed, s);
    else if (d.is_pieces()) launch_axpy_cols_pieces<T>(d.pieces<T>(), cols, coef, count_dev, count, sign, out, s);
    else throw multi_view_error();
}

// ---- sp_tmul: out (L, n) row-major = V X^T for a CSR V of L rows (kernels.hpp: launch_sp_tmul) --------------------------------
inline int64_t raw_sp_tmul_work_elems(const adelie_hip_design& d) { return d.is_csc() ? sp_tmul_work_elems_csc(d.p) : 0; }
template <class T>
void raw_sp_tmul(const adelie_hip_design& d, int64_t L, const int64_t* indptr, const int64_t* indices, const T* values, T* out,
                 T* work, hipStream_t s) {
    if (d.is_dense()) launch_sp_tmul<T>(d.dense<T>(), L, indptr, indices, values, out, s);
    else if (d.is_snp()) launch_sp_tmul_snp<T>(d.snp(), snp_impute<T>(d), L, indptr, indices, values, out, s);
    else if (d.is_csc()) launch_sp_tmul_csc<T>(d.csc<T>(), L, indptr, indices, values, out, work, s);
    else if (d.is_pieces()) launch_sp_tmul_pieces<T>(d.pieces<T>(), L, indptr, indices, values, out, s);
    else throw multi_view_error();
}

// ---- covariance method: the two places the path solver touches A, over its storage (kernels_cov.hip, kernels_cov_sparse.hip) ----
// C[a, pos0 + b] = A(vcol[a], vcol[pos0 + b]) for a < nv, b < N, mirrored for the old values.  `pos` is the caller's (p,) int32
// scratch, read on a matrix kept sparse only.
template <class T>
void raw_cov_gather(const adelie_hip_design& d, const int32_t* vcol, int32_t nv, int32_t pos0, int32_t N, T* C, int64_t ldc,
                    int32_t* pos, hipStream_t s) {
    if (d.cov_csc()) launch_cov_csc_gather<T>(d.cov_csc_view<T>(), vcol, nv, pos0, N, C, ldc, pos, s);
    else launch_cov_gather<T>(static_cast<const T*>(d.X), d.ld, d.cov == 2, vcol, nv, pos0, N, C, ldc, s);
}
// grad = v - sum_k coef[k] A[:, cols[k]] for k < *cnt (on the device; at most max_cnt).  `w` is the caller's (p,) scratch, read
// on a matrix kept sparse only.
template <class T>
void raw_cov_grad(const adelie_hip_design& d, const T* v, const int32_t* cols, const T* coef, const int32_t* cnt, int64_t max_cnt,
                  T* grad, T* w, hipStream_t s) {
    if (d.cov_csc()) {
        launch_cov_csc_fill_w<T>(cols, coef, cnt, max_cnt, w, d.p, s);
        launch_cov_csc_coldot<T>(d.cov_csc_view<T>(), nullptr, d.p, w, v, grad, s);
    } else {
        launch_cov_grad<T>(static_cast<const T*>(d.X), d.ld, d.p, v, cols, coef, cnt, grad, s);
    }
}

} // namespace ahip
