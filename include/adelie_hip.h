/*
 * adelie_hip.h — C ABI of libadelie_hip.so: the MI355X-native replacement for the
 * grpnet hot path of JamesYang007/adelie.
 *
 * The reference has no C ABI: its boundary is the pybind11 module `adelie.adelie_core`
 * (reference adelie/src/py_adelie_core.cpp:6-44).  Every entry point below names the
 * pybind class / method it stands in for (file:line relative to /root/reference).
 * Plain pointers and sizes only; no torch / Eigen / numpy types cross this boundary.
 *
 * Conventions
 *   - dtype: ADELIE_HIP_F32 / ADELIE_HIP_F64 is a property of the design matrix; every
 *     `const void*` / `void*` value array is in that dtype (value_t of the reference).
 *     Scalars cross as double.  Indices are int64 (Eigen::Index, state_base.hpp:33).
 *   - All array arguments are HOST pointers unless the name ends in `_dev`.
 *   - Return value 0 = ok; nonzero = construction / argument error, message via
 *     adelie_hip_last_error() (the reference throws adelie_core_error -> RuntimeError,
 *     state_base.ipp:15-92).  Errors raised INSIDE a solve do not fail the call: they are
 *     recorded in the result's error string and the partial path is returned, exactly as
 *     py_state.cpp:62-91 (`_solve`) does.
 */
#ifndef ADELIE_HIP_H
#define ADELIE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADELIE_HIP_ABI_VERSION 14

enum adelie_hip_dtype { ADELIE_HIP_F32 = 0, ADELIE_HIP_F64 = 1 };
enum adelie_hip_order { ADELIE_HIP_COL_MAJOR = 0, ADELIE_HIP_ROW_MAJOR = 1 };
enum adelie_hip_screen_rule { ADELIE_HIP_SCREEN_STRONG = 0, ADELIE_HIP_SCREEN_PIVOT = 1 };
/* glm_kind: which GlmBase implementation runs on device (glm_gaussian.ipp, glm_binomial.ipp) */
enum adelie_hip_glm_kind {
    ADELIE_HIP_GLM_GAUSSIAN = 0,        /* glm.gaussian(opt=True): StateGaussianNaive, no IRLS (solver.py:683-686) */
    ADELIE_HIP_GLM_BINOMIAL_LOGIT = 1,  /* glm.binomial(link="logit"): StateGlmNaive + IRLS */
    ADELIE_HIP_GLM_GAUSSIAN_IRLS = 2,   /* glm.gaussian(opt=False): Gaussian loss forced through StateGlmNaive */
    ADELIE_HIP_GLM_POISSON = 4,         /* glm.poisson (glm_poisson.ipp:14-58): StateGlmNaive + IRLS */
    ADELIE_HIP_GLM_BINOMIAL_PROBIT = 5, /* glm.binomial(link="probit") (glm_binomial.ipp:100-190) */
    ADELIE_HIP_GLM_CALLBACK = 6,        /* a GlmBase subclass written by the user (Python trampoline PyGlmBase, py_glm.cpp:8-92):
                                           StateGlmNaive + IRLS with gradient / hessian / loss evaluated by the host
                                           callbacks of adelie_hip_glm_callbacks on n-vectors, once per IRLS iteration */
    ADELIE_HIP_GLM_COX = 7,             /* glm.cox (glm_cox.ipp): StateGlmNaive + IRLS, the family evaluated on the device from the
                                           adelie_hip_glm_cox handle in adelie_hip_grpnet_args::glm_cox (ABI 11) */
    ADELIE_HIP_GLM_MULTINOMIAL = 3      /* glm.multinomial: StateMultiGlmNaive (solver_multiglm_naive.hpp) + IRLS; the design must
                                           be a multi-response view (adelie_hip_design_create_multi).  glm_y is (n, K) row-major,
                                           glm_weights is (n,), offsets / eta / resid are (n, K) row-major (glm_multinomial.ipp) */
};

/* Opaque handles. */
typedef struct adelie_hip_design adelie_hip_design; /* device-resident MatrixNaiveBase object */
typedef struct adelie_hip_result adelie_hip_result; /* solved state snapshot (the `state` copy _solve returns) */
typedef struct adelie_hip_glm_cox adelie_hip_glm_cox; /* ABI 11: a Cox family's sort orders and weights, resident on one device */
typedef struct adelie_hip_css_result adelie_hip_css_result; /* ABI 13: a solved column-subset-selection state */
typedef struct adelie_hip_bvls_result adelie_hip_bvls_result; /* ABI 14: a solved bounded-variable least squares state */
typedef struct adelie_hip_pinball_result adelie_hip_pinball_result; /* a solved pinball least squares state (an addition to ABI 14) */

/* ------------------------------------------------------------------------------------------
 * Library
 * ------------------------------------------------------------------------------------------ */
int         adelie_hip_abi_version(void);
/* Thread-local message of the last failing call on this thread. */
const char* adelie_hip_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unavailable). */
int         adelie_hip_device_count(void);
/* Mirrors adelie.configs.set_configs (py_configs.cpp:6-49): names "hessian_min", "dbeta_tol".
 * One name has no counterpart upstream: "sweep_batch" (0/1, default 0).  When 1, solves that run concurrently (from
 * different host threads) on one dense matrix -- a design and its aliases, e.g. the folds of cv_grpnet -- share their
 * full-gradient sweeps: those that reach a sweep within a short window are answered by one pass over X.  The gradients are
 * then accumulated in another (fixed) order than the ordinary sweep's, i.e. they differ from it in the last bits.
 * Device memory: the working buffers of a finished solve are parked in a process-wide cache and handed to the next solve
 * instead of going through hipFree / hipMalloc; "pool_limit_mb" (default 6144; 0 = no caching) bounds what stays parked,
 * "pool_trim" (any value) returns the parked blocks to the driver.
 * adelie_hip_bvls_solve (ABI 14): "bvls_gram_limit_mb" (default 16384) bounds the screen Gram matrix of a solve;
 * "bvls_lds_max_ns" (default 0 = as many as the device's LDS holds) keeps the fit kernel's per-coordinate state in global
 * memory for screen sets larger than the value (test hook: both forms give the same bits).
 * adelie_hip_qp_full_solve: "qp_full_lds_max_d" (default 0 = as many as the device's LDS holds) keeps the per-coordinate state of
 * a problem with d > 64 in global memory from that d on (test hook: both forms give the same bits).
 * adelie_hip_gaussian_pin_solve: "pin_path_launch" (0/1, default 1): a pin path on a screen set that the single-workgroup
 * descent takes runs in one launch (1) or in one launch per lambda (0); both give the same bits.  Read when a solve starts. */
int         adelie_hip_set_config(const char* name, double value);

/* ------------------------------------------------------------------------------------------
 * Design matrix  == adelie.matrix.dense / MatrixNaiveDense{32,64}{C,F}
 *                   (matrix.py:549-680, matrix_naive_dense.ipp:9-21)
 * The reference holds a non-owning Eigen::Map of the caller's ndarray; here the matrix is
 * copied once into HBM (or adopted in place when it already lives there) and stays resident.
 * ------------------------------------------------------------------------------------------ */
/* Copy an (n,p) host matrix to device `device`. */
int adelie_hip_design_create_dense(const void* host, int64_t n, int64_t p, int dtype, int order,
                                   int device, adelie_hip_design** out);
/* Replaces MatrixNaiveSparse{32,64}F (adelie/matrix.py:1301-1385, matrix_naive_sparse.ipp): a CSC matrix (indptr p+1
 * int64, row indices int32, values of `dtype`; host pointers) becomes a resident dense design -- the entries are
 * scattered into zeroed column-major HBM once, every later operation is the dense kernel.  Duplicate entries add up. */
int adelie_hip_design_create_sparse(const int64_t* indptr, const int32_t* indices, const void* values, int64_t n, int64_t p,
                                    int dtype, int device, adelie_hip_design** out);
/* Replaces MatrixNaiveSparse{32,64}F with the matrix KEPT SPARSE in HBM (matrix_naive_sparse.ipp walks the CSC arrays per
 * operation, and so does this design): the stored entries are uploaded column-compressed (indptr p+1 int64, row indices int32
 * ascending and distinct inside a column, values of `dtype`) and row-compressed (row_indptr n+1, column indices, values: the
 * same entries, e.g. scipy's .tocsr()).  12 bytes per stored entry each way instead of n*p values (plus, for designs of more
 * than one tile of 16384 rows and at least a few entries per tile and column, a tile-major copy of 10 bytes per entry that
 * the library builds on the device for its full sweeps): a design whose dense form does not fit can run.  Gradients and Gram rows stream the CSC copy (one wavefront per column), residual updates and X beta
 * the CSR copy; grpnet_solve runs its full-Gram engines on Gaussian fits (the Gram is built once) and, under IRLS, the panel
 * engine over compressed columns, which also serves constrained fits (Gaussian fits with constraints are refused: the caller
 * expands the design).  REPRODUCIBILITY: the IRLS panel form applies the residual update of a block with hardware f64 atomics
 * over the stored entries (csc_panel_update_kernel); where two changed columns of a block share a row the order of the two
 * additions is not fixed, so two runs of a GLM path on a design kept sparse agree to rounding (1e-15 relative), not bit for bit
 * -- every other engine of this library is order-deterministic.  All MatrixNaiveBase operations below accept it; derived designs
 * are composed on the host. */
int adelie_hip_design_create_csc(const int64_t* indptr, const int32_t* indices, const void* values, const int64_t* row_indptr,
                                 const int32_t* row_indices, const void* row_values, int64_t n, int64_t p, int dtype, int device,
                                 adelie_hip_design** out);
/* Additive entry points (the ABI version stays 14; callers look the symbols up).  Replace MatrixNaiveSNPPhasedAncestry{32,64}
 * (adelie/matrix.py:1189-1242, matrix_naive_snp_phased_ancestry.ipp) over an adelie.io.snp_phased_ancestry image
 * (io_snp_phased_ancestry.ipp:10-42,143-347): n samples, s SNPs, A < 256 ancestries, the (n, s A) matrix whose column j A + a
 * counts the two haplotypes of SNP j that are mutated with ancestry a (entries 0, 1, 2; at most two stored per sample and
 * SNP).  The result is a design kept sparse, exactly what adelie_hip_design_create_csc gives for the same matrix in canonical
 * form, with everything said there (engines, reproducibility of GLM paths to rounding, constrained Gaussian fits refused).  The
 * host decodes `snpdat` -- every offset, chunk header and row is checked against the image before it is used; a damaged image
 * is an error and creates nothing -- into one byte per haplotype call (the ancestry, or 255); those 2 n s bytes are uploaded
 * and the device builds the compressed arrays from counts and prefix sums (kernels_phased.hip; two builds give identical
 * arrays), then frees the bytes.  No (n, s A) array is formed on either side. */
int adelie_hip_design_create_snp_phased_ancestry(const void* snpdat, int64_t n_bytes, int dtype, int device, adelie_hip_design** out);
/* Same, from the int8 (n, 2 s) column-major `calldata` (0 / 1) and `ancestries` (in [0, A), also where the call is 0, where the
 * value is otherwise ignored) that adelie.io.snp_phased_ancestry.write takes (column 2 j + k = haplotype k of SNP j), with the
 * writer's errors for a non-binary call, an ancestry out of range and A >= 256, without the file. */
int adelie_hip_design_create_snp_phased_calldata(const int8_t* calldata, const int8_t* ancestries, int64_t n, int64_t s, int64_t A,
                                                 int dtype, int device, adelie_hip_design** out);
/* The arrays of a design kept sparse copied back to the host: the column-compressed form (indptr of cols + 1, indices and
 * values of nnz entries, values in the design's dtype) and the row-compressed form likewise (rows + 1).  A NULL pointer skips
 * that array.  On a standardized view these are the entries of the matrix underneath.  A covariance matrix kept sparse
 * (adelie_hip_design_create_cov_csc) has the column form only: asking for a row array is an error.  adelie_hip_design_nnz gives
 * the number of stored entries, -1 for a design that is not kept sparse. */
int adelie_hip_design_csc_download(adelie_hip_design* d, int64_t* indptr, int32_t* indices, void* values, int64_t* row_indptr,
                                   int32_t* row_indices, void* row_values);
int64_t adelie_hip_design_nnz(const adelie_hip_design* d);
/* Replaces MatrixNaiveStandardize (adelie/matrix.py:1414-1533, matrix_naive_standardize.ipp), the lazy wrapper: the view
 * (x_ij - centers[j]) / scales[j]  of `src` (dense, 2-bit SNP or kept sparse) with the resident matrix untouched and shared.
 * Over a design kept sparse every operation below applies the centring / scaling as a rank-one correction in its epilogue
 * (kernels_sparse.hip: centring would fill every cell).  Over a dense or 2-bit design the handle serves grpnet_solve only,
 * which composes the base design's kernels with those corrections and runs its full-Gram engines (a standardized 2-bit design
 * stays 2 bits per call instead of 8 bytes); its matrix operations are composed by the caller from the base design's
 * (adelie_amd.matrix does).  `src` must outlive the view; constraints and the multi-response view are not offered on it. */
int adelie_hip_design_create_standardized(adelie_hip_design* src, const double* centers, const double* scales,
                                          adelie_hip_design** out);
/* Adopt an (n,p) matrix that is ALREADY in device memory (e.g. a torch tensor's data_ptr);
 * not owned, must outlive the design. */
int adelie_hip_design_adopt_dense_dev(const void* dev_ptr, int64_t n, int64_t p, int dtype, int order,
                                      int device, adelie_hip_design** out);
/* == adelie.matrix.snp_unphased over an adelie.io.snp_unphased file image
 * (matrix.py:1245-1298, io_snp_unphased.ipp:10-41): `snpdat` is the whole .snpdat byte image;
 * it is decoded once into a dense 2-bit-per-call column-major device layout. */
int adelie_hip_design_create_snp_unphased(const void* snpdat, int64_t n_bytes, int dtype,
                                          int device, adelie_hip_design** out);
/* Same, from an int8 calldata matrix (n,p) column-major (values 0/1/2, negative = missing)
 * and per-column impute values (io_snp_unphased.ipp:70-303 semantics, without the file). */
int adelie_hip_design_create_snp_calldata(const int8_t* calldata, int64_t n, int64_t p,
                                          const double* impute, int dtype, int device,
                                          adelie_hip_design** out);
/* Same device layout straight from a PLINK 1 `.bed` image (SNP-major: magic 6c 1b 01, then p records of ceil(n/4)
 * bytes, 2 bits per sample, low bits first: 00 = two copies of allele A1, 10 = one, 11 = none, 01 = missing).  Calls become
 * A1 counts; missing calls are imputed with the column mean of the non-missing ones (the reference's default,
 * io/utils.hpp:10-31).  `bed` is host memory (the header is validated on the host).  SURVEY.md 8(f) rank 2: the on-disk format upstream of
 * adelie.io.snp_unphased in a genotype pipeline; both are 2 bits per call, so the record is transcoded on the device. */
int adelie_hip_design_create_snp_bed(const void* bed, int64_t n_bytes, int64_t n, int64_t p, int dtype, int device,
                                     adelie_hip_design** out);
/* A second handle on the same resident matrix with its own HIP stream and scratch space, so that independent solves
 * (the folds of cv_grpnet) can run concurrently from different host threads: one path leaves most of the chip idle
 * while its sequential block solves run, two or three paths interleave.  The alias must be destroyed before `src`. */
int adelie_hip_design_alias(adelie_hip_design* src, adelie_hip_design** out);
/* A rectangular slice  base[r0 : r0 + nr, c0 : c0 + nc]  as a design that SHARES the resident matrix (nothing is copied; own
 * stream and scratch; must be destroyed before `base`): what adelie.matrix.subset gives for a contiguous index range
 * (matrix_naive_subset.ipp wraps lazily as well; matrix.py:1538-1640).  Dense designs: any column range, row ranges that start on
 * a 16-byte boundary (r0 a multiple of 2 in f64, of 4 in f32); 2-bit SNP designs: column ranges over all rows.  Other designs
 * (sparse, views, covariance matrices) and other ranges are refused: the caller copies (adelie_hip_design_create_derived). */
int adelie_hip_design_create_slice(adelie_hip_design* base, int64_t r0, int64_t nr, int64_t c0, int64_t nc,
                                   adelie_hip_design** out);
/* Shared full-gradient sweeps of concurrent solves on this design and its aliases ("sweep_batch" config above), cumulative
 * since the design was created: out[0] = launches of the K-wide sweep kernel, out[1] = vectors they answered (= the ordinary
 * sweeps saved + launches), out[2] = their HIP-event time in ms on the batcher's stream.  Used by bench.py for the roofline of
 * cv_grpnet's dominant kernel (one launch streams the design once: n*p*sizeof(value) algorithmic bytes). */
int adelie_hip_design_batch_stats(adelie_hip_design* d, double* out);
/* A new design derived from a resident one (dense or SNP; a subset of an SNP design without centring / scaling is again a
 * 2-bit design, the selected calls re-packed four per byte; everything else is dense): rows `rows[0..n_rows)` (NULL: all), columns
 * `cols[0..n_cols)` (NULL: all), every resulting column j centred by centers[j] and divided by scales[j] (NULL: no centring /
 * scaling).  This is what adelie.matrix.subset (matrix_naive_subset.ipp) and adelie.matrix.standardize
 * (matrix_naive_standardize.ipp: X = (Z - 1 c^T) diag(s)^-1) describe; the reference wraps the parent lazily, here the result is
 * materialised in HBM by one kernel (matrix views).  The result does not reference `src`. */
int adelie_hip_design_create_derived(adelie_hip_design* src, const int64_t* rows, int64_t n_rows, const int64_t* cols,
                                     int64_t n_cols, const double* centers, const double* scales, adelie_hip_design** out);
/* Replaces MatrixNaiveCConcatenate / MatrixNaiveRConcatenate (adelie/matrix.py:214-310, matrix_naive_concatenate.ipp):
 * the k resident designs are copied side by side (axis 1: columns; axis 0: rows) into one new dense design; SNP sources
 * are decoded, except that 2-bit designs side by side (axis 1, all of them SNP) give a 2-bit design.  The sources stay valid and
 * independent.  The reference's error strings for mismatched shapes are kept. */
int adelie_hip_design_create_concat(adelie_hip_design* const* srcs, int64_t k, int axis, adelie_hip_design** out);
/* Column blocks kept as they are (adelie_amd.matrix.concatenate(..., axis=1, resident="pieces"); the reference's
 * matrix_naive_concatenate.ipp keeps its pieces too): the (n, sum of p_m) design whose columns are those of the k <= 8 sources side
 * by side, without a copy.  Every source is a plain dense design or a plain 2-bit SNP design (a column slice and the expanded
 * one-hot / interaction / convex-relu designs count as the dense designs they are); all share rows, dtype and device.  Anything
 * else -- a design kept sparse, a standardized or multi-response view, a covariance or constraint matrix, another pieces design,
 * more than 8 sources -- is refused before anything is allocated, with a message that names the piece and its kind.  The new
 * handle BORROWS the sources' device arrays and owns none: the sources must outlive it and every alias of it
 * (adelie_hip_design_owned_bytes does not move).
 * Offered on it: the matrix operations (cmul, ctmul, bmul, btmul, mul, mul_batch, cov, sq_mul, sp_tmul, glm_path_losses),
 * adelie_hip_design_alias, adelie_hip_bench_sweep, and adelie_hip_grpnet_solve for the Gaussian and the single-response GLM
 * families without constraints, always on the full-Gram engines (ADELIE_HIP_INFO_ENGINE_PANEL of such a solve is 0).  A sweep
 * over a column range runs piece by piece with the kernels of the pieces' own storage, so a column's value is what its piece
 * alone gives.  Refused on it with an error: create_multi, create_standardized, create_derived, create_slice, a further
 * create_concat / create_pieces, create_cov_lazy, impute, bvls / pinball solves, constraints, adelie_hip_block_build_test.
 * The entry is additive and changes the layout of no existing structure: ADELIE_HIP_ABI_VERSION stays as it is. */
int adelie_hip_design_create_pieces(adelie_hip_design* const* srcs, int64_t k, adelie_hip_design** out);
/* Multi-response view of a resident dense or 2-bit SNP design: the (n*K) x ((p + intercept)*K) matrix
 *     [ 1_n (x) I_K ,  X (x) I_K ]      (the first block only when `intercept` != 0)
 * that adelie/state.py:1100-1125 (_render_multi_inputs) builds from matrix.kronecker_eye / matrix.concatenate
 * (matrix_naive_kronecker_eye.ipp:27-47, matrix_naive_concatenate.ipp) and hands to StateMultiGaussianNaive.  Column j is
 * (extended feature j / K, response j % K); vectors over the rows are (n, K) row-major, as in the reference.  Nothing is
 * materialised: the view shares `base`'s matrix (which must outlive it) and owns a stream, scratch space and one column of
 * ones.  adelie_hip_grpnet_solve on the view runs the Gaussian naive solver with every kernel reading a column of X once
 * for all K responses (a 2-bit base stays 2-bit: its calls are decoded once per column for all K).  The matrix-op entry
 * points (cmul ... sp_tmul) are not offered on the view: the Python layer reaches them through `base`. */
int adelie_hip_design_create_multi(adelie_hip_design* base, int64_t K, int intercept, adelie_hip_design** out);
/* ABI 12.  Replaces MatrixNaiveOneHotDense{32,64}{C,F} (adelie/matrix.py:1073-1186, matrix_naive_one_hot.ipp): the design
 * whose blocks, in the order of the d columns of Z, are [Z_j] for a continuous column (levels[j] <= 0) and
 * [Z_j == 0, ..., Z_j == L - 1] for a discrete one (levels[j] = L > 0).  A value outside {0..L-1} gives a zero row in its
 * block, as the reference's `==` does.  `Z` is a resident dense naive design (SNP, sparse, view and covariance handles are
 * refused); `levels` has Z's column count.  The result is an ordinary dense column-major design, filled on the device from the
 * resident Z by one kernel (the reference generates the columns inside every operation; here n * P values live in HBM and
 * every kernel of the library runs on them), plus what the structured full sweep needs: an owned copy of Z's d columns and a
 * per-block descriptor table (first column, the two columns of Z, the two basis sizes, the case).  It does not reference `Z`.
 * adelie_hip_design_alias hands the copy and the table on (not owned); slices, derived designs, concatenations and
 * multi-response views of the result are plain dense designs. */
int adelie_hip_design_create_one_hot(adelie_hip_design* Z, const int64_t* levels, adelie_hip_design** out);
/* ABI 12.  Replaces MatrixNaiveInteractionDense{32,64}{C,F} (adelie/matrix.py:721-914, matrix_naive_interaction.ipp): for every
 * row (i, j) of `pairs` ((n_pairs, 2) row-major, i != j, the valid and unique pairs that matrix.py:876-904 builds from intr_map)
 * the block A * B with A's columns running fastest, A / B = [1, Z_.] for a continuous column and [Z_. == 0, ...] for a
 * discrete one, without the constant column when both are continuous ([Z_i, Z_j, Z_i Z_j]): l0 * l1 - both_cont columns with
 * continuous counted as 2 (init_outer, matrix_naive_interaction.ipp:10-26).  Entries are 0, 1, a value of Z or one product of
 * two values of Z in the design's dtype.  Same kind of result and the same handle rules as adelie_hip_design_create_one_hot. */
int adelie_hip_design_create_interaction(adelie_hip_design* Z, const int64_t* pairs, int64_t n_pairs, const int64_t* levels,
                                         adelie_hip_design** out);
/* Additive entry point (the ABI version stays 14; callers look the symbol up).  Replaces MatrixNaiveConvexGatedReluDense and
 * MatrixNaiveConvexReluDense {32,64}{C,F} and their Sparse forms (adelie/matrix.py:390-560, matrix_naive_convex_gated_relu.ipp,
 * matrix_naive_convex_relu.ipp): from the (n, d) design Z and the (n, m) boolean mask the design [D_1 Z, ..., D_m Z] of m d
 * columns (gated != 0) or [Y, -Y] of 2 m d columns (gated == 0); column sgn (m d) + j_m d + j_d holds Z[i, j_d] where
 * mask[i, j_m] != 0 and zero elsewhere (a select: whatever Z holds in a masked-out row), negated for sgn = 1.  `mask` is the
 * host's (n, m) column-major bytes.  Same kind of result and the same handle rules as adelie_hip_design_create_one_hot; what the
 * design owns next to the expanded matrix is a column-major copy of Z and of the mask (n P + n d values and n m bytes), which
 * the structured full sweep (ADELIE_HIP_RELU_SWEEP, kernels_relu.hip) multiplies on the matrix cores. */
int adelie_hip_design_create_convex_relu(adelie_hip_design* Z, const uint8_t* mask, int64_t m, int gated, adelie_hip_design** out);
/* Additive entry point (the ABI version stays 14; callers look the symbol up).  The same design over a Z kept sparse
 * (adelie_hip_design_create_csc or an alias of one; a standardized view and every other kind of handle are refused), kept sparse
 * itself: column sgn (m d) + j_m d + j_d stores +-Z[i, j_d] at the rows where Z stores an entry and mask[i, j_m] != 0, so the
 * result holds (gated ? 1 : 2) sum_i popcount(mask[i, :]) nnz(Z[i, :]) entries and no n x P array is ever formed.  Built on the
 * device into the canonical six arrays of a design kept sparse (kernels_relu_sparse.hip; two builds give identical arrays), with
 * every operation, view and limit of adelie_hip_design_create_csc.  Next to the arrays the handle owns a copy of Z's compressed
 * columns and the mask packed to 32-bit words per row, which the structured full sweep (ADELIE_HIP_RELU_SWEEP) reads instead of
 * the expansion.  `mask` is the host's (n, m) column-major bytes. */
int adelie_hip_design_create_convex_relu_csc(adelie_hip_design* Z, const uint8_t* mask, int64_t m, int gated, adelie_hip_design** out);
/* The reference's read-only `groups` / `group_sizes` of the two classes above (outer[:-1] and diff(outer),
 * matrix_naive_one_hot.hpp / matrix_naive_interaction.hpp): copies min(G, cap) entries into each non-NULL array and returns the
 * number of blocks G, or -1 when `d` was not made by one of the two constructors (or is not an alias of such a design). */
int64_t adelie_hip_design_factor_groups(const adelie_hip_design* d, int64_t* groups, int64_t* group_sizes, int64_t cap);
/* Copies the (p,) impute vector of an SNP design (as double). */
int adelie_hip_design_impute(adelie_hip_design* d, double* out);
/* The float32 shadow that the filtered invariance sweep reads (made on the first eligible solve, shared with the aliases) is
 * freed; the next eligible solve makes it again.  To be called after the memory of an adopted tensor was modified, and with
 * no solve in flight on the design or its aliases.  shadow_stats: out[3] = {state (0 none, 1 built, -1 ineligible), builds,
 * times found ineligible (an entry float32 cannot hold, memory, a failed staleness check)}. */
int adelie_hip_design_drop_shadow(adelie_hip_design* d);
int adelie_hip_design_shadow_stats(adelie_hip_design* d, int64_t* out);
/* The copy as it stands: out_i[2] = {kind (0 float32, 1 int16 with one f64 scale per column: ADELIE_HIP_SHADOW_KIND, -1 when
 * there is no copy), its bytes on the device}, out_d[2] = {median, maximum over the columns of e_j / ||x_j||, the distance of a
 * column from its copy relative to its norm}.  An addition to ABI 14. */
int adelie_hip_design_shadow_info(adelie_hip_design* d, int64_t* out_i, double* out_d);
int adelie_hip_design_destroy(adelie_hip_design* d);
/* Diagnostic, an addition to ABI 14: the bytes of device memory that the design handles of this process own right now -- the
 * matrices, index arrays, tables and shadow copies that adelie_hip_design_destroy (or adelie_hip_design_drop_shadow) gives back,
 * plus the temporaries of a constructor while it runs.  Aliases, slices, views over a base and adopted tensors count nothing for
 * what they share.  Not counted: the handles' scratch space, the block cache, the sweep batcher and a solve's memory.  Free
 * device memory is device-wide; this count is the process's own, so tests can check the handles' ownership exactly. */
int64_t adelie_hip_design_owned_bytes(void);

/* cv_grpnet post-processing on the device (adelie/cv.py:296-312, diagnostic.py:30-121): for the L
 * sparse coefficient rows (CSR, int64 indices) computes eta_l = X beta_l + intercepts[l] + offsets and returns
 *   out[l]     = sum_i weights_a[i] * (A(eta_l,i) - y_i eta_l,i)        (the GLM's loss, glm_gaussian.ipp / glm_binomial.ipp)
 *   out[L + l] = the same under weights_b
 * without moving the (L, n) linear predictors to the host.  values / intercepts / offsets / y / weights in the design's dtype. */
int adelie_hip_design_glm_path_losses(adelie_hip_design* d, int glm_kind, int64_t L, const int64_t* indptr,
                                      const int64_t* indices, const void* values, const void* intercepts,
                                      const void* offsets, const void* y, const void* weights_a, const void* weights_b,
                                      double* out);
/* The same for multi-response fits (glm.multigaussian: glm_kind GAUSSIAN; glm.multinomial: MULTINOMIAL) on the BASE design:
 * row l of the CSR is a coefficient vector over the view columns feature*K + response (intercepts split off, as
 * state.betas holds them), intercepts is (L,K), offsets and y are (n,K) row-major, the weights (n,).  Replaces
 * diagnostic.predict through kronecker_eye + glm.loss per lambda in adelie/cv.py:281-314. */
int adelie_hip_design_multi_path_losses(adelie_hip_design* d, int glm_kind, int K, int64_t L, const int64_t* indptr,
                                        const int64_t* indices, const void* values, const void* intercepts,
                                        const void* offsets, const void* y, const void* weights_a, const void* weights_b,
                                        double* out);

int64_t adelie_hip_design_rows(const adelie_hip_design* d);   /* MatrixNaiveBase::rows */
int64_t adelie_hip_design_cols(const adelie_hip_design* d);   /* MatrixNaiveBase::cols */
int     adelie_hip_design_dtype(const adelie_hip_design* d);
int     adelie_hip_design_device(const adelie_hip_design* d);
/* Raw device pointer / HIP stream of the design (for callers that keep vectors on device). */
void*   adelie_hip_design_stream(const adelie_hip_design* d);

/* The MatrixNaiveBase virtuals (matrix_naive_base.hpp:18-144), host vectors in/out.
 * Semantics follow matrix_naive_dense.ipp line by line:                                   */
/* cmul  (:23-34):  *out = X[:,j] . (v * weights) */
int adelie_hip_design_cmul(adelie_hip_design* d, int64_t j, const void* v, const void* weights, double* out);
/* ctmul (:49-59):  out += v * X[:,j] */
int adelie_hip_design_ctmul(adelie_hip_design* d, int64_t j, double v, void* out);
/* bmul  (:61-80):  out = (v * weights)^T X[:, j:j+q] */
int adelie_hip_design_bmul(adelie_hip_design* d, int64_t j, int64_t q, const void* v, const void* weights, void* out);
/* btmul (:106-123): out += v^T X[:, j:j+q]^T */
int adelie_hip_design_btmul(adelie_hip_design* d, int64_t j, int64_t q, const void* v, void* out);
/* bmul / btmul over an explicit column list (any order, a column may repeat; on a design kept sparse the columns of btmul_cols
 * must be distinct): out[k] = x_cols[k] . (v o weights) for k < q, and out += sum_k v[k] x_cols[k].  On every design the matrix
 * operations take; on a design made of pieces (adelie_hip_design_create_pieces) these are the direct way to the kernels that
 * resolve a column's piece one by one, which bmul / btmul over a range do not take.  Additive: the ABI version stays. */
int adelie_hip_design_bmul_cols(adelie_hip_design* d, const int64_t* cols, int64_t q, const void* v, const void* weights, void* out);
int adelie_hip_design_btmul_cols(adelie_hip_design* d, const int64_t* cols, int64_t q, const void* v, void* out);
/* mul   (:125-146): out = (v * weights)^T X */
int adelie_hip_design_mul(adelie_hip_design* d, const void* v, const void* weights, void* out);
/* L sweeps in one call: out[l,:] = V[l,:]^T X for l < L; V is (L,n) and out (L,p), both row-major.  Replaces the loop of
 * X.mul calls in adelie/diagnostic.py:377-386 (gradients); the design (dense or 2-bit SNP) is streamed once per eight
 * vectors. */
int adelie_hip_design_mul_batch(adelie_hip_design* d, const void* V, int64_t L, void* out);
/* cov   (:162-197): out = X[:, j:j+q]^T diag(sqrt_weights^2) X[:, j:j+q], (q,q) column-major */
int adelie_hip_design_cov(adelie_hip_design* d, int64_t j, int64_t q, const void* sqrt_weights, void* out);
/* sq_mul (:199-217): out = weights^T X^2 */
int adelie_hip_design_sq_mul(adelie_hip_design* d, const void* weights, void* out);
/* sp_tmul (:219-256): out = V X^T with V an (L,p) CSR matrix, out (L,n) row-major */
int adelie_hip_design_sp_tmul(adelie_hip_design* d, int64_t L, const int64_t* indptr, const int64_t* indices,
                              const void* values, void* out);

/* ------------------------------------------------------------------------------------------
 * grpnet path solver
 *   == StateGaussianNaive{32,64}(...).solve(pb, exit_cond)   py_state.cpp:1068-1226
 *   == StateGlmNaive{32,64}(...).solve(glm, pb, exit_cond)   py_state.cpp:1556-1720
 * The struct carries exactly the constructor keyword arguments (py_state.cpp:1068-1154,
 * state_glm_naive.hpp:90-135); the Python sentinels are resolved by the caller the same way
 * adelie/state.py:1007-1045 resolves them (setup_lmda_max / setup_lmda_path / setup_loss_null).
 * ------------------------------------------------------------------------------------------ */
/* Polled once per saved lambda (the reference's exit_cond granularity, solver_base.hpp:581,679)
 * with `final`=1, and once per coordinate-descent fit with `final`=0 (the reference polls
 * PyErr_CheckSignals per CD sweep, py_state.cpp:70-74).  Return nonzero to stop:
 *   final=1 -> behaves as exit_cond() == True;  final=0 -> raises "interrupted" into error. */
typedef int (*adelie_hip_poll_fn)(void* user, int final, int64_t n_solutions, const adelie_hip_result* live);
/* `live` is the state being solved (the reference hands exit_cond the live C++ state, py_state.cpp:62-91): inside the callback
 * every adelie_hip_result_* accessor works on it -- lmdas, devs, intercepts, betas so far, screen / active sets, lmda, the
 * counters.  The device-resident invariants (grad, resid, eta, screen_beta, screen_X_means, screen_vars) are copied to the
 * host on request only: call adelie_hip_result_sync(live) first.  `live` must not be destroyed or kept by the callback. */
int adelie_hip_result_sync(const adelie_hip_result* live);

/* Host callbacks of a user-defined single-response GLM (glm_kind == ADELIE_HIP_GLM_CALLBACK).  They replace the virtuals of
 * GlmBase that the solver calls (glm_base.hpp:19-93; call sites solver_glm_naive.hpp:153,199-231,336-339,439-449): all arrays
 * are HOST pointers to n values of the design's dtype; return nonzero to abort the solve (recorded in the result's error
 * string).  `hessian` fills BOTH hess (GlmBase::hessian) and inv_hess_grad (GlmBase::inv_hessian_gradient, which a subclass may
 * override, glm_base.ipp:23-37) for the given eta and grad = gradient(eta).  loss_full crosses as the scalar in the args. */
typedef struct adelie_hip_glm_callbacks {
    void* user;
    int (*gradient)(void* user, const void* eta, void* grad);
    int (*hessian)(void* user, const void* eta, const void* grad, void* hess, void* inv_hess_grad);
    int (*loss)(void* user, const void* eta, double* loss);
} adelie_hip_glm_callbacks;

/* Host callbacks of the constraint objects the solver cannot run as a closed form on the device (constraint kind
 * ADELIE_HIP_CONSTRAINT_HOST): constraints on groups of several coefficients (the reference's ConstraintBox /
 * ConstraintOneSided proximal-Newton solvers, ConstraintLinear) and user-defined subclasses of ConstraintBase.  They stand
 * for the virtuals of ConstraintBase the solver calls (constraint_base.hpp:40-160; call sites
 * solver_gaussian_pin_naive.hpp:419-458, solver_base.hpp:62-93,158-222), exactly as the reference's PyConstraintBase
 * trampoline does (py_constraint.cpp).  `g` is the group, `d` its number of coefficients; all arrays are HOST doubles;
 * return nonzero to abort the solve.
 *   solve:      x (d) in/out in the coordinates of the group's eigenbasis Q (d x d, column-major), quad (d), linear (d)
 *   gradient:   out (d) = the constraint's term of the group's gradient at its current multipliers
 *   solve_zero: sets the multipliers that best explain v at x = 0; *norm = || v - gradient ||_2
 *   dual:       mu_out (m) = the object's multipliers, m = constraint_duals[g] */
typedef struct adelie_hip_constraint_callbacks {
    void* user;
    int (*solve)(void* user, int64_t g, int64_t d, double* x, const double* quad, const double* linear, double l1, double l2,
                 const double* Q);
    int (*gradient)(void* user, int64_t g, int64_t d, const double* x, double* out);
    int (*solve_zero)(void* user, int64_t g, int64_t d, const double* v, double* norm);
    int (*dual)(void* user, int64_t g, int64_t m, double* mu_out);
} adelie_hip_constraint_callbacks;
enum adelie_hip_constraint_kind {
    ADELIE_HIP_CONSTRAINT_NONE = 0,
    ADELIE_HIP_CONSTRAINT_BOX_1D = 1,       /* closed form on the device */
    ADELIE_HIP_CONSTRAINT_ONE_SIDED_1D = 2, /* closed form on the device */
    ADELIE_HIP_CONSTRAINT_HOST = 3          /* object on the caller's side, reached through adelie_hip_constraint_callbacks */
};

/* ABI 5.  Description of a `linear` constraint object (reference ConstraintLinear, adelie/constraint.py:137-306,
 * constraint_linear.ipp:142-217):  lower <= A z <= upper  on the group's d coefficients, m rows, with the settings of the
 * reference's proximal-Newton solver.  Like constraint_native / _va / _vb / _cfg it is read by the CPU checker (oracle/) only,
 * which runs such a group with its own restatement of that solver; libadelie_hip.so visits the group through constraint_cb. */
typedef struct adelie_hip_linear_constraint {
    int64_t        m, d;
    const double*  A;       /* (m, d) row-major */
    const double*  lower;   /* (m,) <= 0 (-1e100 and below: no bound) */
    const double*  upper;   /* (m,) >= 0 */
    const double*  vars;    /* (m,) squared row norms of A */
    double         cfg[7];  /* max_iters, tol, nnls_max_iters, nnls_tol, pinball_max_iters, pinball_tol, slack */
} adelie_hip_linear_constraint;

/* ABI 11.  Cox proportional-hazards family (reference GlmCox{32,64}, glm_cox.hpp / glm_cox.ipp).
 * create: start, stop, status, weights are (n,) HOST arrays of `dtype`, strata (n,) int64 in {0, ..., M-1} (NULL: one stratum),
 *   tie_method ADELIE_HIP_TIE_BRESLOW / _EFRON.  The library sorts (stratum, stop) and (stratum, start) (stable), finds the tie
 *   groups, the search positions of the at-risk sums, the tie sizes, averaged weights and Efron scales on the host, and uploads
 *   them once to `device`.  The handle is immutable afterwards: every solve / evaluation that uses it brings its own scratch,
 *   so concurrent solves may share it.  Weights are used as given (glm.cox normalises them).
 * eval: one evaluation at eta on the handle's device; eta (n,) HOST, grad / hess (n,) HOST outputs of `dtype` (the negative
 *   gradient and the diagonal Hessian of GlmCox), *loss; any output may be NULL.  Synchronous. */
enum adelie_hip_tie_method { ADELIE_HIP_TIE_BRESLOW = 0, ADELIE_HIP_TIE_EFRON = 1 };
int adelie_hip_glm_cox_create(int device, int dtype, int64_t n, const void* start, const void* stop, const void* status,
                              const int64_t* strata, const void* weights, int tie_method, adelie_hip_glm_cox** out);
int adelie_hip_glm_cox_destroy(adelie_hip_glm_cox* h);
int adelie_hip_glm_cox_eval(adelie_hip_glm_cox* h, const void* eta, void* grad, void* hess, double* loss);
/* cv_grpnet post-processing for the Cox family on the device (what adelie_hip_design_glm_path_losses is for the elementwise
 * families): for the L sparse coefficient rows (CSR, int64 indices) computes eta_l = X beta_l + intercepts[l] + offsets, formed
 * in the design's dtype in that order, and returns
 *   out[l]     = the loss of family ga at eta_l        (the double adelie_hip_glm_cox_eval(ga, eta_l) returns, bit for bit)
 *   out[L + l] = the same under gb
 * without moving the (L, n) linear predictors to the host.  ga and gb are two families over the design's rows that differ by
 * their weights (the full-data family and a fold's training family); both live on the design's device, in the design's dtype.
 * The etas of a panel are evaluated max_batch at a time, in a number of launches that does not depend on the batch; with
 * max_batch == 0 the batch is the largest whose Cox scratch stays within 1 GiB (6 n + 17 ceil(n / 1024) doubles per lambda).
 * The result does not depend on max_batch.  Works on every design sp_tmul works on.  values / intercepts / offsets in the
 * design's dtype.  Errors start with "cox_path_losses:".
 * The entry is additive and changes the layout of no existing structure: ADELIE_HIP_ABI_VERSION stays as it is. */
int adelie_hip_design_cox_path_losses(adelie_hip_design* d, const adelie_hip_glm_cox* ga, const adelie_hip_glm_cox* gb,
                                      int64_t L, const int64_t* indptr, const int64_t* indices, const void* values,
                                      const void* intercepts, const void* offsets, int64_t max_batch, double* out);

typedef struct adelie_hip_grpnet_args {
    /* ---- problem (static) ---- */
    int64_t        G;                 /* number of groups */
    const int64_t* groups;            /* (G,) start column of each group */
    const int64_t* group_sizes;       /* (G,) */
    double         alpha;
    const void*    penalty;           /* (G,) value_t */
    /* Gaussian (glm_kind == GAUSSIAN, the `opt` path of solver.py:683-686) */
    const void*    weights;           /* (n,) value_t, sums to 1 */
    const void*    X_means;           /* (p,) value_t */
    double         y_mean;
    double         y_var;
    double         resid_sum;
    double         rsq;
    /* GLM (glm_kind != GAUSSIAN): the GlmBase object is rebuilt on device from (y, weights) */
    int32_t        glm_kind;
    int32_t        _pad0;
    const void*    glm_y;             /* (n,) value_t */
    const void*    glm_weights;       /* (n,) value_t */
    const void*    offsets;           /* (n,) value_t */
    const void*    eta;               /* (n,) value_t */
    double         beta0;
    double         loss_null;         /* ignored if setup_loss_null */
    double         loss_full;
    int64_t        irls_max_iters;
    double         irls_tol;
    int32_t        setup_loss_null;
    int32_t        _pad1;
    /* shared dynamic inputs */
    const void*    resid;             /* (n,) value_t */
    const void*    grad;              /* (p,) value_t */
    /* ---- lambda path ---- */
    const void*    lmda_path;         /* (n_lmda_path,) value_t, may be NULL when setup_lmda_path */
    int64_t        n_lmda_path;
    double         lmda_max;          /* ignored if setup_lmda_max */
    double         min_ratio;
    int64_t        lmda_path_size;
    /* ---- configuration ---- */
    int64_t        max_screen_size;
    int64_t        max_active_size;
    double         pivot_subset_ratio;
    int64_t        pivot_subset_min;
    double         pivot_slack_ratio;
    int32_t        screen_rule;       /* adelie_hip_screen_rule */
    int32_t        early_exit;
    int64_t        max_iters;
    double         tol;
    double         adev_tol;
    double         ddev_tol;
    double         newton_tol;
    int64_t        newton_max_iters;
    int32_t        setup_lmda_max;
    int32_t        setup_lmda_path;
    int32_t        intercept;
    int32_t        n_threads;         /* accepted for API parity; host-side only */
    /* ---- warm-start invariants ---- */
    int64_t        screen_set_size;
    const int64_t* screen_set;        /* (s,) */
    int64_t        screen_beta_size;
    const void*    screen_beta;       /* (bs,) value_t */
    const int8_t*  screen_is_active;  /* (s,) */
    int64_t        active_set_size;
    const int64_t* active_set;        /* (G,) first active_set_size entries valid */
    double         lmda;              /* +inf for a cold start (solver.py:857) */
    /* ---- callbacks ---- */
    adelie_hip_poll_fn poll;          /* may be NULL */
    void*          poll_user;
    const adelie_hip_glm_callbacks* glm_cb; /* required iff glm_kind == ADELIE_HIP_GLM_CALLBACK */
    /* ---- covariance method (adelie_hip_gaussian_cov_solve only) ---- */
    const void*    cov_v;             /* (p,) value_t: the linear term v of 1/2 b'Ab - v'b */
    double         rdev_tol;          /* early exit on the relative change of the deviance (solver_gaussian_cov.hpp:183-201) */
    /* ---- per-group constraints (`constraints` of StateBase, state_base.hpp:60; adelie_core/constraint/) ----
     * Groups of ONE value with a box / one-sided constraint run as closed forms on the device (constraint_box.ipp:51-96,
     * constraint_one_sided.ipp:12-49); every other constraint object (several coefficients, linear, user-defined classes) is
     * kind 3: its group is visited on the host between two panel steps through constraint_cb (see above).  Accepted on every
     * state kind (naive, multi-response view, covariance method).
     *   kind 0: unconstrained;
     *   kind 1: box        constraint_a[i] <= beta_i <= constraint_b[i]   (a <= 0 <= b, infinities allowed); dual = mu_+ - mu_-
     *   kind 2: one-sided  constraint_a[i] * beta_i <= constraint_b[i]    (a = +-1, b >= 0);               dual = mu >= 0
     *   kind 3: host object; constraint_a / _b / _mu of the group are ignored.
     * NULL kind (or all zeros): no constraints. */
    const int32_t* constraint_kind;   /* (G,) */
    const void*    constraint_a;      /* (G,) value_t */
    const void*    constraint_b;      /* (G,) value_t */
    const void*    constraint_mu;     /* (G,) value_t or NULL: the multipliers the constraint objects hold on entry (warm start) */
    /* ABI 4 */
    const int64_t* constraint_duals;  /* (G,) number of multipliers of each group's constraint (ConstraintBase::duals; 0 = no
                                         constraint); NULL: one per constrained group.  Their running sum is `dual_groups`. */
    const adelie_hip_constraint_callbacks* constraint_cb; /* required when any kind is ADELIE_HIP_CONSTRAINT_HOST */
    /* What the CPU checker (oracle/) needs to run a kind-3 box / one-sided constraint with its OWN restatement of the
     * reference's solver instead of calling back (ABI 7: libadelie_hip.so solves 4 / 5 on the device from them too): constraint_native[g] = 0 (call back),
     * 4 (box: constraint_va = lower, constraint_vb = upper) or 5 (one-sided: va = sgn, vb = b), per COEFFICIENT (p,) arrays of
     * value_t indexed like the design's columns, and the solver settings (max_iters, tol, pinball_max_iters, pinball_tol,
     * slack) as 5 doubles per group. */
    const int32_t* constraint_native; /* (G,) or NULL */
    const void*    constraint_va;     /* (p,) value_t or NULL */
    const void*    constraint_vb;     /* (p,) value_t or NULL */
    const double*  constraint_cfg;    /* (G, 5) row-major or NULL */
    /* ABI 5: constraint_native[g] = 6 (linear): constraint_lin[g] describes the object (NULL entries elsewhere) */
    const adelie_hip_linear_constraint* const* constraint_lin; /* (G,) or NULL */
    /* ABI 7: kind-3 groups whose constraint_native is 4 (box) or 5 (one-sided) and that hold <= 64 coefficients are solved ON
     * THE DEVICE from constraint_va / _vb / _cfg (kernels_cons.hip: the reference's proximal-Newton dual solver in one
     * wavefront; no callback is made for them).  constraint_vmu: the multipliers those objects hold on entry, per COEFFICIENT
     * (p,) value_t, or NULL for zeros; what they hold on return is the result vector ADELIE_HIP_V_CONSTRAINT_VMU. */
    const void*    constraint_vmu;
    /* ABI 8: separate factors for the quadratic part of the penalty, (G,) value_t or NULL (= penalty): the objective's penalty
     * term becomes  lmda * sum_g (alpha * penalty[g] * |b_g| + (1 - alpha) / 2 * penalty_l2[g] * b_g^2).  Groups of one
     * coefficient only.  The reference has no such argument; it is what an elastic net on the standardized view
     * (Z - 1 c') diag(s)^-1 of a resident design needs to run on Z's own columns (penalty * |s|, penalty * s^2: every
     * coordinate update, screening score and KKT test is the same number in both coordinate systems, adelie_amd/solver.py). */
    const void*    penalty_l2;
    /* ABI 10: the lambda grid of a CV fold, assembled by the solve itself (adelie/cv.py:255-264 does it between two grpnet calls:
     * a first one with lmda_path_size = 0 for the fold's own lmda_max, then the path).  With lmda_path given
     * (setup_lmda_path = 0) and n_lmda_aug > 0 the solve, once its lmda_max is known, adds  lmda_max * lmda_aug_ratios[i]  for
     * every i whose product exceeds lmda_aug_min to the given path (all of them kept, sorted descending, cast to value_t) --
     * the numbers `state.lmda_max * np.logspace(0, log10(min_ratio), L)`, `> full_lmdas[0]`, `np.sort(np.concatenate(...))[::-1]`
     * produce; the first grpnet call (three sweeps over X and a state's worth of host work per fold) is not needed.  NULL / 0
     * for any other solve. */
    const double*  lmda_aug_ratios;
    int64_t        n_lmda_aug;
    double         lmda_aug_min;
    /* ABI 11: the family of glm_kind ADELIE_HIP_GLM_COX (required iff that kind; on the design's device).  NULL otherwise. */
    const adelie_hip_glm_cox* glm_cox;
} adelie_hip_grpnet_args;

/* Runs the whole path.  `*out` is always set on return code 0 (even when the solve recorded
 * an error string): the caller owns it and frees it with adelie_hip_result_destroy. */
int adelie_hip_grpnet_solve(adelie_hip_design* X, const adelie_hip_grpnet_args* args, adelie_hip_result** out);
/* ABI 10.  Replaces the fold loop of adelie.cv.cv_grpnet (adelie/cv.py:239-314, a Python `for fold in range(n_folds)` upstream)
 * for the solves it runs: `count` INDEPENDENT paths -- the folds' fits: the same matrix, their own weights / lambda grids /
 * warm starts in args[k] -- run concurrently, solve k on X[k], one host thread per solve below this call.  The handles are a
 * design and its aliases on one device (adelie_hip_design_alias: own stream and scratch each; with the "sweep_batch" config
 * on, the solves in flight share their full-gradient sweeps), or replicas on several devices of the node (each solve runs on
 * its handle's device; no collective is involved).  The same handle must not appear twice.  Callbacks in args[k] (poll, GLM,
 * constraints) are invoked from the solve's own thread, possibly several at once: a binding that needs a lock (the Python
 * binding: the interpreter lock, taken by ctypes) takes it there.  out[k] is what adelie_hip_grpnet_solve would have returned
 * for (X[k], args[k]) or NULL where that call failed; returns 0 when every solve returned 0, else 1 with the first failing
 * solve's message in adelie_hip_last_error.  `on_done` (may be NULL) is called from solve k's own thread as soon as that solve
 * has returned and out[k] is set -- rc = its return code -- while the other solves are still running: the caller's per-fold work
 * behind a path (cv.py:281-314: coefficients at the full-data grid, predictions, losses) overlaps with them instead of queueing
 * up behind the slowest fold. */
typedef void (*adelie_hip_done_fn)(int32_t k, int rc, void* user);
int adelie_hip_grpnet_solve_many(adelie_hip_design* const* X, const adelie_hip_grpnet_args* const* args, int32_t count,
                                 adelie_hip_result** out, adelie_hip_done_fn on_done, void* user);

/* ------------------------------------------------------------------------------------------
 * Covariance method  
 *   == adelie.matrix.dense(method="cov") / MatrixCovDense{32,64}{C,F}   (matrix_cov_dense.ipp:9-84)
 *   == StateGaussianCov{32,64}(...).solve(pb, exit_cond)                (py_state.cpp, state_gaussian_cov.hpp:40-145,
 *                                                                        solver_gaussian_cov.hpp:362-457)
 * minimises 1/2 b'Ab - v'b + penalty along a lambda path from summary statistics: A is a symmetric positive semi-definite
 * (p, p) matrix resident in HBM, the solver keeps grad = v - A b and never sees individual-level data.  The args struct is
 * the one of grpnet_solve; of it the covariance state reads the problem, path, configuration and warm-start fields,
 * `grad`, `rsq`, `cov_v` and `rdev_tol` (weights / X_means / resid / GLM fields are ignored; there is no intercept).
 * Result accessors as above: devs holds rsq (the unnormalised decrease of the loss), intercepts are zero.
 * ------------------------------------------------------------------------------------------ */
int adelie_hip_design_create_cov_dense(const void* host, int64_t p, int dtype, int order, int device, adelie_hip_design** out);
/* == adelie.matrix.sparse(method="cov", resident="csc") / MatrixCovSparse{32,64}{C,F} (matrix_cov_sparse.ipp) and
 * adelie.matrix.block_diag(method="cov", resident="csc") / MatrixCovBlockDiag: the covariance matrix kept sparse in HBM.  Only
 * the column-compressed form of the symmetric (p, p) matrix is uploaded (indptr of p + 1, row indices and values of indptr[p]
 * entries: 12 bytes per entry in f64, 8 in f32); the (p, p) array is never formed.  Inside a column the row indices must be
 * sorted and distinct and lie in [0, p); indptr starts at 0 and does not decrease; explicit zeros are kept.  The values are not
 * checked for symmetry, as on the dense handle.  The handle serves adelie_hip_gaussian_cov_solve, the three cov_* operations
 * below, adelie_hip_design_nnz, adelie_hip_design_csc_download (column form only) and adelie_hip_design_destroy;
 * adelie_hip_css_cov_solve refuses it (it keeps a dense (p, p) residual anyway). */
int adelie_hip_design_create_cov_csc(const int64_t* indptr, const int32_t* indices, const void* values, int64_t p, int dtype, int device,
                                     adelie_hip_design** out);
/* == adelie.matrix.lazy_cov(mat) / MatrixCovLazyCov{32,64}{C,F} (matrix_cov_lazy_cov.ipp): A = X^T X of a resident naive design
 * (dense or 2-bit SNP).  The reference computes rows of A on demand and caches them because A may not fit in host memory;
 * here the whole (p, p) matrix is formed once by the MFMA Gram kernel and kept in HBM (p = 100 000 is 80 GB of the 288),
 * after which it is an ordinary covariance-method design.  X is not retained. */
int adelie_hip_design_create_cov_lazy(adelie_hip_design* X, adelie_hip_design** out);
/* MatrixCovBase::bmul (matrix_cov_dense.ipp:23-41): out[j] = sum_i values[i] * A(indices[i], subset[j]) */
int adelie_hip_design_cov_bmul(adelie_hip_design* A, const int64_t* subset, int64_t n_subset, const int64_t* indices,
                               const void* values, int64_t n_indices, void* out);
/* MatrixCovBase::mul (:43-62): out = sum_i values[i] * A[indices[i], :] */
int adelie_hip_design_cov_mul(adelie_hip_design* A, const int64_t* indices, const void* values, int64_t n_indices, void* out);
/* MatrixCovBase::mul for many sparse vectors at once (what DiagnosticCov needs, reference diagnostic.py:1126-1170): for the L
 * rows beta_l of a CSR matrix (int64 indices; inside a row ascending and distinct) computes
 *   out[l, :] = v - A beta_l        (v == NULL: A beta_l)
 * into the (L, p) array `out`, rows contiguous; values, v and out in the handle's dtype.  Row l has the bits of
 * v - adelie_hip_design_cov_mul(beta_l), the subtraction in the handle's dtype, for every finite A, whichever rows share its
 * batch.  The rows are multiplied eight at a time: a matrix kept sparse is read once per eight rows, dense storage once per
 * column index of the eight rows' union.  The device scratch is that of a bounded number of rows (at most 128, fewer when p is
 * large), not of L.  Accepts covariance handles of both storages and refuses any other design; indptr / indices that are out of
 * range or not ascending inside a row are refused on the host before anything is uploaded.  L == 0 is a no-op.  Errors other
 * than a null argument start with "mul_batch:".
 * The entry is additive and changes the layout of no existing structure: ADELIE_HIP_ABI_VERSION stays as it is. */
int adelie_hip_design_cov_mul_batch(adelie_hip_design* A, int64_t L, const int64_t* indptr, const int64_t* indices,
                                    const void* values, const void* v, void* out);
/* MatrixCovBase::to_dense (:64-74): out = A[i:i+q, i:i+q], (q, q) column-major */
int adelie_hip_design_cov_to_dense(adelie_hip_design* A, int64_t i, int64_t q, void* out);
int adelie_hip_gaussian_cov_solve(adelie_hip_design* A, const adelie_hip_grpnet_args* args, adelie_hip_result** out);
/* == adelie.state.gaussian_pin_naive(...).solve() / gaussian_pin_cov(...).solve()  (solver_gaussian_pin_naive.hpp:217-401,
 * solver_gaussian_pin_cov.hpp:530-705): block coordinate descent along args->lmda_path on a screen set that never changes.
 * No screening, no KKT sweep, no lambda_max search.  `method` is ADELIE_HIP_PIN_NAIVE (a naive design) or ADELIE_HIP_PIN_COV
 * (a covariance handle; `screen_grad`, in the handle's dtype, holds v_S - A_SS beta_S in screen-value order and is ignored by
 * the naive method).  Of the args the entry reads what a pin state has: the problem (G, groups, group_sizes, alpha, penalty),
 * the Gaussian block (weights, X_means, y_mean, y_var; naive only), resid, rsq, resid_sum, lmda_path / n_lmda_path,
 * max_active_size, max_iters, tol, adev_tol, ddev_tol, rdev_tol, newton_tol, newton_max_iters, intercept, n_threads and the
 * warm-start block (screen_set, screen_beta, screen_is_active, active_set_size, active_set).  tol is absolute, as in the
 * reference's pin states; adev_tol / ddev_tol are taken as they come; max_iters bounds the iterations of the whole path.
 * grad and cov_v may be NULL (with cov_v NULL the linear term is put back together from screen_grad).  Constraints and
 * penalty_l2 are refused; so is a multi-response view.
 * A screen set that the single-workgroup descent takes runs the whole path in ONE launch (kernels_cd_pin.hip), or -- with
 * adelie_hip_set_config("pin_path_launch", 0) -- one launch per lambda; both give the same bits.  Larger screen sets run the
 * block / panel engines, one fit per lambda.  The path stops after the first lambda that meets an exit rule (naive:
 * rsq >= adev_tol * y_var, or rsqs[l] - rsqs[l-1] <= ddev_tol * y_var; cov: rsqs[l] - rsqs[l-1] <= rdev_tol * rsqs[l]); that
 * row is kept.  A lambda that fails ("max coordinate descents reached at lambda index: l.", "Maximum number of active groups
 * reached.") ends the solve: the rows before it are kept, the state is the one the last solved lambda left, the message is
 * adelie_hip_result_error.  Results: the accessors below; ADELIE_HIP_V_RSQS, ADELIE_HIP_V_BENCHMARK_SCREEN / _ACTIVE,
 * ADELIE_HIP_V_SCREEN_GRAD, ADELIE_HIP_I_ACTIVE_BEGINS / _ORDER and ADELIE_HIP_S_PIN_ITERS belong to this entry.
 * The entry is additive and changes the layout of no existing structure: ADELIE_HIP_ABI_VERSION stays as it is. */
enum adelie_hip_pin_method { ADELIE_HIP_PIN_NAIVE = 0, ADELIE_HIP_PIN_COV = 1 };
int adelie_hip_gaussian_pin_solve(adelie_hip_design* X, const adelie_hip_grpnet_args* args, int method, const void* screen_grad,
                                  adelie_hip_result** out);
int adelie_hip_result_destroy(adelie_hip_result* r);

/* ---- result accessors: the read-only properties of py_state.cpp:763-1040,1156-1217 ---- */
enum adelie_hip_vec {
    /* value vectors (copied out as double) */
    ADELIE_HIP_V_INTERCEPTS = 0, ADELIE_HIP_V_DEVS, ADELIE_HIP_V_LMDAS, ADELIE_HIP_V_LMDA_PATH,
    ADELIE_HIP_V_SCREEN_BETA, ADELIE_HIP_V_GRAD, ADELIE_HIP_V_ABS_GRAD, ADELIE_HIP_V_RESID,
    ADELIE_HIP_V_ETA, ADELIE_HIP_V_SCREEN_X_MEANS, ADELIE_HIP_V_SCREEN_VARS,
    ADELIE_HIP_V_SCREEN_TRANSFORMS, /* concatenated column-major (q,q) blocks in screen order */
    ADELIE_HIP_V_BENCHMARK_SCREEN, ADELIE_HIP_V_BENCHMARK_FIT_SCREEN, ADELIE_HIP_V_BENCHMARK_FIT_ACTIVE,
    ADELIE_HIP_V_BENCHMARK_KKT, ADELIE_HIP_V_BENCHMARK_INVARIANCE,
    /* adelie_hip_gaussian_pin_solve: rsq after each solved lambda; the active-pass share of each lambda's time (the screen-pass
     * share is ADELIE_HIP_V_BENCHMARK_SCREEN); the final screen gradient of the covariance method */
    ADELIE_HIP_V_RSQS, ADELIE_HIP_V_BENCHMARK_ACTIVE, ADELIE_HIP_V_SCREEN_GRAD,
    /* index vectors (copied out as int64) */
    ADELIE_HIP_I_SCREEN_SET = 100, ADELIE_HIP_I_SCREEN_BEGINS, ADELIE_HIP_I_SCREEN_IS_ACTIVE,
    ADELIE_HIP_I_ACTIVE_SET, ADELIE_HIP_I_N_VALID_SOLUTIONS, ADELIE_HIP_I_ACTIVE_SIZES,
    ADELIE_HIP_I_SCREEN_SIZES, ADELIE_HIP_I_BETAS_INDPTR, ADELIE_HIP_I_BETAS_INDICES,
    /* duals, CSR (L, n_duals) (state_base.hpp `duals`, filled by sparsify_dual, solver_base.hpp:158-222); n_duals = number
     * of constrained groups here (one multiplier per singleton constraint) */
    ADELIE_HIP_I_DUALS_INDPTR, ADELIE_HIP_I_DUALS_INDICES,
    /* ABI 9: the groups whose box / one-sided constraint objects were solved ON THE DEVICE during this solve (ascending group
     * indices; their multipliers are the entries of ADELIE_HIP_V_CONSTRAINT_VMU) -- the binding reads this list instead of
     * re-deriving the library's rule, and the objects of every other group stayed live on the caller's side */
    ADELIE_HIP_I_CONSTRAINT_DEV_GROUPS,
    /* adelie_hip_gaussian_pin_solve: active_begins / active_order of the reference's pin states */
    ADELIE_HIP_I_ACTIVE_BEGINS, ADELIE_HIP_I_ACTIVE_ORDER,
    /* betas values (double), CSR (L, p) like convert_sparse_to_dense's input, py_state.cpp:9-60 */
    ADELIE_HIP_V_BETAS_VALUES = 200,
    ADELIE_HIP_V_DUALS_VALUES,
    /* (G,) the multiplier each constraint object is left holding when the solve returns (0 for unconstrained groups) */
    ADELIE_HIP_V_CONSTRAINT_MU,
    /* ABI 7: (p,) per coefficient, the multipliers of the box / one-sided objects that were solved on the device (0 elsewhere) */
    ADELIE_HIP_V_CONSTRAINT_VMU
};
enum adelie_hip_scalar {
    ADELIE_HIP_S_LMDA_MAX = 0, ADELIE_HIP_S_LMDA, ADELIE_HIP_S_RSQ, ADELIE_HIP_S_RESID_SUM,
    ADELIE_HIP_S_ACTIVE_SET_SIZE, ADELIE_HIP_S_BETA0, ADELIE_HIP_S_LOSS_NULL, ADELIE_HIP_S_LOSS_FULL,
    ADELIE_HIP_S_TOTAL_TIME,
    /* instrumentation used by bench.py for the algorithmic-byte count */
    ADELIE_HIP_S_N_BASIL_ITERS = 50, ADELIE_HIP_S_N_SWEEPS, ADELIE_HIP_S_N_CD_VISITS_SCREEN,
    ADELIE_HIP_S_N_CD_VISITS_ACTIVE, ADELIE_HIP_S_N_UPDATES, ADELIE_HIP_S_N_IRLS_ITERS,
    ADELIE_HIP_S_N_NEW_SCREEN_COLS, ADELIE_HIP_S_N_CD_PASSES_SCREEN, ADELIE_HIP_S_N_CD_PASSES_ACTIVE,
    ADELIE_HIP_S_N_GRAM_COL_READS, ADELIE_HIP_S_N_RESID_COL_READS, ADELIE_HIP_S_GRAM_FLOPS,
    ADELIE_HIP_S_N_PANEL_BLOCKS, ADELIE_HIP_S_N_PANEL_GRAMS, /* block visits / diagonal blocks built by the panel engine */
    ADELIE_HIP_S_N_PANEL_COLS, /* design columns streamed by the panel steps (gradient + residual update) */
    ADELIE_HIP_S_N_IRLS_SCREEN_COLS, /* sum over IRLS iterations of the screened columns (their means and variances are
                                        recomputed under every iteration's weights: the IRLS term of SURVEY.md 8d's B_path) */
    ADELIE_HIP_S_N_SPECULATED,       /* fits whose first active-set pass was enqueued behind the previous lambda's sweep */
    ADELIE_HIP_S_N_SPEC_ROLLBACKS,   /* ... of which were taken back (KKT failure, early exit, live-state read) */
    ADELIE_HIP_S_N_SWEEPS_SHARED,    /* full-gradient sweeps of this solve that were answered by a launch shared with other
                                        solvers on the same design (cv_grpnet folds in flight): X is streamed once for all */
    ADELIE_HIP_S_N_UPDATE_COLS,      /* design columns streamed by the residual updates of the panel steps (n_updates counts
                                        groups on grouped problems; this counts their columns) */
    ADELIE_HIP_S_N_DEVICE_SCREENS,   /* screening steps (solver_base.hpp:273-403) whose decision was taken on the device
                                        (kernels_screen.hip) ... */
    ADELIE_HIP_S_N_HOST_SCREENS,     /* ... and by the host routine (first iteration, host constraint objects, G > 2^18) */
    ADELIE_HIP_S_N_HOST_CONS_VISITS, /* ABI 7: visits of constrained groups made on the host through the callbacks ... */
    ADELIE_HIP_S_N_DEV_CONS_VISITS,  /* ... and by the device kernel (box / one-sided objects, kernels_cons.hip) */
    ADELIE_HIP_S_N_SWEEPS_FACTOR,    /* ABI 12: full-gradient sweeps of a one-hot / interaction design answered by the structured
                                        kernel (kernels_factor.hip: read off Z, not off the expanded matrix) */
    /* the filtered invariance sweep (float32 shadow of a dense f64 design, ADELIE_HIP_FILTER_SWEEP): */
    ADELIE_HIP_S_N_SWEEPS_FILTERED,  /* invariance sweeps answered by the shadow sweep + exact sweeps of the columns it left open */
    ADELIE_HIP_S_N_SWEEPS_REFILLED,  /* ... of which were followed by the full sweep after all (every value had to be exact) */
    ADELIE_HIP_S_N_FILTER_EXACT_COLS,  /* columns the filtered sweeps read in f64 */
    ADELIE_HIP_S_N_FILTER_SHADOW_COLS, /* columns the filtered sweeps read from the shadow */
    /* HIP-event time (ms) of the device phases on the design's stream, summed over the solve, and launch counts */
    ADELIE_HIP_S_T_SWEEP_MS = 80, ADELIE_HIP_S_T_GRAM_MS, ADELIE_HIP_S_T_CD_MS, ADELIE_HIP_S_T_AXPY_MS,
    ADELIE_HIP_S_N_SWEEP_LAUNCHES, ADELIE_HIP_S_N_GRAM_LAUNCHES, ADELIE_HIP_S_T_HOST_SCREEN_MS,
    /* per-launch timing of the panel step kernel; only collected when ADELIE_HIP_TIME_PANEL=1 (adds two events per launch) */
    ADELIE_HIP_S_T_PANEL_STEP_MS, ADELIE_HIP_S_N_PANEL_STEP_LAUNCHES,
    /* the part of T_HOST_SCREEN_MS the host spent waiting for the device (stream / event synchronisation) rather than
     * computing the screening rule, the appends and the launches of the new groups' variances */
    ADELIE_HIP_S_T_HOST_SCREEN_WAIT_MS,
    /* the filtered invariance sweeps as a whole (T_SWEEP_MS / N_SWEEP_LAUNCHES count the launches that read the whole f64
     * design only): time, count, and the design bytes they asked for */
    ADELIE_HIP_S_T_FSWEEP_MS, ADELIE_HIP_S_N_FSWEEP_LAUNCHES, ADELIE_HIP_S_FSWEEP_BYTES,
    /* the pivot rule's reading of the sorted scores (ADELIE_HIP_FILTER_DEPTH): positions screen() read, counted from the top
     * and summed over its calls; threshold passes that fell short of what the rule read (each takes the full sweep and the
     * sort of all G after all); columns the filtered sweeps listed as open and read a second time in f64 */
    ADELIE_HIP_S_N_SCREEN_READS, ADELIE_HIP_S_N_SCREEN_SHORT, ADELIE_HIP_S_N_FILTER_OPEN_COLS,
    /* 1 when the set-up of this solve left the panel engines open to it (they take a fit once its screen set is large enough),
     * 0 when it kept the solve on the full-Gram engines throughout: the covariance method, a design kept sparse or a
     * standardized view without their panel forms, and always a design made of pieces (adelie_hip_design_create_pieces) */
    ADELIE_HIP_S_ENGINE_PANEL,
    /* adelie_hip_gaussian_pin_solve: iterations (passes) of the whole path; descent launches (one-launch route: 1; one launch
     * per lambda: the lambdas it ran; block / panel engines: their fits); the route taken (1: one launch, 2: one launch per
     * lambda, 3: block engine, 4: panel engine) */
    ADELIE_HIP_S_PIN_ITERS, ADELIE_HIP_S_N_PIN_LAUNCHES, ADELIE_HIP_S_PIN_ROUTE
};
int64_t     adelie_hip_result_size(const adelie_hip_result* r, int which);
/* Copies min(size, cap) elements: value vectors as double, index vectors as int64. */
int         adelie_hip_result_copy(const adelie_hip_result* r, int which, void* out, int64_t cap);
double      adelie_hip_result_scalar(const adelie_hip_result* r, int which);
const char* adelie_hip_result_error(const adelie_hip_result* r);

/* ------------------------------------------------------------------------------------------
 * ABI 13.  Column subset selection on a resident covariance matrix
 *   == adelie.solver.css_cov / StateCSSCov{32,64}(...).solve()   (state_css_cov.ipp:8-67, solver_css_cov.hpp:164-537)
 * `A` is a dense covariance-method handle (adelie_hip_design_create_cov_dense / _cov_lazy; one kept sparse is refused), assumed symmetric and never modified.
 * The solve keeps one (p, p) residual covariance in HBM (both triangles, so that every access is a contiguous column) and
 * streams it once per rank-one update with the loss's per-column score fused into the pass (kernels_css.hip).  Greedy runs
 * without a host synchronisation inside its loop; swapping makes one small device -> host read per attempt (a record of
 * scalars and k + 1 entries of A) and keeps its k x k Cholesky algebra on the host in double.  The args carry the
 * constructor arguments of the reference's state; its checks (state_css_cov.ipp:15-57) fail the call, errors raised inside
 * the solve ("Initial subset are not linearly independent columns.", "Maximum swapping cycles reached!") are recorded in the
 * result's error string.  Results are bit-reproducible run to run.
 * ------------------------------------------------------------------------------------------ */
enum adelie_hip_css_method { ADELIE_HIP_CSS_GREEDY = 0, ADELIE_HIP_CSS_SWAPPING = 1 };
enum adelie_hip_css_loss { ADELIE_HIP_CSS_LEAST_SQUARES = 0, ADELIE_HIP_CSS_SUBSET_FACTOR = 1, ADELIE_HIP_CSS_MIN_DET = 2 };
typedef struct adelie_hip_css_args {
    int64_t        subset_size;
    const int64_t* subset;      /* (n_subset,) the initial subset of swapping; greedy: n_subset = 0 */
    int64_t        n_subset;
    int32_t        method;      /* adelie_hip_css_method */
    int32_t        loss;        /* adelie_hip_css_loss */
    int64_t        max_iters;   /* swapping: cycles over the subset */
    int32_t        n_threads;   /* accepted for API parity (>= 1) */
    int32_t        _pad0;
} adelie_hip_css_args;
int adelie_hip_css_cov_solve(adelie_hip_design* A, const adelie_hip_css_args* args, adelie_hip_css_result** out);
int adelie_hip_css_result_destroy(adelie_hip_css_result* r);
enum adelie_hip_css_vec {
    ADELIE_HIP_CSS_SUBSET = 0,       /* (k,) int64, in selection order (swapping: positional) */
    ADELIE_HIP_CSS_S_RESID = 1,      /* (p, p) column-major values of the design's dtype, fetched from the device by the copy;
                                        size 0 when swapping returned at once (k <= 0 or k >= p) */
    ADELIE_HIP_CSS_S_RESID_DIAG = 2, /* (p,) its diagonal, design's dtype (already on the host) */
    ADELIE_HIP_CSS_L_T = 3           /* (k, k) column-major double: lower Cholesky factor of A[T, T], T in the rotated order */
};
enum adelie_hip_css_scalar {
    ADELIE_HIP_CSS_N_UPDATES = 0,    /* rank-one passes over the matrix */
    ADELIE_HIP_CSS_N_SWAPS,
    ADELIE_HIP_CSS_N_ATTEMPTS,       /* swapping attempts (= host round trips inside the loop) */
    ADELIE_HIP_CSS_EARLY_EXIT,       /* the score routine's early-exit flag at the last attempt */
    ADELIE_HIP_CSS_TOTAL_TIME        /* seconds */
};
int64_t     adelie_hip_css_result_size(const adelie_hip_css_result* r, int which);
/* Copies min(size, cap) elements in the element type named above. */
int         adelie_hip_css_result_copy(const adelie_hip_css_result* r, int which, void* out, int64_t cap);
double      adelie_hip_css_result_scalar(const adelie_hip_css_result* r, int which);
const char* adelie_hip_css_result_error(const adelie_hip_css_result* r);

/* ------------------------------------------------------------------------------------------
 * ABI 14.  Bounded-variable least squares   min 1/2 ||y - X beta||_W^2  s.t.  lower <= beta <= upper
 *   == adelie.solver.bvls / StateBVLS{32,64}(...).solve()   (state_bvls.ipp:8-84, solver_bvls.hpp:22-348)
 * `X` is a plain dense handle (kind dense, no standardized view, not a covariance handle).  The reference's coordinate descent
 * with its visiting order, predicates and counters; a visit reads the coordinate's gradient from a vector that is kept current
 * through the resident screen Gram matrix X_S^T W X_S instead of two passes over n rows, one workgroup runs a whole fit(), and
 * the residual is caught up once per fit (kernels_bvls.hip).  All vectors are host pointers of the design's dtype; the args
 * carry the constructor arguments of the reference's state with their lengths; its checks (state_bvls.ipp:15-74) fail the call.
 * Errors raised inside the solve ("bvls: max iterations reached!", the Gram limit) are recorded in the result's error string
 * and the result carries the state reached.  Ties between equal violations go to the lower index (the reference's std::sort
 * leaves them unspecified).  Results are bit-reproducible run to run.
 * ------------------------------------------------------------------------------------------ */
typedef struct adelie_hip_bvls_args {
    const void*    X_vars;      /* (n_X_vars,) */
    const void*    lower;       /* (n_lower,) */
    const void*    upper;       /* (n_upper,) */
    const void*    weights;     /* (n_weights,) */
    const void*    beta;        /* (n_beta,) */
    const void*    resid;       /* (n_resid,) */
    const void*    grad;        /* (n_grad,) returned unchanged when no KKT round runs */
    int64_t        n_X_vars, n_lower, n_upper, n_weights, n_beta, n_resid, n_grad;
    const int64_t* screen_set;  /* the first screen_set_size entries are read */
    int64_t        screen_set_size;
    const int64_t* active_set;  /* (n_active_set,) buffer, the first active_set_size entries are read */
    int64_t        active_set_size;
    int64_t        n_active_set, n_is_active; /* buffer lengths of the caller's state (checked against p) */
    double         y_var;
    double         loss;
    int64_t        kappa;
    int64_t        max_iters;
    double         tol;
} adelie_hip_bvls_args;
int adelie_hip_bvls_solve(adelie_hip_design* X, const adelie_hip_bvls_args* args, adelie_hip_bvls_result** out);
int adelie_hip_bvls_result_destroy(adelie_hip_bvls_result* r);
enum adelie_hip_bvls_vec {
    ADELIE_HIP_BVLS_BETA = 0,        /* (p,) design's dtype */
    ADELIE_HIP_BVLS_RESID = 1,       /* (n,) design's dtype */
    ADELIE_HIP_BVLS_GRAD = 2,        /* (p,) design's dtype: the violations of the last KKT round */
    ADELIE_HIP_BVLS_SCREEN_SET = 3,  /* (screen_set_size,) int64, in order */
    ADELIE_HIP_BVLS_ACTIVE_SET = 4,  /* (active_set_size,) int64, in order */
    ADELIE_HIP_BVLS_IS_SCREEN = 5,   /* (p,) uint8 */
    ADELIE_HIP_BVLS_IS_ACTIVE = 6    /* (p,) uint8 */
};
enum adelie_hip_bvls_scalar {
    ADELIE_HIP_BVLS_LOSS = 0,
    ADELIE_HIP_BVLS_ITERS,
    ADELIE_HIP_BVLS_N_KKT,
    ADELIE_HIP_BVLS_SCREEN_SET_SIZE,
    ADELIE_HIP_BVLS_ACTIVE_SET_SIZE,
    ADELIE_HIP_BVLS_TOTAL_TIME,      /* seconds */
    ADELIE_HIP_BVLS_T_SWEEP_MS,      /* HIP-event time of the full and screen sweeps (with their w * r products) */
    ADELIE_HIP_BVLS_T_GRAM_MS,       /* ... of the Gram builds */
    ADELIE_HIP_BVLS_T_FIT_MS,        /* ... of the fit kernel */
    ADELIE_HIP_BVLS_N_CHANGED        /* visits that changed a coefficient, over all fits */
};
int64_t     adelie_hip_bvls_result_size(const adelie_hip_bvls_result* r, int which);
/* Copies min(size, cap) elements in the element type named above. */
int         adelie_hip_bvls_result_copy(const adelie_hip_bvls_result* r, int which, void* out, int64_t cap);
double      adelie_hip_bvls_result_scalar(const adelie_hip_bvls_result* r, int which);
const char* adelie_hip_bvls_result_error(const adelie_hip_bvls_result* r);

/* ------------------------------------------------------------------------------------------
 * Constraint matrices and pinball least squares.  Additions to ABI 14: nothing that existed changes, so the version number
 * stays (tests/test_bvls_host.py pins it).
 *     min over beta in R^m   1/2 || S^{-1/2} v - S^{1/2} A' beta ||^2 + penalty_neg' beta_- + penalty_pos' beta_+
 *   == adelie.matrix.dense(method="constraint") / MatrixConstraintDense{32,64}{C,F}   (matrix_constraint_base.hpp)
 *   == adelie.solver.pinball / StatePinball{32,64}(...).solve()   (state_pinball.ipp:8-104, solver_pinball.hpp:11-309)
 *
 * A constraint handle holds the (m, d) matrix A row-major, i.e. the (d, m) column-major matrix A' of an ordinary dense handle
 * (design_rows == d, design_cols == m) with a `constraint` flag: a row of A is one contiguous column, A v is the column sweep
 * and v' A the column axpy.  `order` names the memory order of the (m, d) source: a row-major source is taken as it lies (a
 * device one is adopted in place), a column-major one is transposed once.  Every entry point that takes a naive design
 * (grpnet_solve, bvls_solve, the MatrixNaiveBase operations, views, slices, concatenations, factor designs, lazy_cov) refuses a
 * handle with the flag; only adelie_hip_constraint_op, adelie_hip_pinball_solve and the design_{rows,cols,dtype,device,stream,
 * destroy} accessors take one.  The handle makes no float32 shadow copy.
 * ------------------------------------------------------------------------------------------ */
int adelie_hip_design_create_constraint_dense(const void* host, int64_t m, int64_t d, int dtype, int order, int device,
                                              adelie_hip_design** out);
int adelie_hip_design_adopt_constraint_dense_dev(const void* dev_ptr, int64_t m, int64_t d, int dtype, int order, int device,
                                                 adelie_hip_design** out);
/* Additive entry point (the ABI version stays 14; callers look the symbol up).  Replaces MatrixConstraintSparse{32,64}
 * (adelie.matrix.sparse(method="constraint"), adelie/matrix.py:1301-1411, matrix_constraint_sparse.ipp): the (m, d) matrix A kept
 * sparse.  A is given twice in canonical form (sorted distinct indices), row-compressed (row_indptr of m + 1) and
 * column-compressed (col_indptr of d + 1) -- the pair adelie_hip_design_create_csc takes for the (d, m) matrix A', whose
 * compressed columns are A's rows.  The handle is that design kept sparse (design_rows == d, design_cols == m, 24 bytes per
 * stored entry in f64) with the `constraint` flag: a row of A is one compressed column.  It is taken and refused exactly where
 * the dense constraint handle is: adelie_hip_constraint_op (all operations; rmmul, cov and the solve's A_S S and A_S S A_S' run
 * over the stored entries, kernels_pinball_sparse.hip) and adelie_hip_pinball_solve take it, every naive entry point refuses it.
 * m and d must be positive and below 2^31. */
int adelie_hip_design_create_constraint_csc(const int64_t* row_indptr, const int32_t* row_indices, const void* row_values,
                                            const int64_t* col_indptr, const int32_t* col_indices, const void* col_values, int64_t m,
                                            int64_t d, int dtype, int device, adelie_hip_design** out);
/* The MatrixConstraintBase operations; all vectors are host pointers of the handle's dtype.  None of them is a hot path. */
enum adelie_hip_constraint_op_kind {
    ADELIE_HIP_CONS_TMUL = 0,    /* out (m,) = A in,  in (d,) */
    ADELIE_HIP_CONS_MUL = 1,     /* out (d,) = in' A, in (m,) */
    ADELIE_HIP_CONS_SP_MUL = 2,  /* out (d,) = sum_i in[i] A[indices[i], :], n_indices entries, indices in [0, m) */
    ADELIE_HIP_CONS_RVMUL = 3,   /* out (1,) = A[j, :] . in,  in (d,) */
    ADELIE_HIP_CONS_RVTMUL = 4,  /* out (d,) += in[0] * A[j, :] */
    ADELIE_HIP_CONS_RMMUL = 5,   /* out (d,) = A[j, :] Q,  in = Q (d, d) column-major */
    ADELIE_HIP_CONS_COV = 6,     /* out (m, m) column-major = A Q A',  in = Q (d, d) column-major */
    ADELIE_HIP_CONS_TO_DENSE = 7 /* out (m, d) row-major = A */
};
int adelie_hip_constraint_op(adelie_hip_design* A, int op, int64_t j, const void* in, const int64_t* indices, int64_t n_indices,
                             void* out);

/* The reference's coordinate descent with its visiting order, predicates and counters.  A visit reads the coordinate's gradient
 * from a vector that is kept current through the resident matrix H = A_S S A_S' of the screen set instead of a d-long dot, one
 * workgroup runs a whole fit() (the kernel bvls_solve runs, with the pinball update), the residual is caught up once per fit from
 * the compact rows A_S S, and a KKT round is one sweep over the m rows plus a host sort (kernels_pinball.hip).  `S` is (d, d)
 * column-major; all vectors are host pointers of the handle's dtype; the args carry the constructor arguments of the reference's
 * state with their lengths, and its checks (state_pinball.ipp:15-94) fail the call.  screen_ASAT_diag / screen_AS are not passed
 * in (the solve builds them for the caller's screen set); n_screen_ASAT_diag, screen_AS_rows and screen_AS_cols are the shapes
 * of the caller's buffers for those checks.  Errors raised inside the solve ("pinball: max iterations reached!", the limit on H)
 * are recorded in the result's error string and the result carries the state reached.  Ties between equal violations go to the
 * lower index.  Results are bit-reproducible run to run.
 * adelie_hip_set_config: "pinball_gram_limit_mb" (default 16384) bounds H; "pinball_lds_max_ns" (default 0 = as many as the
 * device's LDS holds) keeps the fit kernel's per-coordinate state in global memory beyond that many screen members. */
typedef struct adelie_hip_pinball_args {
    const void*    S;           /* (S_rows, S_cols) column-major */
    const void*    penalty_neg; /* (n_penalty_neg,) */
    const void*    penalty_pos; /* (n_penalty_pos,) */
    const void*    beta;        /* (n_beta,) */
    const void*    resid;       /* (n_resid,) */
    const void*    grad;        /* (n_grad,) returned unchanged when no KKT round runs */
    int64_t        S_rows, S_cols, n_penalty_neg, n_penalty_pos, n_beta, n_resid, n_grad;
    const int64_t* screen_set;  /* the first screen_set_size entries are read */
    int64_t        screen_set_size;
    const int64_t* active_set;  /* the first active_set_size entries are read */
    int64_t        active_set_size;
    int64_t        n_screen_set, n_is_screen, n_active_set, n_is_active; /* buffer lengths of the caller's state */
    int64_t        n_screen_ASAT_diag, screen_AS_rows, screen_AS_cols;
    double         y_var;
    double         loss;
    int64_t        kappa;
    int64_t        max_iters;
    double         tol;
} adelie_hip_pinball_args;
int adelie_hip_pinball_solve(adelie_hip_design* A, const adelie_hip_pinball_args* args, adelie_hip_pinball_result** out);
int adelie_hip_pinball_result_destroy(adelie_hip_pinball_result* r);
enum adelie_hip_pinball_vec {
    ADELIE_HIP_PINBALL_BETA = 0,         /* (m,) handle's dtype */
    ADELIE_HIP_PINBALL_RESID = 1,        /* (d,) handle's dtype */
    ADELIE_HIP_PINBALL_GRAD = 2,         /* (m,) handle's dtype: the violations of the last KKT round */
    ADELIE_HIP_PINBALL_SCREEN_SET = 3,   /* (screen_set_size,) int64, in order */
    ADELIE_HIP_PINBALL_ACTIVE_SET = 4,   /* (active_set_size,) int64, in order */
    ADELIE_HIP_PINBALL_IS_SCREEN = 5,    /* (m,) uint8 */
    ADELIE_HIP_PINBALL_IS_ACTIVE = 6,    /* (m,) uint8 */
    ADELIE_HIP_PINBALL_SCREEN_ASAT_DIAG = 7, /* (screen_set_size,) handle's dtype, screen order */
    ADELIE_HIP_PINBALL_SCREEN_AS = 8     /* (screen_set_size, d) row-major, screen order: copied from the device at this call */
};
enum adelie_hip_pinball_scalar {
    ADELIE_HIP_PINBALL_LOSS = 0,
    ADELIE_HIP_PINBALL_ITERS,
    ADELIE_HIP_PINBALL_N_KKT,
    ADELIE_HIP_PINBALL_SCREEN_SET_SIZE,
    ADELIE_HIP_PINBALL_ACTIVE_SET_SIZE,
    ADELIE_HIP_PINBALL_TOTAL_TIME,       /* seconds */
    ADELIE_HIP_PINBALL_T_SWEEP_MS,       /* HIP-event time of the full and screen sweeps */
    ADELIE_HIP_PINBALL_T_GRAM_MS,        /* ... of the A_S S and H builds */
    ADELIE_HIP_PINBALL_T_FIT_MS,         /* ... of the fit kernel */
    ADELIE_HIP_PINBALL_N_CHANGED         /* visits that changed a coefficient, over all fits */
};
int64_t     adelie_hip_pinball_result_size(const adelie_hip_pinball_result* r, int which);
/* Copies min(size, cap) elements in the element type named above. */
int         adelie_hip_pinball_result_copy(const adelie_hip_pinball_result* r, int which, void* out, int64_t cap);
double      adelie_hip_pinball_result_scalar(const adelie_hip_pinball_result* r, int which);
const char* adelie_hip_pinball_result_error(const adelie_hip_pinball_result* r);

/* ------------------------------------------------------------------------------------------
 * Kernel-level timing hook used by bench.py (HIP events on the design's own stream):
 * runs `reps` launches of the dominant kernel (the full gradient sweep grad = X^T(w*r) - rs*X_means
 * with fused per-group abs_grad) on resident buffers and returns the mean milliseconds per launch.
 * On a one-hot / interaction design it times the route ADELIE_HIP_FACTOR_SWEEP selects (read at the call).
 * On a convex-relu design likewise the route ADELIE_HIP_RELU_SWEEP selects.
 * ------------------------------------------------------------------------------------------ */
int adelie_hip_bench_sweep(adelie_hip_design* d, int64_t reps, double* ms_per_launch);
/* One filtered invariance sweep on a dense f64 design (tests): v = w o r, the float32 shadow sweep, the classification of the
 * groups outside `screen_groups` against tstar * penalty, the exact f64 sweeps of the columns left open.  grad (p), exact (p
 * bytes: 1 where the value is bit for bit the full sweep's), info[4] = {columns listed, flags (1: more than max(1024, p/4)
 * columns were wanted, 2: a column swept both ways left its bound), 1 if the route ran / 0 if the plain full sweep answered
 * (ADELIE_HIP_FILTER_SWEEP=0, a design without a shadow), columns wanted}. */
int adelie_hip_filter_sweep_test(adelie_hip_design* d, const double* w, const double* r, double sub_scale, const double* sub_vec,
                                 const int64_t* screen_groups, int64_t n_screen, const int64_t* groups, const int64_t* group_sizes,
                                 int64_t G, const double* penalty, double tstar, double* grad, uint8_t* exact, int64_t* info);

/* One block build of the panel engine on caller-supplied inputs (tests): ONE build launch and its reduce, through the launcher
 * the solver calls.  The design is plain dense (f64 / f32), 2-bit or compressed-column; w (n - row_off), xm (p, may be null when
 * center == 0) and the outputs are in the design's element type.  row_off > 0 (dense only) builds on rows [row_off, n) of the
 * design: an offset that is not a multiple of 16 bytes selects the kernels' scalar-load variants.
 * mode 0: one diagonal block; 1: a batch of diagonal blocks (<= 16); 2: the general Gram panel (the design-kind dispatch);
 * 3: a batch of cross blocks (<= 16; dense, 2-bit); 4: a batch of strips (<= 8; dense).  `cols` (n_cols) is the column list the
 * blocks index into; `table` holds `count` rows of 10 int64:
 *   mode 0, 1: {off, nb, dst}                     block = cols[off .. off + nb), nb <= 128, written at out0 + dst
 *   mode 2:    {moff, M, m_pos0, noff, N, n_pos0}  rows cols[moff ..), columns cols[noff ..), entry (m_pos0 + a, n_pos0 + b)
 *   mode 3:    {moff, m, noff, nn, dst}
 *   mode 4:    {voff, m, c0off, c0n, c1off, c1n, row0, dstX, dstD}   row0 + m == c1n; D in out0, the cross block in out1
 * ldc is the leading dimension of every block.  strip_plain != 0 (mode 4): the f64 kernel without the LDS transpose.
 * out0 (out0_elems) and out1 (out1_elems; may be null unless a strip has c0n > 0) are uploaded as the caller filled them and
 * downloaded whole afterwards.  info[10] = {launcher (1 syrk, 2 syrk_batch, 3 gram, 4 gram_batch, 5 strip, 6 csc diagonal
 * blocks, 7 csc gram), K-splits, rows per K-split, tile class (SB; M tiles of the general Gram; MT of a strip), 128-wide and
 * 64-wide N tiles of the general Gram, 1 if the 16-byte-load variant ran, 1 if strip_lt_kernel ran, the general Gram's
 * symmetric flag, row blocks of a compressed-column design}. */
int adelie_hip_block_build_test(adelie_hip_design* d, int mode, int64_t row_off, const void* w, const int32_t* cols, int64_t n_cols,
                                const int64_t* table, int64_t count, const void* xm, int center, int64_t ldc, int strip_plain,
                                void* out0, int64_t out0_elems, void* out1, int64_t out1_elems, int64_t* info);

/* One device piece of the group engine on caller-supplied inputs, through the launcher the solver calls (tests): uploads, launches
 * on the default stream, synchronises, downloads.  No design handle.  Every field is 8 bytes wide; value arrays (`void*`) are in
 * `dtype`, scalars cross as double.  Everything a kernel indexes by is checked against the sizes given here before anything is
 * launched: a bad table is refused with an error string, nothing runs and no output is written.  A block is at most 128 values.
 *
 * mode  ADELIE_HIP_GROUP_EIG: launch_grp_eig over `count` descriptors eig[5 y ..] = {src, vars_pos, v_off, ld, q} (1 <= q <= max_q
 *       <= 96; the block is src[src + r + c ld]); in/out: vars, V (pre-filled by the caller).
 *       ADELIE_HIP_GROUP_ROTATE: launch_grp_block_rotate, D <- R^T Dsrc R on 128 x 128 slots (ld 128); Dsrc null: in place.  `ng`
 *       groups, goff [ng + 1] (goff[0] = 0, increasing, goff[ng] <= 128), rvoff [ng] into V.  in/out: D.  info[1] = 1 if a group
 *       is wider than 16 (the global-scratch route).
 *       ADELIE_HIP_GROUP_LAYOUT: launch_grp_layout for `nblk` blocks of the pass {blk_g0 [nblk + 1], list [n_list] or null (then
 *       positions are screen groups), sbegin / ssize / voff [ns]}; out: desc [nblk * 1168].
 *       ADELIE_HIP_GROUP_PANEL_SOLVE: the layout, then launch_cd_group_panel_solve for j = 0 .. nblk - 1 in order with rot = 1, no
 *       look-ahead, on the caller's rotated blocks Dblk [nblk * 128 * 128] and gradients gblk [nblk * 128]; in/out: beta [nv],
 *       is_active [ns], active_set [ns]; out: desc, dcol / dlt / dd [nblk * 128] (pre-filled by the caller), st_f [nblk * 3] =
 *       {rsq, resid_sum, cm} and st_i [nblk * 4] = {n_updates, active_size, status, nz} after each block.
 *       ADELIE_HIP_GROUP_GRAM_PASS: launch_cd_group_block_pass over the pass on the Gram matrix C (nv x nv, leading dimension
 *       ldc) and gradient g [nv]; in/out: beta, g, is_active, active_set; out: st_f [3], st_i [4] after the pass.
 * The solves read vars / xmean [nv], spen [ns], vcol [nv], V, the penalties l1 / l2 (already multiplied with lambda) and start
 * from the state {rsq, resid_sum, n_updates, active_size}, status 0.  A pass names every screen group at most once.
 * info [2]: info[0] = kernels launched, info[1] as under ROTATE (0 otherwise).
 * The entry is additive and changes the layout of no existing structure: ADELIE_HIP_ABI_VERSION stays as it is. */
enum adelie_hip_group_piece_mode {
    ADELIE_HIP_GROUP_EIG = 0, ADELIE_HIP_GROUP_ROTATE = 1, ADELIE_HIP_GROUP_LAYOUT = 2, ADELIE_HIP_GROUP_PANEL_SOLVE = 3,
    ADELIE_HIP_GROUP_GRAM_PASS = 4
};
typedef struct adelie_hip_group_piece {
    int64_t dtype, mode;
    /* EIG */
    int64_t count, max_q;
    const int64_t* eig;
    const void* src;
    int64_t src_elems;
    /* eigenvalues and eigenbases: in/out of EIG, inputs of the other modes */
    void* vars;
    int64_t vars_elems;
    void* V;
    int64_t V_elems;
    /* ROTATE */
    int64_t ng;
    const int32_t* goff;
    const int64_t* rvoff;
    void* D;
    const void* Dsrc;
    /* LAYOUT and the solves */
    int64_t ns, nv, nblk, n_list;
    const int32_t* sbegin;
    const int32_t* ssize;
    const int64_t* voff;
    const int32_t* blk_g0;
    const int32_t* list;
    int32_t* desc;
    /* the solves */
    const void* Dblk;
    const void* gblk;
    const void* C;
    int64_t ldc;
    const void* xmean;
    const void* spen;
    const int32_t* vcol;
    void* beta;
    void* g;
    int8_t* is_active;
    int32_t* active_set;
    double l1, l2, newton_tol, dbeta_tol;
    int64_t newton_max_iters, max_active_size, mark;
    double rsq, resid_sum;
    int64_t n_updates, active_size;
    int32_t* dcol;
    void* dlt;
    void* dd;
    double* st_f;
    int64_t* st_i;
} adelie_hip_group_piece;
int adelie_hip_group_piece_test(const adelie_hip_group_piece* a, int64_t* info);

/* One launcher of the multi-response kernels (kernels_multi.hip) on caller-supplied inputs, exactly as the solver calls it (tests):
 * uploads, builds the view [1 (x) I_K, X (x) I_K] itself, launches on one stream, synchronises, downloads.  No design handle.
 * Every field is 8 bytes wide; value arrays (`void*`) are in `dtype`, scalars cross as double.  Everything a kernel indexes by is
 * checked against the sizes given here before anything is launched: a bad table is refused with an error string, nothing runs
 * and no output is written.
 *
 * The view (SWEEP, STEP, FUSED_STEP, AXPY): nb rows, pb base columns, K responses, icpt (0 / 1) a leading column of ones.  Dense
 * base: X (X_elems values, pad rows included) is uploaded to a 256-byte aligned allocation at element x_off (0 .. 64); column j
 * starts at element j ld, ld >= nb, (pb - 1) ld + nb <= X_elems.  An ld that is no multiple of the 16-byte vector, or an x_off
 * that breaks 16-byte alignment, selects the scalar-load kernels.  2-bit base (bits != null; X ignored): bits (bits_elems bytes),
 * ldb >= (nb + 3) / 4 bytes per column, (pb - 1) ldb + (nb + 3) / 4 <= bits_elems, impute (pb).  Vectors of nb K values are
 * response-major (element (i, l) at l nb + i); column index c = u K + l is (extended feature u, response l), u < pb + icpt.
 *
 * mode  SWEEP: launch_multi_sweep, out (in/out, (pb + icpt) K) = x_u . v_l; v (nb K) is placed v_off (0 .. 64) elements behind a
 *         256-byte boundary.  info = {variant (0 plain, 1 four waves, 2 staged through LDS), rows per load, responses per chunk,
 *         features per workgroup, feature blocks, row splits, rows per split, response chunks}.
 *       STEP: launch_multi_panel_step.  r (in/out) -= sum_{m < min(nz, 128)} dlt[m] x(dcol[m]) with nz read on the device
 *         (dcol / dlt hold n_dcol >= min(nz, 128) entries); part (in/out, part_elems >= nb_cols * slices, pre-filled by the
 *         caller, comes back whole): part[c * slices + s] = x(cols[c])[slice s] . (w r)[slice s], c < nb_cols <= 256.
 *         info = {slices = leading dimension of part, rows per load}.
 *       FUSED_STEP: launch_multi_panel_fused, the same step (nb_cols <= 128) beside a group solve of one singleton group with
 *         zero gradient and a penalty above it, which changes nothing.  info as STEP (leading dimension = slices rounded up to
 *         whole 16-wave workgroups).
 *       BLOCK_LISTS: launch_multi_block_lists of cols (nv <= 128) -> ulist, slot, resp (in/out, nv each).
 *       EXPAND: launch_multi_expand, D (in/out, D_elems, leading dimension ldd >= nv) from C (C_elems, ldc) through slot / resp
 *         (nv, inputs) for every lsel in lsel_list (n_lsel calls in sequence on the one output).
 *       EXPAND_CROSS: launch_multi_expand_cross, D (nr x nc, ldd >= nr) from C through slot / resp (rows, nr = nv) and slot_c /
 *         resp_c (columns, nc).
 *       AXPY: launch_multi_axpy_cols, r (in/out, nb K) += sign * sum_{m < nz} dlt[m] x(dcol[m]), nz <= n_dcol read on the device.
 *       TO_MAJOR / FROM_MAJOR: launch_multi_{to,from}_major of v (nb K) into out (in/out, nb K).
 *       BATCH_PICK: launch_batch_pick, out (in/out, pb) [u] = v[u K + lsel] - (w ? sign * w[u] : 0); v holds pb K values, w pb.
 * The entry is additive and changes the layout of no existing structure: ADELIE_HIP_ABI_VERSION stays as it is. */
enum adelie_hip_multi_piece_mode {
    ADELIE_HIP_MULTI_SWEEP = 0, ADELIE_HIP_MULTI_STEP = 1, ADELIE_HIP_MULTI_FUSED_STEP = 2, ADELIE_HIP_MULTI_BLOCK_LISTS = 3,
    ADELIE_HIP_MULTI_EXPAND = 4, ADELIE_HIP_MULTI_EXPAND_CROSS = 5, ADELIE_HIP_MULTI_AXPY = 6, ADELIE_HIP_MULTI_TO_MAJOR = 7,
    ADELIE_HIP_MULTI_FROM_MAJOR = 8, ADELIE_HIP_MULTI_BATCH_PICK = 9
};
typedef struct adelie_hip_multi_piece {
    int64_t dtype, mode;
    /* the view */
    int64_t nb, pb, K, icpt;
    const void* X;
    int64_t X_elems, x_off, ld;
    const uint8_t* bits;
    int64_t bits_elems, ldb;
    const void* impute;
    /* vectors */
    const void* v;
    int64_t v_off;
    void* out;
    const void* w;
    void* r;
    /* lists */
    const int32_t* dcol;
    const void* dlt;
    int64_t n_dcol, nz;
    const int32_t* cols;
    int64_t nb_cols;
    void* part;
    int64_t part_elems;
    double sign;
    /* BLOCK_LISTS, EXPAND, EXPAND_CROSS */
    int64_t nv, nc;
    int32_t* ulist;
    int32_t* slot;
    int32_t* resp;
    const int32_t* slot_c;
    const int32_t* resp_c;
    const void* C;
    int64_t C_elems, ldc;
    void* D;
    int64_t D_elems, ldd;
    const int64_t* lsel_list;
    int64_t n_lsel, lsel;
} adelie_hip_multi_piece;
int adelie_hip_multi_piece_test(const adelie_hip_multi_piece* a, int64_t* info);

/* One launcher of kernels_glm.hip -- the elementwise and reduction kernels every IRLS iteration runs -- on caller-supplied inputs
 * (tests): uploads, calls exactly the launch_* the solver calls on one stream, synchronises, downloads.  No design handle is used.
 * Every field is 8 bytes wide; value arrays are of `dtype` (adelie_hip_dtype), index arrays int32, scalars cross as double.  Arrays
 * marked in/out are pre-filled by the caller and come back whole, so an element the launch did not write shows.  `sums` (out, 16
 * values) receives the first 16 elements of the device's reduction scratch, which is allocated as the solver allocates it
 * (16 + 4 * 256 elements) and filled with `sentinel` before the launch: the results of a reduction are sums[0 .. 2], the result of
 * REL_CHANGE is sums[15], as in the solver.  kind is an adelie_hip_glm_kind; with ADELIE_HIP_GLM_MULTINOMIAL the arrays of n
 * values are response-major (nb, K), element (i, k) at [k * nb + i], and n == nb * K is required (w: the observation weights
 * repeated for every class).  A NULL array is accepted only where the launcher does not read it for that kind.  Everything a kernel
 * indexes by is checked before anything is launched; a call that is refused (nonzero return, adelie_hip_last_error) writes nothing.
 * info receives 8 values: {launcher calls made, 0, ...}.
 *   PREPARE: launch_irls_prepare(kind, y, w, eta, resid, off, hmin, n, hess, irls_resid, irls_y, sums, K); hess, irls_resid, irls_y
 *     in/out.  kinds CALLBACK and COX read hess, CALLBACK reads irls_resid; y, w may be NULL for those, resid for CALLBACK.
 *   WEIGHTS: launch_irls_weights(hess, hess_sum, irls_y, shift, n, wts, irls_resid, sums); wts, irls_resid in/out.
 *   FINISH: launch_irls_finish(kind, y, w, irls_y, off, irls_resid, shift, n, eta, resid, sums, K); eta, resid in/out; y, w may be
 *     NULL for CALLBACK and COX.
 *   NULL_STEP: launch_null_step(kind, y, w, eta, resid, off, hmin, n, sums, K, hess, cb_z); hess is required for CALLBACK and COX,
 *     cb_z for CALLBACK (y, w, and for CALLBACK resid, may be NULL then).  K >= 1 for MULTINOMIAL, n is the length of the one
 *     class handed in (the solver calls it class by class).
 *   GRADIENT: launch_glm_gradient(kind, y, w, eta, n, resid, K); resid in/out.   LOSS: launch_glm_loss(kind, y, w, eta, n, sums, K).
 *   LOSS2: launch_glm_loss2(kind, y, w, wb, eta, b0, off, n, sums): eta holds the base.
 *   MULTI_LOSS2: launch_multi_loss2(kind, y, w, wb, eta, b0v, off, nb, K, sums): kind GAUSSIAN (multigaussian) or MULTINOMIAL,
 *     y / eta / off hold n == nb * K values response-major, w / wb nb values, b0v K values.
 *     (GRADIENT, LOSS, LOSS2 take the kinds GAUSSIAN .. BINOMIAL_PROBIT; PREPARE, FINISH, NULL_STEP also CALLBACK and COX.)
 *   SET_ETA: launch_set_eta(off, b0, n, eta); eta in/out.
 *   DOT_DIFF: launch_dot_diff(resid, resid_prev, eta, eta_prev, n, sums).
 *   REL_CHANGE: launch_rel_change(wts, prev, n, sums + 15); prev in/out.
 *   GATHER: launch_gather(src, idx, cnt, dst): dst[a] = src[idx[a]], src holds src_elems, dst (in/out) cnt values.
 *   SCATTER: launch_scatter(src, idx, cnt, dst): dst[idx[a]] = src[a], distinct indices, src holds cnt, dst (in/out) dst_elems
 *     values.  cnt == 0 is allowed in both and leaves dst as it was.
 * The entry is additive and changes the layout of no existing structure: ADELIE_HIP_ABI_VERSION stays as it is. */
enum adelie_hip_glm_piece_mode {
    ADELIE_HIP_GLM_PIECE_PREPARE = 0, ADELIE_HIP_GLM_PIECE_WEIGHTS = 1, ADELIE_HIP_GLM_PIECE_FINISH = 2,
    ADELIE_HIP_GLM_PIECE_NULL_STEP = 3, ADELIE_HIP_GLM_PIECE_GRADIENT = 4, ADELIE_HIP_GLM_PIECE_LOSS = 5,
    ADELIE_HIP_GLM_PIECE_LOSS2 = 6, ADELIE_HIP_GLM_PIECE_MULTI_LOSS2 = 7, ADELIE_HIP_GLM_PIECE_SET_ETA = 8,
    ADELIE_HIP_GLM_PIECE_DOT_DIFF = 9, ADELIE_HIP_GLM_PIECE_REL_CHANGE = 10, ADELIE_HIP_GLM_PIECE_GATHER = 11,
    ADELIE_HIP_GLM_PIECE_SCATTER = 12
};
typedef struct adelie_hip_glm_piece {
    int64_t dtype, mode, kind;
    int64_t n, nb, K;
    double hmin, hess_sum, shift, b0, sentinel;
    const void* y;
    const void* w;
    const void* wb;
    void* eta;
    void* resid;
    const void* off;
    void* hess;
    void* irls_resid;
    void* irls_y;
    void* wts;
    const void* cb_z;
    const void* b0v;
    const void* resid_prev;
    const void* eta_prev;
    void* prev;
    /* GATHER, SCATTER */
    const void* src;
    const int32_t* idx;
    void* dst;
    int64_t cnt, src_elems, dst_elems;
    void* sums;
} adelie_hip_glm_piece;
int adelie_hip_glm_piece_test(const adelie_hip_glm_piece* a, int64_t* info);

/* One of the two places where the path solver touches the covariance matrix A (dense or kept sparse), through exactly the launcher
 * the solver calls (tests): uploads, launches on A's stream, synchronises, downloads.  Column lists must be distinct and in [0, p).
 *   ADELIE_HIP_COV_PIECE_GATHER: the copy of A[S, S] into the screen Gram matrix for the new screen values [pos0, nv) of the
 *     column list vcol (nv), N = nv - pos0, leading dimension ldc >= nv.  A (ldc, nv) buffer is filled with `sentinel`, the gather
 *     for the values [0, pos0) runs as a first step when pos0 > 0, then the step under test; `out` receives the whole buffer.
 *   ADELIE_HIP_COV_PIECE_GRAD: out (p) = v - sum_k coef[k] A[:, cols[k]] over k < count, the count read on the device.
 * Arguments of the other piece are ignored.  This entry and adelie_hip_design_create_cov_csc are additive and change the layout of
 * no existing structure: ADELIE_HIP_ABI_VERSION stays as it is. */
enum adelie_hip_cov_piece { ADELIE_HIP_COV_PIECE_GATHER = 0, ADELIE_HIP_COV_PIECE_GRAD = 1 };
int adelie_hip_cov_piece_test(adelie_hip_design* A, int what, const int32_t* vcol, int64_t nv, int64_t pos0, int64_t N, int64_t ldc,
                              double sentinel, const void* v, const int32_t* cols, const void* coef, int64_t count, void* out);

/* ------------------------------------------------------------------------------------------
 * Full-matrix quadratic programs   min 1/2 x' Q x - v' x + pen(x),   Q a full (d, d) matrix, a batch per call
 *   == adelie.optimization.StateNNQPFull / StateLassoFull / StatePinballFull (...).solve()
 *      (py_optimization.cpp; nnqp_full.hpp:30-99, lasso_full.hpp:29-107, pinball_full.hpp:31-120)
 *   NNQP     pen = indicator of x >= 0                                   visit nnqp_full.hpp:76-92,     thr = d * tol
 *   LASSO    pen = sum_i penalty_a[i] |x_i|                              visit lasso_full.hpp:82-100,   thr = tol
 *   PINBALL  pen = sum_i penalty_b[i] max(x_i, 0) + penalty_a[i] max(-x_i, 0)   (penalty_a = penalty_neg, penalty_b = penalty_pos)
 *                                                                        visit pinball_full.hpp:92-113, thr = y_var * tol
 * Cyclic coordinate descent, the reference's visit restated operation for operation in the value type (no contraction): sweeps
 * over i = 0 .. d-1 until one ends with max_i q_ii del_i^2 < thr (thr formed in the value type), at most max_iters of them.
 * grad must hold v - Q x on entry and does so on exit; a changed visit does grad[a] -= del * Q[a, i] as a multiply and a
 * subtract with Q[., i] the i-th contiguous slice of the buffer (a column of a column-major Q, a row of a row-major one: the
 * reference reads the same slice of either, so both orders are one path and no order is passed).
 *
 * One call solves n_problems independent problems of one kind and dtype (kernels_qp_full.hip): those with d <= 64 in one launch
 * with a wavefront per problem (Q in LDS, the iterate in registers), those with d > 64 in another with a workgroup per problem
 * (Q read from HBM; the per-coordinate state in LDS, or in global memory when it does not fit or from the d that
 * adelie_hip_set_config("qp_full_lds_max_d", d) names -- default 0 = automatic; both forms give the same bits).  There is no
 * reduction and no atomic on the path, so results are bit-reproducible and no problem's result depends on the batch it is in.
 *
 * All per-problem arrays have n_problems entries.  quad[k], penalty_a[k], penalty_b[k], x[k], grad[k] are HOST pointers of
 * `dtype` ((d, d) contiguous; (d,) each), except that quad[k] is a DEVICE pointer on `device` where quad_is_dev[k] != 0: that
 * matrix is read in place and never written.  penalty_a may be NULL for NNQP, penalty_b and y_var unless PINBALL.  x[k] / grad[k]
 * are read and overwritten; iters[k] receives the sweeps run and status[k] an adelie_hip_qp_full_status.  *time_elapsed (may be
 * NULL) receives the wall-clock seconds of the whole call.
 * Returns 0 when every problem was run, whether or not one stopped at max_iters (the statuses say which; x / grad / iters are
 * then those of the last sweep); nonzero with adelie_hip_last_error for malformed arguments (nothing is written then).
 * The entry is additive and changes the layout of no existing structure: ADELIE_HIP_ABI_VERSION stays as it is.
 * ------------------------------------------------------------------------------------------ */
enum adelie_hip_qp_full_kind { ADELIE_HIP_QP_FULL_NNQP = 0, ADELIE_HIP_QP_FULL_LASSO = 1, ADELIE_HIP_QP_FULL_PINBALL = 2 };
enum adelie_hip_qp_full_status { ADELIE_HIP_QP_FULL_OK = 0, ADELIE_HIP_QP_FULL_MAX_ITERS = 1 };
typedef struct adelie_hip_qp_full_args {
    int32_t            kind;         /* adelie_hip_qp_full_kind */
    int32_t            dtype;        /* adelie_hip_dtype */
    int32_t            device;
    int32_t            _pad0;
    int64_t            n_problems;
    const int64_t*     d;
    const void* const* quad;
    const uint8_t*     quad_is_dev;  /* NULL: every quad is a host pointer */
    const void* const* penalty_a;
    const void* const* penalty_b;
    void* const*       x;
    void* const*       grad;
    const double*      tol;
    const double*      y_var;
    const int64_t*     max_iters;
    int64_t*           iters;        /* out */
    int32_t*           status;       /* out */
    double*            time_elapsed; /* out, may be NULL */
} adelie_hip_qp_full_args;
int adelie_hip_qp_full_solve(const adelie_hip_qp_full_args* args);

#ifdef __cplusplus
}
#endif
#endif /* ADELIE_HIP_H */
