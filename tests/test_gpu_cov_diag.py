"""diagnostic.DiagnosticCov and the lambda-batched covariance product under it (A.mul_batch, adelie_hip_design_cov_mul_batch):
out[l] = v - A beta_l for the rows of a CSR matrix, on dense storage (F- and C-ordered arrays, lazy_cov, block_diag) and on
matrices kept sparse.  Bit equality with one A.mul per row, the product against float64 numpy within a derived bound, KKT of a
solved path at p = 250 000 through the diagnostic object, and the refusals."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import adelie_amd as ad
from adelie_amd import constraint

pytestmark = pytest.mark.gpu

LB = 8                                  # rows per batch (cov_batch_host.hpp)
LS = [1, LB - 1, LB, LB + 1, 2 * LB + 1]
PS = [1, 37, 300]
DENSE = ["F", "C", "lazy", "block_diag"]
SPARSE = ["band", "long4", "long16", "block_diag_csc"]
DTYPES = [np.float64, np.float32]


def symmetric(p, dtype, seed, density=1.0, half_width=None):
    rng = np.random.RandomState(seed)
    M = rng.normal(size=(p, p)) * (rng.uniform(size=(p, p)) < density)
    A = M + M.T
    if half_width is not None:
        i, j = np.indices((p, p))
        A[np.abs(i - j) > half_width] = 0
    return np.asfortranarray(A.astype(dtype))


def blocks_of(p, dtype):
    sizes = {1: [1], 37: [3, 17, 17], 300: [40, 70, 190]}[p]
    return [symmetric(q, dtype, 100 + q + k) for k, q in enumerate(sizes)]


def lanes_of(S):
    """cov_csc_lanes (cov_csc_host.hpp) of the stored form"""
    mean = -(-S.nnz // S.shape[0])
    return 4 if mean <= 8 else (16 if mean <= 64 else 64)


def kept(S):
    return ad.matrix.sparse(S, method="cov", resident="csc")


def build(storage, p, dtype):
    """(the matrix as a host array of the handle's dtype, the handle)"""
    if storage == "F":
        A = symmetric(p, dtype, p)
        return A, ad.matrix.dense(A, method="cov")
    if storage == "C":
        A = np.ascontiguousarray(symmetric(p, dtype, p + 1))
        assert p == 1 or not A.flags.f_contiguous
        return A, ad.matrix.dense(A, method="cov")
    if storage == "lazy":
        X = np.asfortranarray(np.random.RandomState(p + 2).normal(size=(p + 4, p)).astype(dtype))
        M = ad.matrix.lazy_cov(X)
        A = np.empty((p, p), dtype=dtype, order="F")
        M.to_dense(0, p, A)                                                # the matrix the device formed
        return A, M
    if storage == "block_diag":
        blocks = blocks_of(p, dtype)
        return scipy.linalg.block_diag(*blocks).astype(dtype), ad.matrix.block_diag(blocks, method="cov")
    if storage == "block_diag_csc":
        blocks = blocks_of(p, dtype)
        return scipy.linalg.block_diag(*blocks).astype(dtype), ad.matrix.block_diag(blocks, method="cov", resident="csc")
    if storage == "band":            # columns without a stored entry and explicit stored zeros
        A = symmetric(p, dtype, p + 3, half_width=3)
        if p > 3:
            for j in (2, p - 1):
                A[j, :] = 0
                A[:, j] = 0
        S = sp.csc_matrix(A)
        if p > 3:
            assert np.any(np.diff(S.indptr) == 0)
            cols = np.repeat(np.arange(p), np.diff(S.indptr))
            S.data[(S.indices + cols) % 5 == 0] = 0                        # (i, j) and (j, i) together: still symmetric
            assert np.count_nonzero(S.data == 0) > 0
        M = kept(S)
        assert M.nnz == S.nnz                                              # the zeros stay stored
        return np.asfortranarray(S.toarray()), M
    if storage in ("long4", "long16"):  # one full column (and row) in a matrix whose mean count picks 4 resp. 16 lanes
        A = symmetric(p, dtype, p + 4, half_width=1 if storage == "long4" else 8)
        full = symmetric(p, dtype, p + 5)
        A[:, 0] = full[:, 0]
        A[0, :] = full[:, 0]
        S = sp.csc_matrix(A)
        if p == 300:
            lanes = lanes_of(S)
            assert lanes == (4 if storage == "long4" else 16)
            assert np.diff(S.indptr).max() > 8 * lanes                     # more than one trip of the lane group
        return A, kept(S)
    if storage == "full600":         # a whole wavefront per column and more than 8 x 64 entries in every column
        A = symmetric(p, dtype, p + 6)
        S = sp.csc_matrix(A)
        assert lanes_of(S) == 64 and np.diff(S.indptr).min() > 8 * 64
        return A, kept(S)
    raise AssertionError(storage)


@pytest.fixture(scope="module")
def handles(hip):
    made = {}

    def get(storage, p, dtype):
        key = (storage, p, np.dtype(dtype).name)
        if key not in made:
            made[key] = build(storage, p, dtype)
        return made[key]
    return get


def rows_of(L, p, dtype, seed):
    """(L, p) CSR in dtype: rows of about a fifth of the columns; from two rows on, the middle row is empty and the last is full."""
    rng = np.random.RandomState(seed)
    D = (rng.normal(size=(L, p)) * (rng.uniform(size=(L, p)) < 0.2)).astype(dtype)
    if L >= 2:
        D[L // 2] = 0
        D[-1] = rng.normal(size=p).astype(dtype) + dtype(4)                # no zero among them
    return sp.csr_matrix(D)


def single(M, row, v):
    """v - A.mul(row), the subtraction in the handle's dtype; A.mul alone without v"""
    out = np.empty(M.cols(), dtype=M.dtype)
    M.mul(row.indices, row.data, out)
    return out if v is None else v - out


CASES = [(s, p) for s in DENSE + SPARSE for p in PS] + [("full600", 600)]


# ---- 1. the object exists ----------------------------------------------------------------------------------------------------
def small_problem():
    rng = np.random.RandomState(5)
    X = rng.normal(size=(100, 60))
    beta = np.zeros(60)
    beta[rng.choice(60, 8, replace=False)] = rng.normal(size=8) * 2
    y = X @ beta + 0.1 * rng.normal(size=100)
    return np.asfortranarray(X.T @ X / 100), X.T @ y / 100


@pytest.mark.parametrize("resident", ["dense", "csc"])
def test_diagnostic_returns_a_diagnostic_cov(hip, resident):
    A, v = small_problem()
    M = ad.matrix.dense(A, method="cov") if resident == "dense" else kept(sp.csc_matrix(A))
    st = ad.gaussian_cov(M, v, lmda_path_size=12, min_ratio=0.05, tol=1e-12, early_exit=False, progress_bar=False)
    assert st.error == "" and len(st.lmdas) == 12
    d = ad.diagnostic.diagnostic(st)
    assert isinstance(d, ad.diagnostic.DiagnosticCov)
    assert d.gradients.shape == (12, 60) and d.gradients.dtype == np.float64
    assert d.state is st and d.betas is st.betas and d.duals is st.duals
    assert d._args["constraints"] is None and d._args["groups"] is st.groups and d._args["penalty"] is st.penalty
    assert d.gradient_norms.shape == (12, 60) and d.gradient_scores.shape == (12, 60)
    B = st.betas.toarray()
    assert np.abs(d.gradients - (v[None] - B @ A)).max() < 1e-12
    assert np.abs(d.gradients[-1] - st.grad).max() < 1e-9
    assert np.all(d.gradient_scores[B == 0] <= np.repeat(st.lmdas[:, None], 60, axis=1)[B == 0] * (1 + 1e-6))


def test_diagnostic_still_returns_a_diagnostic_naive(hip):
    rng = np.random.RandomState(6)
    X = np.asfortranarray(rng.normal(size=(50, 10)))
    st = ad.grpnet(X, ad.glm.gaussian(X[:, 0] + 0.1 * rng.normal(size=50)), lmda_path_size=5, progress_bar=False)
    assert type(ad.diagnostic.diagnostic(st)) is ad.diagnostic.DiagnosticNaive


def test_fallback_loop_gives_the_same_bits(hip, monkeypatch):
    """Against a library without the entry DiagnosticCov multiplies once per lambda: the same gradients, bit for bit."""
    A, v = small_problem()
    st = ad.gaussian_cov(kept(sp.csc_matrix(A)), v, lmda_path_size=12, min_ratio=0.05, tol=1e-12, early_exit=False, progress_bar=False)
    batched = ad.diagnostic.DiagnosticCov(st)
    has = type(hip).has
    monkeypatch.setattr(type(hip), "has", lambda self, name: name != "design_cov_mul_batch" and has(self, name))
    looped = ad.diagnostic.DiagnosticCov(st)
    assert np.array_equal(looped.gradients, batched.gradients)
    assert np.array_equal(looped.gradient_scores, batched.gradient_scores)


# ---- 2. bit equality with the single-vector entry -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("storage,p", CASES)
def test_rows_have_the_bits_of_single_products(hip, handles, storage, p, dtype):
    A, M = handles(storage, p, dtype)
    assert np.all(np.isfinite(A))
    v = np.random.RandomState(p).normal(size=p).astype(dtype)
    for L in LS:
        B = rows_of(L, p, dtype, seed=L + p)
        out = M.mul_batch(B, v)
        assert out.shape == (L, p) and out.dtype == dtype and out.flags.c_contiguous
        for l in range(L):
            assert np.array_equal(out[l], single(M, B[l], v)), (L, l)
        if L >= 2:
            assert B[L // 2].nnz == 0 and np.array_equal(out[L // 2], v)   # a row without entries: v exactly
            assert B[L - 1].nnz == p                                       # a full row
        if p > 1 and L >= LB:
            first = B[:LB]
            assert len(np.unique(first.indices)) > LB                      # the batch's union exceeds its rows
    # v = None: the product alone; dense (L, p) input
    B = rows_of(LB + 1, p, dtype, seed=3)
    out = M.mul_batch(B)
    for l in range(LB + 1):
        assert np.array_equal(out[l], single(M, B[l], None))
    assert np.array_equal(M.mul_batch(B.toarray()), out)
    buf = np.full((LB + 1, p), 7, dtype=dtype)
    assert M.mul_batch(B, out=buf) is buf and np.array_equal(buf, out)     # into the caller's array
    # a row does not depend on the rows that share its batch: alone, first of a full batch, last of a full batch
    others = rows_of(LB - 1, p, dtype, seed=4)
    for row in (B[0], B[LB]):                                              # an ordinary row and the full one
        alone = M.mul_batch(row, v)[0]
        assert np.array_equal(M.mul_batch(sp.vstack([row, others]).tocsr(), v)[0], alone)
        assert np.array_equal(M.mul_batch(sp.vstack([others, row]).tocsr(), v)[LB - 1], alone)
        assert np.array_equal(alone, single(M, row, v))


def test_unsorted_and_duplicated_csr_input_is_made_canonical(hip, handles):
    A, M = handles("F", 37, np.float64)
    v = np.arange(37, dtype=np.float64)
    # row 0: indices descending with a duplicate; row 1: empty; row 2: one entry
    B = sp.csr_matrix((np.array([1.0, 2.0, 0.5, 3.0]), np.array([9, 4, 9, 36]), np.array([0, 3, 3, 4])), shape=(3, 37))
    before = (B.indptr.copy(), B.indices.copy(), B.data.copy())
    out = M.mul_batch(B, v)
    assert all(np.array_equal(a, b) for a, b in zip(before, (B.indptr, B.indices, B.data)))   # the caller's matrix is untouched
    C = sp.csr_matrix(B.toarray())
    for l in range(3):
        assert np.array_equal(out[l], single(M, C[l], v))


# ---- 3. against numpy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("storage,p", CASES)
def test_product_against_float64_numpy(hip, handles, storage, p, dtype):
    """|out[l, j] - (v - A beta_l)[j]| <= (k_l + 2) eps ((|A| |beta_l|)[j] + |v[j]|), k_l = nnz(beta_l): a sum of k_l non-zero
    products in any order is within k_l eps / 2 of sum |a||b| to first order, the subtraction rounds once more."""
    A, M = handles(storage, p, dtype)
    A64 = A.astype(np.float64)
    v = np.random.RandomState(p + 1).normal(size=p).astype(dtype)
    eps = np.finfo(dtype).eps
    L = 2 * LB + 1
    B = rows_of(L, p, dtype, seed=p + 9)
    out = M.mul_batch(B, v).astype(np.float64)
    D = B.toarray().astype(np.float64)
    ref = v.astype(np.float64)[None] - D @ A64.T
    k = np.diff(B.indptr)
    bound = (k[:, None] + 2) * eps * (np.abs(D) @ np.abs(A64).T + np.abs(v.astype(np.float64))[None])
    err = np.abs(out - ref)
    assert np.all(err <= bound), (err - bound).max()


# ---- 4. KKT on a solved path ---------------------------------------------------------------------------------------------------
def test_kkt_of_a_matrix_whose_dense_form_does_not_fit(hip):
    """The banded p = 250 000 problem of tests/test_gpu_cov_sparse.py with its solve arguments and bounds, checked through the
    diagnostic object instead of scipy on the host."""
    p, bw = 250_000, 8
    rng = np.random.RandomState(11)
    offs = [rng.uniform(-1, 1, p - k) for k in range(1, bw + 1)]
    diag = np.ones(p)
    for k, o in enumerate(offs, start=1):                                 # diagonally dominant: positive definite
        diag[:-k] += np.abs(o)
        diag[k:] += np.abs(o)
    A = sp.diags([diag] + offs + offs, [0] + list(range(1, bw + 1)) + [-k for k in range(1, bw + 1)], format="csc")
    beta = np.zeros(p)
    beta[rng.choice(p, 40, replace=False)] = rng.choice([-1.0, 1.0], 40) * rng.uniform(1, 2, 40)
    v = A @ beta + 0.01 * rng.normal(size=p)
    cA = ad.matrix.sparse(A, method="cov", resident="csc")
    st = ad.gaussian_cov(cA, v, lmda_path_size=10, min_ratio=0.5, tol=1e-12, early_exit=False, progress_bar=False)
    assert st.error == "" and len(st.lmdas) == 10
    d = ad.diagnostic.diagnostic(st)
    assert isinstance(d, ad.diagnostic.DiagnosticCov) and d.gradients.shape == (10, p)
    B = st.betas.tocsr()
    assert B[-1].nnz > 0
    for l, lm in enumerate(st.lmdas):
        b = np.asarray(B[l].todense()).ravel()
        act = b != 0
        assert np.all(d.gradient_scores[l][~act] <= lm * (1 + 1e-6))       # penalty 1, alpha 1: the score is |grad|
        assert np.abs(d.gradients[l][act] - lm * np.sign(b[act])).max(initial=0.0) < 1e-6
    assert np.abs(d.gradients[-1] - st.grad).max() < 1e-9


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(hip, handles):
    A, M = handles("band", 37, np.float64)
    v = np.ones(37)
    B = rows_of(3, 37, np.float64, seed=1)
    indptr, indices, values = B.indptr.astype(np.int64), B.indices.astype(np.int64), B.data.copy()
    out = np.empty((3, 37))
    # a naive design's handle through the raw entry
    X = ad.matrix.dense(np.asfortranarray(np.ones((37, 37))))
    with pytest.raises(RuntimeError, match="covariance matrix"):
        hip.check(hip.fn("design_cov_mul_batch")(X._handle, 3, indptr.ctypes.data, indices.ctypes.data, values.ctypes.data, None,
                                                 out.ctypes.data))
    # L == 0 is a no-op, whatever the other arguments are
    hip.check(hip.fn("design_cov_mul_batch")(M._handle, 0, None, None, None, None, None))
    assert M.mul_batch(sp.csr_matrix((0, 37)), v).shape == (0, 37)
    # an index equal to p: refused on the host, nothing allocated or launched, and the handle works as before
    M.mul_batch(B, v)
    owned = hip.fn("design_owned_bytes")()
    bad = B.copy()
    bad.indices[bad.indptr[1] - 1] = 37                                    # the last entry of row 0, still ascending
    with pytest.raises(RuntimeError, match="column index out of range"):
        M.mul_batch(bad, v)
    assert hip.fn("design_owned_bytes")() == owned
    ref = np.asarray(B[0].todense()).ravel() @ A
    got = np.empty(37)
    M.mul(B[0].indices, B[0].data, got)
    assert np.abs(got - ref).max() < 1e-12
    # descending indices through the raw entry (mul_batch itself sorts a CSR operand first)
    swapped = indices.copy()
    assert indptr[1] >= 2
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(RuntimeError, match="ascending"):
        hip.check(hip.fn("design_cov_mul_batch")(M._handle, 3, indptr.ctypes.data, swapped.ctypes.data, values.ctypes.data, None,
                                                 out.ctypes.data))
    # shapes and types, in mul's style
    with pytest.raises(RuntimeError, match="mul_batch\\(\\) is given inconsistent inputs"):
        M.mul_batch(sp.csr_matrix((2, 36)), v)
    with pytest.raises(RuntimeError, match="mul_batch\\(\\) is given inconsistent inputs"):
        M.mul_batch(B, np.ones(36))
    with pytest.raises(RuntimeError, match="mul_batch\\(\\) is given inconsistent inputs"):
        M.mul_batch(B, v, out=np.empty((3, 37), order="F"))
    with pytest.raises(RuntimeError, match="mul_batch\\(\\) is given inconsistent inputs"):
        M.mul_batch(B, v, out=np.empty((3, 37), dtype=np.float32))
    with pytest.raises(RuntimeError, match="float32 or float64"):
        M.mul_batch(sp.csr_matrix(np.eye(37, dtype=np.int64)), v)
    with pytest.raises(RuntimeError, match="np.ndarray or scipy.sparse.csr_matrix"):
        M.mul_batch(B.tocsc(), v)


def test_a_constrained_state_reaches_gradient_norms_refusal(hip):
    A, v = small_problem()
    cons = [constraint.lower(np.zeros(1)) for _ in range(60)]
    st = ad.gaussian_cov(ad.matrix.dense(A, method="cov"), v, constraints=cons, lmda_path_size=12, min_ratio=0.05, tol=1e-12,
                         early_exit=False, progress_bar=False)
    assert st.error == ""
    with pytest.raises(NotImplementedError, match="constraints"):
        ad.diagnostic.DiagnosticCov(st)
    with pytest.raises(NotImplementedError, match="constraints"):
        ad.diagnostic.diagnostic(st)
