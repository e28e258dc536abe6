"""The covariance matrix kept sparse in HBM: matrix.sparse(method="cov", resident="csc") and matrix.block_diag(method="cov",
resident="csc") (reference MatrixCovSparse / MatrixCovBlockDiag).  The members against numpy, the two places the path solver
touches A one launch at a time (adelie_hip_cov_piece_test), paths against the dense route and the CPU oracle, and a matrix whose
dense form does not fit in HBM.  Generators and the oracle's paths: tests/cov_sparse_checks.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import adelie_amd as ad
from adelie_amd import _abi, constraint
import cov_sparse_checks as cc

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def kept_sparse(A, fmt="csc"):
    """The kept-sparse handle of the array A; fmt "csr": from a csr_matrix (with the reference's warning)."""
    if fmt == "csc":
        return ad.matrix.sparse(sp.csc_matrix(A), method="cov", resident="csc")
    with pytest.warns(UserWarning, match="Converting to CSC format."):
        return ad.matrix.sparse(sp.csr_matrix(A), method="cov", resident="csc")


# ---- members ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csc", "csr"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", cc.GRID[:3])
def test_members(hip, case, dtype, fmt):
    """run_cov's list (tests/test_cov.py): to_dense exact, bmul / mul within (k + 1) eps sum |a||b| of float64 numpy."""
    A = cc.problem(case, dtype)[0]
    p = A.shape[0]
    cA = kept_sparse(A, fmt)
    A64, counts = A.astype(np.float64), cc.col_counts(A)
    assert cA.nnz == counts.sum() and isinstance(cA, ad.matrix.MatrixCovBase64 if dtype == np.float64 else ad.matrix.MatrixCovBase32)
    assert cA.rows() == p and cA.cols() == p and cA.shape == (p, p) and cA.ndim == 2 and cA.dtype == dtype
    rng = np.random.RandomState(p)
    v = rng.normal(0, 1, p).astype(dtype).astype(np.float64)
    v[rng.binomial(1, 0.3, p).astype(bool)] = 0
    indices = np.flatnonzero(v) if p > 1 else np.arange(1)
    values = v[indices].astype(dtype)
    bound = cc.dot_bound(np.abs(A64), np.abs(v), counts, dtype)
    ref = v @ A64
    for i in sorted({1, 2, 7, 64, 65, p // 2, p - 1, p} & set(range(1, p + 1))):
        subset = np.sort(rng.choice(p, i, replace=False))
        out = np.empty(i, dtype=dtype)
        cA.bmul(subset, indices, values, out)
        assert np.all(np.abs(out - ref[subset]) <= bound[subset]), np.abs(out - ref[subset]).max()
    out = np.empty(p, dtype=dtype)
    cA.mul(indices, values, out)
    assert np.all(np.abs(out - ref) <= bound), np.abs(out - ref).max()
    cA.mul(indices[:0], values[:0], out)
    assert np.all(out == 0)
    q = min(10, p)
    blk = np.empty((q, q), dtype=dtype, order="F")
    for i in range(p - q + 1):
        cA.to_dense(i, q, blk)
        assert np.array_equal(blk, A[i:i + q, i:i + q])
    full = np.empty((p, p), dtype=dtype, order="F")
    cA.to_dense(0, p, full)
    assert np.array_equal(full, sp.csc_matrix(A).toarray())
    with pytest.raises(RuntimeError, match="bmul"):
        cA.bmul(np.arange(min(2, p)), indices, values, np.empty(3, dtype=dtype))
    with pytest.raises(RuntimeError, match="mul"):
        cA.mul(indices, values, np.empty(p + 1, dtype=dtype))
    with pytest.raises(RuntimeError, match="to_dense"):
        cA.to_dense(p - q + 1, q, blk)


def test_constructor_sums_duplicates_keeps_zeros_and_checks_arguments(hip):
    A = cc.problem(cc.GRID[1])[0]
    S = sp.csc_matrix(A)
    # every entry stored as two halves, the rows of a column in descending and then ascending order, and an explicit zero at
    # (0, 22) and (22, 0), which lie outside the band
    indptr, indices, data = [0], [], []
    for j in range(23):
        idx, val = S.indices[S.indptr[j]:S.indptr[j + 1]], S.data[S.indptr[j]:S.indptr[j + 1]]
        extra = {0: [22], 22: [0]}.get(j, [])
        indices += list(idx[::-1]) + list(idx) + extra
        data += list(val[::-1] / 2) + list(val / 2) + [0.0] * len(extra)
        indptr.append(len(indices))
    D = sp.csc_matrix((np.array(data), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=S.shape)
    assert D.nnz == 2 * S.nnz + 2 and A[0, 22] == 0
    before = (D.indptr.copy(), D.indices.copy(), D.data.copy())
    cD = ad.matrix.sparse(D, method="cov", resident="csc")
    assert all(np.array_equal(a, b) for a, b in zip(before, (D.indptr, D.indices, D.data)))   # the caller's matrix is untouched
    assert cD.nnz == S.nnz + 2 and cD._scipy.has_canonical_format
    out = np.empty(A.shape, order="F")
    cD.to_dense(0, 23, out)
    assert np.array_equal(out, A)
    with pytest.raises(RuntimeError, match=r"mat must be \(p, p\)"):
        ad.matrix.sparse(sp.csc_matrix(np.ones((3, 4))), method="cov", resident="csc")
    with pytest.raises(RuntimeError, match="n_threads must be >= 1"):
        ad.matrix.sparse(S, method="cov", resident="csc", n_threads=0)
    with pytest.raises(RuntimeError, match="float32 or float64"):
        ad.matrix.sparse(sp.csc_matrix(np.eye(3, dtype=np.int64)), method="cov", resident="csc")


# ---- the two device pieces -------------------------------------------------------------------------------------------------
def gather_piece(hip, M, vcol, pos0, ldc):
    vcol = np.ascontiguousarray(vcol, dtype=np.int32)
    nv = len(vcol)
    out = np.empty(ldc * nv, dtype=M.dtype)
    hip.check(hip.fn("cov_piece_test")(M._handle, _abi.COV_PIECE_GATHER, vcol.ctypes.data, nv, pos0, nv - pos0, ldc, SENTINEL,
                                       None, None, None, 0, out.ctypes.data))
    return out.reshape((ldc, nv), order="F")


def grad_piece(hip, M, v, cols, coef):
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    coef = np.ascontiguousarray(coef, dtype=M.dtype)
    v = np.ascontiguousarray(v, dtype=M.dtype)
    out = np.empty(len(v), dtype=M.dtype)
    hip.check(hip.fn("cov_piece_test")(M._handle, _abi.COV_PIECE_GRAD, None, 0, 0, 0, 0, 0.0, v.ctypes.data, cols.ctypes.data,
                                       coef.ctypes.data, len(cols), out.ctypes.data))
    return out


def _piece_matrix(name):
    if name == "lone":
        return cc.lone_diag_matrix()
    if name == "blocks":
        return cc.block_diag_matrix()[0]
    return cc.problem({"p301": cc.GRID[2], "wide": cc.WIDE, "dense": cc.DENSE}[name])[0]


@pytest.fixture(scope="module")
def piece_handles(hip):
    made = {}

    def get(name):
        if name not in made:
            A = _piece_matrix(name)
            made[name] = (A, kept_sparse(A), ad.matrix.dense(A, method="cov"))
        return made[name]
    return get


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("nv,split", [(1, "pos0=0"), (65, "pos0=0"), (65, "pos0>0"), (300, "pos0=0"), (300, "pos0>0")])
@pytest.mark.parametrize("name", ["p301", "wide", "blocks", "dense", "lone"])
def test_gather_piece(hip, piece_handles, name, nv, split, order):
    """The copy of A[S, S] into the screen Gram matrix: equal to the array, equal to the dense handle's result through the same
    entry, and nothing outside the nv x nv square is written."""
    A, cs, cd = piece_handles(name)
    p = A.shape[0]
    nv = min(nv, p)
    rng = np.random.RandomState(nv + p)
    vcol = rng.choice(p, nv, replace=False)
    if name == "lone" and cc.LONE not in vcol:
        vcol[nv // 2] = cc.LONE
    if order == "sorted":
        vcol = np.sort(vcol)
    else:
        assert nv == 1 or np.any(np.diff(vcol) < 0)                        # non-monotone
    pos0 = 0 if split == "pos0=0" else max(1, nv // 3)
    ldc = nv + 7
    got, ref = gather_piece(hip, cs, vcol, pos0, ldc), gather_piece(hip, cd, vcol, pos0, ldc)
    assert np.array_equal(got[:nv], A[np.ix_(vcol, vcol)])
    assert np.array_equal(got[:nv], ref[:nv])
    assert np.all(got[nv:] == SENTINEL) and np.all(ref[nv:] == SENTINEL)
    if name == "lone":
        k = int(np.flatnonzero(vcol == cc.LONE)[0])
        assert got[k, k] == 1.0 and np.count_nonzero(got[:nv, k]) == 1 and np.count_nonzero(got[k, :]) == 1


@pytest.mark.parametrize("count", [0, 1, 200])
@pytest.mark.parametrize("name", ["p301", "wide", "dense", "lone"])
def test_grad_piece(hip, piece_handles, name, count):
    """grad = v - A beta over `count` coefficients: within the bound of float64 numpy, the same bits twice, exactly v at count 0."""
    A, cs, cd = piece_handles(name)
    p = A.shape[0]
    count = min(count, p)
    rng = np.random.RandomState(count + p)
    v = rng.normal(size=p)
    cols = rng.choice(p, count, replace=False)
    coef = rng.normal(size=count)
    w = np.zeros(p)
    w[cols] = coef
    got = grad_piece(hip, cs, v, cols, coef)
    counts = cc.col_counts(A)
    # the dot within (k + 1) eps sum |a||b|, and one more rounding for the subtraction from v
    bound = cc.dot_bound(np.abs(A), np.abs(w), counts, np.float64) + np.finfo(np.float64).eps * (np.abs(v) + np.abs(w @ A))
    assert np.all(np.abs(got - (v - w @ A)) <= bound)
    assert np.array_equal(got, grad_piece(hip, cs, v, cols, coef))
    if count == 0:
        assert np.array_equal(got, v)
    assert np.all(np.abs(grad_piece(hip, cd, v, cols, coef) - got) <= 2 * bound)


def test_piece_entry_checks_its_arguments(hip, piece_handles):
    A, cs, cd = piece_handles("p301")
    for M in (cs, cd):
        with pytest.raises(RuntimeError, match="distinct"):
            gather_piece(hip, M, [3, 3], 0, 4)
        with pytest.raises(RuntimeError, match="distinct"):
            gather_piece(hip, M, [3, 301], 0, 4)
        with pytest.raises(RuntimeError, match="GATHER"):
            gather_piece(hip, M, [3, 4, 5], 0, 2)
        with pytest.raises(RuntimeError, match="distinct"):
            grad_piece(hip, M, np.zeros(301), [-1], [1.0])


# ---- paths -----------------------------------------------------------------------------------------------------------------
def _solve(M, case, dtype, **over):
    return ad.gaussian_cov(M, cc.problem(case, dtype)[1], **dict(cc.path_kwargs(case, dtype), **over))


@pytest.mark.parametrize("case,dtype", [(c, np.float64) for c in cc.GRID] + [(c, np.float32) for c in cc.GRID32])
def test_paths_match_the_dense_route_and_the_oracle(hip, oracle, case, dtype):
    A = cc.problem(case, dtype)[0]
    f64 = dtype == np.float64
    cs = kept_sparse(A)
    a, b, o = _solve(cs, case, dtype), _solve(ad.matrix.dense(A, method="cov"), case, dtype), cc.oracle_path(case, dtype)
    assert a.error == "" and b.error == "" and o.error == ""
    assert len(a.lmdas) == len(b.lmdas) == len(o.lmdas) == 30
    Ba = a.betas.toarray()
    assert np.abs(Ba - b.betas.toarray()).max() < (1e-9 if f64 else 2e-3)
    # the tolerances of tests/test_cov.py::test_hip_cov_matches_oracle
    assert np.abs(Ba - o.betas.toarray()).max() < (1e-7 if f64 else 2e-3)
    np.testing.assert_allclose(a.devs, o.devs, rtol=1e-5 if f64 else 1e-2, atol=1e-9 if f64 else 1e-4)
    assert np.abs(a.grad - o.grad).max() < (1e-9 if f64 else 1e-3)
    again = _solve(cs, case, dtype)
    assert np.array_equal(again.betas.toarray(), Ba) and np.array_equal(again.grad, a.grad)
    assert np.array_equal(again.screen_set, a.screen_set)
    if case in (cc.GRID[3], cc.GROUPED):
        assert cc.screen_values(a, case) >= 256                            # the multi-CU Gram engines ran
    if case == cc.WIDE:
        assert cc.col_counts(A).max() > 256                                # more than one pass of a 64-lane group


def test_path_with_constraints_matches_the_dense_route(hip):
    case = cc.GRID[2]
    A = cc.problem(case)[0]
    p = A.shape[0]
    mk = lambda: [constraint.lower(np.zeros(1)) for _ in range(p)]
    a = _solve(kept_sparse(A), case, np.float64, constraints=mk())
    b = _solve(ad.matrix.dense(A, method="cov"), case, np.float64, constraints=mk())
    assert a.error == "" and b.error == "" and len(a.lmdas) == len(b.lmdas) == 30
    Ba = a.betas.toarray()
    assert np.abs(Ba - b.betas.toarray()).max() < 1e-9
    assert Ba.min() >= -1e-12 and np.count_nonzero(Ba[-1]) > 0


def test_warm_start_continues_the_path(hip):
    """The first 12 lambdas, then the rest from that state, against the full path within 1e-9 (the bound and the form of
    tests/test_cov.py::test_hip_cov_warm_start_errors_and_exit_cond), on the well-conditioned grid case: cond(A) = 1.6e3.

    A continuation screens in another order than the full path did, so the two only agree to the resolution of the stopping
    rule, which grows with the conditioning of A -- whatever the storage.  Measured on an MI355X, max |dbeta| of the continuation
    against the full path at tol = 1e-12, the same figures to every printed digit on the dense and on the kept-sparse handle:
    (60, 23, 5) 4e-16 dense / 0 sparse; (400, 301, 24), cond 1e6: 2.6e-7 (3.0e-9 at tol = 1e-13, 1.1e-9 at 1e-16);
    (900, 700, 90), cond 7e7: 1.8e-6.  On the p = 301 case the check is therefore the one that bears on the storage: the
    continuation on the kept-sparse handle against the continuation on the dense handle."""
    case = cc.GRID[1]
    cs = kept_sparse(cc.problem(case)[0])
    full = _solve(cs, case, np.float64)
    half = _solve(cs, case, np.float64, lmda_path=full.lmdas[:12])
    rest = _solve(cs, case, np.float64, lmda_path=full.lmdas[12:], warm_start=half, check_state=True)
    assert half.error == "" and rest.error == "" and len(rest.lmdas) == 18
    assert np.array_equal(half.betas.toarray(), full.betas[:12].toarray())
    assert np.abs(rest.betas.toarray() - full.betas[12:].toarray()).max() < 1e-9
    case = cc.GRID[2]
    A = cc.problem(case)[0]
    conts = []
    for M in (kept_sparse(A), ad.matrix.dense(A, method="cov")):
        full = _solve(M, case, np.float64)
        half = _solve(M, case, np.float64, lmda_path=full.lmdas[:12])
        conts.append(_solve(M, case, np.float64, lmda_path=full.lmdas[12:], warm_start=half, check_state=True))
        assert conts[-1].error == "" and len(conts[-1].lmdas) == 18
    assert np.abs(conts[0].betas.toarray() - conts[1].betas.toarray()).max() < 1e-9
    assert np.array_equal(conts[0].screen_set, conts[1].screen_set)


# ---- block_diag ------------------------------------------------------------------------------------------------------------
def test_block_diag_kept_sparse(hip):
    blocks = cc.block_diag_blocks()
    ref, v = cc.block_diag_matrix()
    p = ref.shape[0]
    mk = lambda: [blocks[0], ad.matrix.dense(blocks[1], method="cov"), kept_sparse(blocks[2]), blocks[3]]
    A = ad.matrix.block_diag(mk(), method="cov", resident="csc")
    assert isinstance(A, ad.matrix.MatrixCovBase64) and A.shape == (p, p)
    assert A.nnz == sum(q * q for q in cc.BLOCKS)
    out = np.empty((p, p), order="F")
    A.to_dense(0, p, out)
    assert np.array_equal(out, ref)
    D = ad.matrix.block_diag(mk(), method="cov")
    assert not hasattr(D, "nnz")
    D.to_dense(0, p, out)
    assert np.array_equal(out, ref)
    kw = dict(lmda_path_size=30, min_ratio=0.05, tol=1e-12, early_exit=False, progress_bar=False)
    a, b = ad.gaussian_cov(A, v, **kw), ad.gaussian_cov(D, v, **kw)
    assert a.error == "" and b.error == "" and len(a.lmdas) == len(b.lmdas) == 30
    assert np.abs(a.betas.toarray() - b.betas.toarray()).max() < 1e-9
    with pytest.raises(ValueError, match="resident"):
        ad.matrix.block_diag(list(blocks), method="cov", resident="tile")


# ---- beyond what a dense matrix can hold -------------------------------------------------------------------------------------
def test_a_matrix_whose_dense_form_does_not_fit(hip):
    """p = 250 000, bandwidth 8: 500 GB dense in f64, 51 MB kept sparse.  KKT on the host with scipy from v - A beta."""
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
    assert cA.shape == (p, p) and cA.nnz == A.nnz == p * (2 * bw + 1) - bw * (bw + 1)
    st = ad.gaussian_cov(cA, v, lmda_path_size=10, min_ratio=0.5, tol=1e-12, early_exit=False, progress_bar=False)
    assert st.error == "" and len(st.lmdas) == 10
    B = st.betas.tocsr()
    assert B[-1].nnz > 0
    for l, lm in enumerate(st.lmdas):
        b = np.asarray(B[l].todense()).ravel()
        grad = v - A @ b
        act = b != 0
        assert np.all(np.abs(grad[~act]) <= lm * (1 + 1e-6))               # penalty 1, alpha 1
        assert np.abs(grad[act] - lm * np.sign(b[act])).max(initial=0.0) < 1e-6
    assert np.abs(st.grad - (v - A @ np.asarray(B[-1].todense()).ravel())).max() < 1e-9


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    A, v = cc.problem(cc.GRID[1])
    cs = kept_sparse(A)
    with pytest.raises(RuntimeError, match='resident="dense"'):
        ad.css_cov(cs, 3, method="greedy")
    with pytest.raises(RuntimeError):
        ad.grpnet(cs, ad.glm.gaussian(v), progress_bar=False)
    with pytest.raises(RuntimeError):
        ad.bvls(cs, v, np.full(23, -1.0), np.full(23, 1.0))
    with pytest.raises(RuntimeError):
        ad.matrix.standardize(cs)
    with pytest.raises(RuntimeError):
        ad.matrix.subset(cs, np.arange(3), axis=1)
    with pytest.raises(RuntimeError):
        ad.matrix.concatenate([cs, cs], axis=1)
    # the native entry points refuse the handle themselves: the row arrays they would read do not exist
    zeros, ones, mask = np.zeros(23), np.ones(23), np.ones((23, 1), dtype=np.uint8)
    fns = {
        "alias": lambda out: hip.fn("design_alias")(cs._handle, out),
        "standardize": lambda out: hip.fn("design_create_standardized")(cs._handle, zeros.ctypes.data, ones.ctypes.data, out),
        "subset": lambda out: hip.fn("design_create_derived")(cs._handle, None, 0, None, 0, None, None, out),
        "relu": lambda out: hip.fn("design_create_convex_relu_csc")(cs._handle, mask.ctypes.data, 1, 1, out),
    }
    for name, f in fns.items():
        out = _abi.C.c_void_p()
        assert f(out) != 0 and not out.value, name
    ptr = np.empty(24, dtype=np.int64)
    assert hip.fn("design_csc_download")(cs._handle, ptr.ctypes.data, None, None, None, None, None) == 0
    assert np.array_equal(ptr, sp.csc_matrix(A).indptr)
    assert hip.fn("design_csc_download")(cs._handle, None, None, None, ptr.ctypes.data, None, None) != 0
    with pytest.raises(ValueError, match="resident"):
        ad.matrix.sparse(sp.csc_matrix(A), method="cov", resident="tile")
    # "auto" and "dense" are the dense handle, as before
    for r in ("auto", "dense"):
        assert not hasattr(ad.matrix.sparse(sp.csc_matrix(A), method="cov", resident=r), "nnz")
