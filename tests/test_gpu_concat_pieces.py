"""``matrix.concatenate(..., axis=1, resident="pieces")``: column blocks of dense and 2-bit designs kept as they are
(``adelie_hip_design_create_pieces``; the reference's ``matrix_naive_concatenate.ipp`` keeps its pieces too).

The pieces are ``[dense 3, snp 7, dense 2, snp 5]`` columns with about 5 % missing calls.  The matrix operations are checked
against numpy on the concatenated array, the solves against ``concatenate`` of the same pieces under the default ``resident``
(one dense copy, panel engines), with the bounds ``test_gpu_sparse.py`` uses for a design kept sparse against its dense copy."""
import gc

import numpy as np
import pytest
import scipy.sparse as sp

import adelie_amd as ad
from adelie_amd import _abi
from matrix_checks import run_naive

pytestmark = pytest.mark.gpu

SIZES = [3, 7, 2, 5]
KINDS = ["dense", "snp", "dense", "snp"]
FIRST = [0, 3, 10, 12]
P = 17
# first and last column of every piece
EDGES = [0, 2, 3, 9, 10, 11, 12, 16]


def owned(hip):
    gc.collect()
    return int(hip.fn("design_owned_bytes")())


def _calls(rng, n, p):
    return rng.choice(np.array([0, 1, 2, -9], dtype=np.int8), size=(n, p), p=[0.55, 0.28, 0.12, 0.05])


def _decoded(calls, dtype):
    return np.where(calls < 0, ad.matrix.compute_impute(calls)[None], calls).astype(dtype)


def _pieces(n, dtype, scalar=False, seed=21):
    """The four pieces and the numpy concatenation.  ``scalar``: the first dense piece is columns 1..3 of an adopted tensor that
    starts one element behind a 16-byte boundary, so its base is misaligned whatever n is (and its leading dimension n is odd
    at n = 203 and 9001): ``dense_vec_ok`` is false for it and the whole pieces design takes the scalar kernels."""
    rng = np.random.RandomState(seed + n % 97)
    A = np.asfortranarray(rng.normal(size=(n, 3)).astype(dtype))
    C = np.asfortranarray(rng.normal(size=(n, 2)).astype(dtype))
    c1, c2 = _calls(rng, n, 7), _calls(rng, n, 5)
    if scalar:
        import torch

        W = np.asfortranarray(np.concatenate([rng.normal(size=(n, 1)), A, rng.normal(size=(n, 1))], axis=1).astype(dtype))
        buf = torch.empty(n * 5 + 1, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
        t = buf[1:].view(5, n).t()
        t.copy_(torch.from_numpy(W))
        assert t.stride() == (1, n) and t.data_ptr() % 16 != 0
        base = ad.matrix.dense(t)
        D1 = ad.matrix.subset(base, np.arange(1, 4), axis=1)
        assert D1._slice_of is base and D1._kind == "dense"
    else:
        D1 = ad.matrix.dense(A)
    mats = [D1, ad.matrix.snp_calldata(c1, dtype=dtype), ad.matrix.dense(C), ad.matrix.snp_calldata(c2, dtype=dtype)]
    Xnp = np.asfortranarray(np.concatenate([A, _decoded(c1, dtype), C, _decoded(c2, dtype)], axis=1))
    return mats, Xnp


def _pieces_design(n, dtype, scalar=False, seed=21):
    mats, Xnp = _pieces(n, dtype, scalar, seed)
    X = ad.matrix.concatenate(mats, axis=1, resident="pieces")
    assert X._kind == "pieces" and X.pieces == list(zip(FIRST, KINDS)) and X.shape == Xnp.shape
    return X, mats, Xnp


def _tol(Xnp, dtype):
    """run_naive's own bound for one entry of an operation (matrix_checks.py)."""
    n = Xnp.shape[0]
    if dtype == np.float64:
        return 1e-12 * max(1.0, np.abs(Xnp).max()) * n
    return 1e-4 * max(1.0, np.abs(Xnp).max()) * np.sqrt(n) * 10


# n = 203: a row tail (n % 4 != 0); 256: whole vectors; 9001: several row splits of the sweeps (sweep_shape splits above 2048
# rows in f64 and 4096 in f32)
@pytest.mark.parametrize("scalar", [False, True], ids=["vec", "scalar"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [203, 256, 9001])
def test_pieces_design_runs_the_reference_check_list(hip, n, dtype, scalar):
    """1 and 2: run_naive (its cov and bmul blocks straddle piece boundaries: (0, 17), (8, 9), (14, 3), (5, 4)) and mul_batch."""
    X, mats, Xnp = _pieces_design(n, dtype, scalar)
    run_naive(X, Xnp, dtype)
    rng = np.random.RandomState(3)
    V = rng.normal(size=(11, n)).astype(dtype)   # eight vectors and three: both legs of the batched route
    out = X.mul_batch(V)
    assert np.abs(out - V.astype(np.float64) @ Xnp.astype(np.float64)).max() <= _tol(Xnp, dtype)
    out1 = X.mul_batch(V[:1])
    assert np.array_equal(out1[0], out[0])


@pytest.mark.parametrize("scalar", [False, True], ids=["vec", "scalar"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [203, 9001])
def test_single_columns_and_column_lists_at_every_piece_edge(hip, n, dtype, scalar):
    """3: cmul and ctmul at the first and last column of every piece; bmul / btmul over an explicit unsorted column list with a
    repeated column (the sweep and axpy kernels that resolve every column's piece themselves), and the same list through
    sp_tmul."""
    X, mats, Xnp = _pieces_design(n, dtype, scalar)
    X64 = Xnp.astype(np.float64)
    tol = _tol(Xnp, dtype)
    rng = np.random.RandomState(5)
    v = rng.normal(size=n).astype(dtype)
    w = rng.uniform(0, 1, n).astype(dtype)
    vw = v.astype(np.float64) * w
    for j in EDGES:
        assert abs(X.cmul(j, v, w) - X64[:, j] @ vw) <= tol
        out = rng.normal(size=n).astype(dtype)
        ref = out + (-0.81) * X64[:, j]
        X.ctmul(j, -0.81, out)
        assert np.abs(out - ref).max() <= tol
    cols = np.array([16, 3, 0, 10, 9, 3, 12, 2, 11, 16], dtype=np.int64)   # every edge, unsorted, 3 and 16 twice
    assert set(cols) == set(EDGES)
    out = np.empty(cols.size, dtype=dtype)
    X.bmul_cols(cols, v, w, out)
    assert np.abs(out - vw @ X64[:, cols]).max() <= tol
    # a column's value does not depend on the route: the list sweep and the piece's own sweep read the same rows in one order
    single = np.array([X.cmul(int(j), v, w) for j in cols], dtype=dtype)
    assert np.abs(out - single).max() <= tol
    c = rng.normal(size=cols.size).astype(dtype)
    o = rng.normal(size=n).astype(dtype)
    ref = o + X64[:, cols] @ c
    X.btmul_cols(cols, c, o)
    assert np.abs(o - ref).max() <= tol
    V = sp.csr_matrix((c.astype(np.float64), cols, np.array([0, cols.size])), shape=(1, P))   # unsorted, with the repeats
    o2 = np.empty((1, n), dtype=dtype)
    X.sp_tmul(V, o2)
    assert np.abs(o2[0] - X64[:, cols] @ c).max() <= tol


def _problem(n, seed=31):
    mats, Xnp = _pieces(n, np.float64, False, seed)
    rng = np.random.RandomState(seed)
    eta = Xnp[:, [1, 5, 11, 14]] @ np.array([1.0, -1.2, 0.8, 0.6])
    return mats, Xnp, eta, rng


KW = dict(tol=1e-12, early_exit=False, lmda_path_size=12, min_ratio=0.05, progress_bar=False)


def _both(mats, glm, **kw):
    a = ad.grpnet(ad.matrix.concatenate(mats, axis=1, resident="pieces"), glm, **kw)
    D = ad.matrix.concatenate(mats, axis=1)
    assert D._kind == "dense"
    b = ad.grpnet(D, glm, **kw)
    assert a.error == "" and b.error == ""
    assert len(a.lmdas) == len(b.lmdas) and np.allclose(a.lmdas, b.lmdas, rtol=1e-12)
    db = np.abs(a.betas.toarray() - b.betas.toarray()).max()
    di = np.abs(np.asarray(a.intercepts) - np.asarray(b.intercepts)).max()
    print("max|dbeta|", db, "max|dintercept|", di)
    return a, b, db, di


@pytest.mark.parametrize("case", ["lasso", "groups3", "pen0_dense", "lasso_n9001"])
def test_gaussian_paths_on_pieces_match_the_dense_copy(hip, case):
    """4: max|dbeta| < 1e-9, intercepts alike (the bound of test_gpu_sparse.py for a design kept sparse against its dense copy)."""
    n = 9001 if case == "lasso_n9001" else 300
    mats, Xnp, eta, rng = _problem(n)
    y = eta + 0.3 * rng.normal(size=n)
    kw = dict(KW)
    if case == "groups3":   # [2, 5) straddles the boundary at 3, [8, 11) the one at 10, [11, 14) the one at 12
        kw.update(groups=np.array([0, 2, 5, 8, 11, 14]), alpha=0.7)
    if case == "pen0_dense":   # the covariates of the dense pieces are not penalised
        pen = np.ones(P)
        pen[[0, 1, 2, 10, 11]] = 0.0
        kw.update(penalty=pen)
    a, b, db, di = _both(mats, ad.glm.gaussian(y), **kw)
    assert db < 1e-9 and di < 1e-9
    assert a.counters["engine_panel"] == 0 and a.counters["n_panel_blocks"] == 0
    if case == "pen0_dense":
        assert np.all(np.abs(a.betas.toarray()[:, [0, 1, 2, 10, 11]]).sum(axis=0) > 0)


def test_binomial_path_on_pieces_matches_the_dense_copy(hip):
    """4: max|dbeta| < 1e-8 for binomial, intercepts alike."""
    mats, Xnp, eta, rng = _problem(300)
    y = (rng.uniform(size=300) < 1 / (1 + np.exp(-eta))).astype(float)
    a, b, db, di = _both(mats, ad.glm.binomial(y), irls_tol=1e-10, **KW)
    assert db < 1e-8 and di < 1e-8
    assert a.counters["engine_panel"] == 0 and a.counters["n_panel_blocks"] == 0


def test_cv_grpnet_on_pieces_matches_the_dense_copy(hip):
    """5: three folds on aliases of the pieces design, the losses through glm_path_losses (raw_sp_tmul)."""
    mats, Xnp, eta, rng = _problem(300)
    y = eta + 0.3 * rng.normal(size=300)
    kw = dict(n_folds=3, seed=3, lmda_path_size=12, min_ratio=0.05, progress_bar=False)
    a = ad.cv_grpnet(ad.matrix.concatenate(mats, axis=1, resident="pieces"), ad.glm.gaussian(y), **kw)
    b = ad.cv_grpnet(ad.matrix.concatenate(mats, axis=1), ad.glm.gaussian(y), **kw)
    assert np.allclose(a.lmdas, b.lmdas, rtol=1e-10)
    d = np.abs(a.losses - b.losses)
    print("max|dloss|", d.max())
    assert np.all(d <= 1e-7 * np.maximum(1.0, np.abs(b.losses)))
    assert a.best_idx == b.best_idx


def test_diagnostic_on_pieces_matches_the_dense_copy(hip):
    """6: diagnostic.diagnostic(state) runs (predict through sp_tmul, gradients through mul_batch).  The two states' coefficients
    differ by less than 1e-9 (test 4), so an entry of the gradients X^T W (y - X beta - b0) under weights 1/n differs by at most
    (p max|x|^2 + max|x|) 1e-9, beside the rounding of the sums (run_naive's bound for one entry)."""
    mats, Xnp, eta, rng = _problem(300)
    y = eta + 0.3 * rng.normal(size=300)
    a, b, db, di = _both(mats, ad.glm.gaussian(y), **KW)
    da, dd = ad.diagnostic.diagnostic(a), ad.diagnostic.diagnostic(b)
    mx = np.abs(Xnp).max()
    bound = (P * mx * mx + mx) * 1e-9 + _tol(Xnp, np.float64)
    g = np.abs(np.asarray(da.gradients) - np.asarray(dd.gradients)).max()
    print("max|dgrad|", g, "bound", bound)
    assert np.asarray(da.gradients).shape == (len(a.lmdas), P) and g <= bound
    assert np.abs(np.asarray(da.linear_preds) - np.asarray(dd.linear_preds)).max() <= (P * mx + 1) * 1e-9 + _tol(Xnp, np.float64)


def _mul_is_right(X, Xnp):
    rng = np.random.RandomState(9)
    n = Xnp.shape[0]
    v, w = rng.normal(size=n), rng.uniform(0.5, 1.5, size=n)
    out = np.empty(P)
    X.mul(v, w, out)
    return np.abs(out - (v * w) @ Xnp).max() <= _tol(Xnp, np.float64)


def test_what_a_pieces_design_refuses(hip):
    """7: every refusal raises, owns nothing afterwards and launches nothing on a view the design does not have (a following
    mul is right)."""
    X, mats, Xnp = _pieces_design(203, np.float64)
    n = 203
    rng = np.random.RandomState(4)
    y = rng.normal(size=n)
    base = owned(hip)

    def refused(fn, match="pieces", exc=RuntimeError):
        with pytest.raises(exc, match=match):
            fn()
        assert owned(hip) == base and _mul_is_right(X, Xnp)

    refused(lambda: ad.matrix.kronecker_eye(X, 2))
    refused(lambda: ad.grpnet(X, ad.glm.multigaussian(np.stack([y, -y], axis=1)), progress_bar=False))
    refused(lambda: ad.grpnet(X, ad.glm.multinomial(np.eye(2)[(y > 0).astype(int)]), progress_bar=False))
    refused(lambda: ad.matrix.standardize(X), match="standardize.*lazy=False before concatenating")
    refused(lambda: ad.matrix.standardize(X, lazy=True))
    refused(lambda: ad.matrix.standardize(X, lazy=False))
    refused(lambda: ad.matrix.subset(X, np.array([1, 2]), axis=1), match="subset other than the identity")
    refused(lambda: ad.matrix.subset(X, np.arange(10), axis=0))
    refused(lambda: X[:, 1:3])
    assert ad.matrix.subset(X, np.arange(P), axis=1) is X and ad.matrix.subset(X, np.arange(n), axis=0) is X
    refused(lambda: ad.matrix.concatenate([X, mats[0]], axis=1), match="a further concatenate")
    refused(lambda: ad.matrix.concatenate([mats[0], X], axis=1, resident="pieces"), match=r"piece 1 \(pieces\)")
    refused(lambda: ad.matrix.lazy_cov(X))
    refused(lambda: ad.bvls(X, y, np.full(P, -1.0), np.full(P, 1.0)), match="bvls")
    refused(lambda: X.impute())
    refused(lambda: ad.grpnet(X, ad.glm.gaussian(y), constraints=[ad.constraint.box(np.array([-1.0]), np.array([1.0])) for _ in range(P)],
                              progress_bar=False), match="constraints are not implemented on a design made of pieces")

    # the C-level guards behind the Python gates
    h = _abi.C.c_void_p()
    one = (_abi.C.c_void_p * 1)(X._handle)
    idx = np.array([1, 2], dtype=np.int64)
    ones = np.ones(P)
    c_calls = [
        lambda: hip.fn("design_create_multi")(X._handle, 2, 0, h),
        lambda: hip.fn("design_create_standardized")(X._handle, ones.ctypes.data, ones.ctypes.data, h),
        lambda: hip.fn("design_create_derived")(X._handle, None, 0, idx.ctypes.data, 2, None, None, h),
        lambda: hip.fn("design_create_derived")(X._handle, None, 0, None, 0, ones.ctypes.data, ones.ctypes.data, h),
        lambda: hip.fn("design_create_slice")(X._handle, 0, n, 1, 2, h),
        lambda: hip.fn("design_create_concat")(one, 1, 1, h),
        lambda: hip.fn("design_create_pieces")(one, 1, h),
        lambda: hip.fn("design_create_cov_lazy")(X._handle, h),
        lambda: hip.fn("design_impute")(X._handle, ones.ctypes.data),
    ]
    for call in c_calls:
        refused(lambda: hip.check(call()))
        assert h.value is None
    # adelie_hip_block_build_test: a diagonal block of two columns
    w = np.full(n, 1.0 / n)
    cols = np.array([0, 1], dtype=np.int32)
    table = np.zeros(10, dtype=np.int64)
    table[1] = 2
    out0 = np.zeros(4)
    info = np.zeros(16, dtype=np.int64)
    refused(lambda: hip.check(hip.fn("block_build_test")(X._handle, 0, 0, w.ctypes.data, cols.ctypes.data, 2, table.ctypes.data, 1,
                                                          None, 0, 2, 0, out0.ctypes.data, 4, None, 0, info.ctypes.data)),
            match="block_build_test is not offered on a design made of pieces")
    assert not out0.any()


def test_what_may_not_be_a_piece(hip):
    """7 and 8: refused constructions name the piece, its kind and resident="pieces", and leave nothing allocated."""
    mats, Xnp = _pieces(203, np.float64)
    rng = np.random.RandomState(8)
    S = (rng.normal(size=(203, 4)) * (rng.uniform(size=(203, 4)) < 0.2))
    others = {
        "kept sparse": ad.matrix.sparse(sp.csc_matrix(S), resident="csc"),
        "standardized view": ad.matrix.standardize(mats[1], lazy=True),
        "multi-response view": ad.matrix.kronecker_eye(mats[0], 2),
        "covariance matrix": ad.matrix.dense(np.eye(5), method="cov"),
        "constraint matrix": ad.matrix.dense(np.asfortranarray(rng.normal(size=(4, 203))), method="constraint"),
        "pieces": ad.matrix.concatenate(mats[:2], axis=1, resident="pieces"),
    }
    base = owned(hip)
    for kind, m in others.items():
        with pytest.raises(RuntimeError, match=rf'piece 2 \({kind}\).*resident="pieces"'):
            ad.matrix.concatenate([mats[0], mats[1], m], axis=1, resident="pieces")
        assert owned(hip) == base
        # the C entry refuses the same handle with the same words
        h = _abi.C.c_void_p()
        hs = (_abi.C.c_void_p * 3)(mats[0]._handle, mats[1]._handle, m._handle)
        with pytest.raises(RuntimeError, match=rf'piece 2 \({kind}\).*resident="pieces"'):
            hip.check(hip.fn("design_create_pieces")(hs, 3, h))
        assert h.value is None and owned(hip) == base
    short = ad.matrix.dense(np.asfortranarray(rng.normal(size=(100, 2))))
    f32 = ad.matrix.dense(np.asfortranarray(rng.normal(size=(203, 2)).astype(np.float32)))
    base = owned(hip)
    for m, why in [(short, "number of rows"), (f32, "dtype")]:
        with pytest.raises(RuntimeError, match=rf'piece 1 \(dense\) differs in.*{why}.*resident="pieces"'):
            ad.matrix.concatenate([mats[1], m], axis=1, resident="pieces")
        h = _abi.C.c_void_p()
        hs = (_abi.C.c_void_p * 2)(mats[1]._handle, m._handle)
        with pytest.raises(RuntimeError, match=rf'piece 1 \(dense\) differs in.*{why}.*resident="pieces"'):
            hip.check(hip.fn("design_create_pieces")(hs, 2, h))
        assert owned(hip) == base
    with pytest.raises(RuntimeError, match=r'axis must be 1.*resident="pieces"'):
        ad.matrix.concatenate(mats, axis=0, resident="pieces")
    with pytest.raises(RuntimeError, match=r'9 pieces given, at most 8'):
        ad.matrix.concatenate([mats[1]] * 9, axis=1, resident="pieces")
    h = _abi.C.c_void_p()
    hs = (_abi.C.c_void_p * 9)(*[mats[1]._handle] * 9)
    with pytest.raises(RuntimeError, match=r'9 pieces given, at most 8'):
        hip.check(hip.fn("design_create_pieces")(hs, 9, h))
    assert owned(hip) == base
    # allowed: the cap itself, any order, the same kind (the same design, even) repeated
    X8 = ad.matrix.concatenate([mats[1], mats[3], mats[1], mats[0], mats[2], mats[2], mats[3], mats[1]], axis=1, resident="pieces")
    assert owned(hip) == base
    order = [1, 3, 1, 0, 2, 2, 3, 1]
    blocks = [Xnp[:, FIRST[k]:FIRST[k] + SIZES[k]] for k in order]
    run_naive(X8, np.asfortranarray(np.concatenate(blocks, axis=1)), np.float64)


def test_a_pieces_design_owns_nothing(hip):
    """8: adelie_hip_design_owned_bytes does not move when the pieces design is made (it borrows every array; its descriptor
    lives in the handle), and returns to its base after the design and its pieces are deleted."""
    base = owned(hip)
    mats, Xnp = _pieces(256, np.float64)
    with_pieces = owned(hip)
    assert with_pieces > base
    X = ad.matrix.concatenate(mats, axis=1, resident="pieces")
    assert owned(hip) == with_pieces
    Xa = X.alias()
    assert owned(hip) == with_pieces and Xa._kind == "pieces" and _mul_is_right(Xa, Xnp)
    # the pieces stay alive through the design (keep=): dropping the caller's references frees nothing yet
    del mats
    assert owned(hip) == with_pieces and _mul_is_right(X, Xnp) and _mul_is_right(Xa, Xnp)
    del Xa, X
    assert owned(hip) == base


def test_a_solve_on_pieces_never_takes_the_panel_engine(hip, monkeypatch):
    """9: the guard.  ADELIE_HIP_CD_BLOCK_MIN_NV=1 sends every fit of the dense copy to the panel engine from the first screened
    coefficient on; the pieces design reports engine_panel == 0 and no panel block under the same hook, for the Gaussian path,
    for groups and under IRLS."""
    monkeypatch.setenv("ADELIE_HIP_CD_BLOCK_MIN_NV", "1")
    mats, Xnp, eta, rng = _problem(300)
    y = eta + 0.3 * rng.normal(size=300)
    yb = (rng.uniform(size=300) < 1 / (1 + np.exp(-eta))).astype(float)
    for glm, bound, extra in [(ad.glm.gaussian(y), 1e-9, {}), (ad.glm.gaussian(y), 1e-9, dict(groups=np.array([0, 2, 5, 8, 11, 14]))),
                              (ad.glm.binomial(yb), 1e-8, dict(irls_tol=1e-10))]:
        a, b, db, di = _both(mats, glm, **KW, **extra)
        assert b.counters["engine_panel"] == 1 and b.counters["n_panel_blocks"] > 0   # (the hook does what it says)
        assert a.counters["engine_panel"] == 0 and a.counters["n_panel_blocks"] == 0 and a.counters["n_panel_grams"] == 0
        assert db < bound and di < bound
