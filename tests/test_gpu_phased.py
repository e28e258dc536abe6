"""matrix.snp_phased_ancestry / matrix.snp_phased_calldata on the device (``adelie_hip_design_create_snp_phased_ancestry``,
``..._calldata``, ``kernels_phased.hip``) -- reference ``MatrixNaiveSNPPhasedAncestry`` (``matrix_naive_snp_phased_ancestry.ipp``,
``adelie/matrix.py:1189-1242``).

The design is built on the device as a design kept sparse; its arrays, downloaded again, must EQUAL scipy's canonical
compressed forms of the numpy expansion, for both dtypes and both entry points, and two builds must agree exactly.  The
reference's check list for a matrix class (``run_naive``) runs against the expansion; paths are compared with the same arrays
uploaded through ``matrix.sparse(resident="csc")`` (equal bit for bit: the same arrays under the same deterministic engines)
and with the CPU restatement on the dense expansion."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adelie_amd as ad
from adelie_amd import _abi
from adelie_amd import matrix as M
from matrix_checks import run_naive
from phased_checks import altered

pytestmark = pytest.mark.gpu

TILE = M._PHASED_TILE_ROWS
SHAPES = [(5, 2, 2), (211, 7, 3), (1030, 5, 8), (70, 40, 1), (1, 3, 2), (2 * TILE + 37, 4, 3)]

_cases = {}


def case(n, s, A):
    """(calldata, ancestries, E) of one shape, made once and shared (read-only) by the tests."""
    key = (n, s, A)
    if key not in _cases:
        cal, anc, E = altered(ad.data.snp_phased_ancestry(n, s, A, sparsity=0.5, seed=n % 7), A)
        for a in (cal, anc, E):
            a.setflags(write=False)
        _cases[key] = (cal, anc, E)
    return _cases[key]


def canonical(E, dtype):
    C = sp.csc_matrix(E.astype(dtype))
    C.sort_indices()
    R = C.tocsr()
    R.sort_indices()
    return C, R


def assert_equals_canonical(arrays, E, dtype):
    C, R = canonical(E, dtype)
    c_ptr, c_idx, c_val, r_ptr, r_idx, r_val = arrays
    assert c_val.dtype == dtype and r_val.dtype == dtype
    assert np.array_equal(c_ptr, C.indptr) and np.array_equal(c_idx, C.indices) and np.array_equal(c_val, C.data)
    assert np.array_equal(r_ptr, R.indptr) and np.array_equal(r_idx, R.indices) and np.array_equal(r_val, R.data)


def from_file(tmp_path, cal, anc, A, dtype, read=True):
    path = str(tmp_path / "phased.snpdat")
    ad.io.snp_phased_ancestry(path).write(cal, anc, A)
    h = ad.io.snp_phased_ancestry(path)
    if read:
        h.read()
    return ad.matrix.snp_phased_ancestry(h, dtype=dtype)


def _csc(Mx):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ad.matrix.sparse(Mx, resident="csc")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,s,A", SHAPES)
def test_build_equals_the_canonical_compressed_forms(hip, tmp_path, dtype, n, s, A):
    cal, anc, E = case(n, s, A)
    X = ad.matrix.snp_phased_calldata(cal, anc, A, dtype=dtype)
    assert X._kind == "sparse" and (X.rows(), X.cols()) == (n, s * A) and X.dtype == dtype
    assert X.ancestries == A and np.array_equal(X.groups, A * np.arange(s)) and np.array_equal(X.group_sizes, np.full(s, A))
    first = M._csc_download(X)
    assert int(hip.fn("design_nnz")(X._handle)) == np.count_nonzero(E) == first[1].size
    assert_equals_canonical(first, E, dtype)
    again = M._csc_download(ad.matrix.snp_phased_calldata(cal, anc, A, dtype=dtype))   # a second build: identical arrays
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    F = from_file(tmp_path, cal, anc, A, dtype, read=(n % 2 == 0))                       # (read here or by the constructor)
    assert F.ancestries == A and (F.rows(), F.cols()) == (n, s * A)
    assert_equals_canonical(M._csc_download(F), E, dtype)
    # a NULL pointer skips its array
    ptr = np.empty(s * A + 1, dtype=np.int64)
    hip.check(hip.fn("design_csc_download")(X._handle, ptr.ctypes.data, None, None, None, None, None))
    assert np.array_equal(ptr, first[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_build_without_a_single_entry(hip, dtype):
    """All-zero calldata: the build's counts sum to nothing, the six arrays are those of an empty csc_matrix, mul gives zeros."""
    n, s, A = 5, 2, 2
    cal = np.zeros((n, 2 * s), dtype=np.int8, order="F")
    anc = np.asfortranarray(np.random.RandomState(0).randint(0, A, size=(n, 2 * s)).astype(np.int8))
    X = ad.matrix.snp_phased_calldata(cal, anc, A, dtype=dtype)
    assert int(hip.fn("design_nnz")(X._handle)) == 0
    assert_equals_canonical(M._csc_download(X), np.zeros((n, s * A)), dtype)
    out = np.full(s * A, 7, dtype=dtype)
    X.mul(np.arange(1, n + 1, dtype=dtype), np.ones(n, dtype=dtype), out)
    assert not out.any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,s,A", SHAPES[:4] + SHAPES[5:])
def test_design_runs_the_reference_check_list(hip, dtype, n, s, A):
    cal, anc, E = case(n, s, A)
    run_naive(ad.matrix.snp_phased_calldata(cal, anc, A, dtype=dtype), np.asfortranarray(E.astype(dtype)), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_design_with_the_tile_major_copy(hip, dtype):
    """About 4.8e5 stored entries over 70 001 rows: create_csc's finishing half builds the tile-major copy for the full sweeps
    (16384 f64 / 32768 f32 rows per tile, a ragged last tile) from the arrays the device build left."""
    n, s, A = 70_001, 20, 3
    cal, anc, E = altered(ad.data.snp_phased_ancestry(n, s, A, seed=2), A)
    nnz = np.count_nonzero(E)
    itemsize = np.dtype(dtype).itemsize
    nt = -(-n // (128 * 1024 // itemsize))
    assert nt > 1 and nnz >= 1 << 16 and nnz // (nt * s * A) >= 4     # the `worth` condition of the copy
    X = ad.matrix.snp_phased_calldata(cal, anc, A, dtype=dtype)
    assert_equals_canonical(M._csc_download(X), E, dtype)
    D = np.asfortranarray(E.astype(dtype))
    run_naive(X, D, dtype)
    D64 = E.astype(np.float64)
    c, sc = D64.mean(axis=0), D64.std(axis=0)
    sc[sc == 0] = 1.0                                                # (the columns of the empty SNP have no spread)
    Z = ad.matrix.standardize(X, centers=c, scales=sc)
    assert Z._kind == "sparse"
    run_naive(Z, np.asfortranarray(((D64 - c) / sc).astype(dtype)), dtype)


@pytest.fixture(scope="module")
def problem():
    n, s, A = 1030, 12, 3
    d = ad.data.snp_phased_ancestry(n, s, A, sparsity=0.5, seed=5)
    cal, anc, E = altered(d, A)
    D = np.asfortranarray(E.astype(np.float64))
    rng = np.random.RandomState(9)
    beta = np.zeros(s * A)
    beta[[4, 5, 16, 30]] = (1.0, -1.5, 0.8, 0.6)
    eta = D @ beta
    y = eta + 0.3 * rng.normal(size=n)
    yb = (rng.uniform(size=n) < 1 / (1 + np.exp(-(eta - eta.mean())))).astype(float)
    return dict(cal=cal, anc=anc, A=A, D=D, E=E, y=y, yb=yb, groups=A * np.arange(s))


def test_gaussian_path_equals_the_scipy_built_design_and_matches_the_cpu(hip, oracle, problem):
    p = problem
    kw = dict(groups=p["groups"], tol=1e-12, early_exit=False, lmda_path_size=12, min_ratio=0.05, progress_bar=False)
    X = ad.matrix.snp_phased_calldata(p["cal"], p["anc"], p["A"])
    a = ad.grpnet(X, ad.glm.gaussian(p["y"]), **kw)
    # laziness: building the design and running a path has formed no host copy of the matrix
    assert X._scipy_host is None
    b = ad.grpnet(_csc(sp.csc_matrix(p["D"])), ad.glm.gaussian(p["y"]), **kw)
    c = ad.grpnet(oracle.dense(p["D"]), ad.glm.gaussian(p["y"]), **kw)
    assert a.error == "" and b.error == "" and c.error == ""
    assert np.count_nonzero(a.betas.toarray()[-1]) > 3
    assert np.array_equal(a.betas.toarray(), b.betas.toarray()) and np.array_equal(a.intercepts, b.intercepts)
    db, di = np.abs(a.betas.toarray() - c.betas.toarray()).max(), np.abs(a.intercepts - c.intercepts).max()
    print(f"gaussian vs cpu: max|dbeta|={db:.3e} max|dintercept|={di:.3e}")
    assert db < 1e-9 and di < 1e-9
    # ... and the host matrix, when something asks for it, is the expansion
    S = X._scipy
    assert X._scipy_host is S and (S != sp.csc_matrix(p["D"])).nnz == 0


def test_binomial_path_matches_the_cpu(hip, oracle, problem):
    p = problem
    kw = dict(groups=p["groups"], tol=1e-10, irls_tol=1e-10, early_exit=False, lmda_path_size=12, min_ratio=0.05, progress_bar=False)
    X = ad.matrix.snp_phased_calldata(p["cal"], p["anc"], p["A"])
    a = ad.grpnet(X, ad.glm.binomial(p["yb"]), **kw)
    c = ad.grpnet(oracle.dense(p["D"]), ad.glm.binomial(p["yb"]), **kw)
    assert a.error == "" and c.error == ""
    db, di = np.abs(a.betas.toarray() - c.betas.toarray()).max(), np.abs(a.intercepts - c.intercepts).max()
    print(f"binomial vs cpu: max|dbeta|={db:.3e} max|dintercept|={di:.3e}")
    assert db < 1e-6 and di < 1e-6


def test_cv_grpnet_matches_the_scipy_built_design(hip, problem):
    """The folds are derived designs: they start from the lazily downloaded host matrix."""
    p = problem
    kw = dict(groups=p["groups"], n_folds=3, seed=1, lmda_path_size=8, min_ratio=0.1, progress_bar=False)
    X = ad.matrix.snp_phased_calldata(p["cal"], p["anc"], p["A"])
    assert X._scipy_host is None
    a = ad.cv_grpnet(X, ad.glm.gaussian(p["y"]), **kw)
    b = ad.cv_grpnet(_csc(sp.csc_matrix(p["D"])), ad.glm.gaussian(p["y"]), **kw)
    assert np.allclose(a.lmdas, b.lmdas, rtol=1e-10)
    assert np.abs(a.losses - b.losses).max() < 1e-7 * max(1.0, np.abs(b.losses).max())
    assert a.best_idx == b.best_idx


def test_damaged_image_is_an_error_and_creates_no_design(hip, tmp_path):
    cal, anc, _ = case(211, 7, 3)
    path = str(tmp_path / "cut.snpdat")
    ad.io.snp_phased_ancestry(path).write(cal, anc, 3)
    h = ad.io.snp_phased_ancestry(path)
    nbytes = h.read()
    buf = np.ascontiguousarray(h._buffer[:nbytes - 7])
    handle = _abi.C.c_void_p()
    rc = hip.fn("design_create_snp_phased_ancestry")(buf.ctypes.data, buf.size, _abi.dtype_code(np.float64), 0, handle)
    assert rc != 0 and handle.value is None
    assert b"corrupt .snpdat SNP index" in hip.fn("last_error")()
    h._buffer = buf
    with pytest.raises(RuntimeError, match="corrupt .snpdat"):
        ad.matrix.snp_phased_ancestry(h)
    # the calldata route raises the writer's errors
    bad = np.array(anc)
    bad[3, 2] = 3
    with pytest.raises(RuntimeError, match=r"Detected an ancestry not in the range \[0, A\)"):
        ad.matrix.snp_phased_calldata(cal, bad, 3)
    bad = np.array(cal)
    bad[3, 2] = 2
    with pytest.raises(RuntimeError, match="Detected a non-binary value"):
        ad.matrix.snp_phased_calldata(bad, anc, 3)
    with pytest.raises(RuntimeError, match="Number of ancestries A must be < 256"):
        ad.matrix.snp_phased_calldata(cal, anc, 256)
