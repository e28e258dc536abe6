"""matrix.convex_relu over a sparse base, kept sparse, on the device: the builder writes the canonical compressed arrays of the
scipy restatement (twice the same, from a csc_matrix and from a resident handle), every MatrixNaiveBase operation matches
numpy on the dense expansion, the structured full sweep (ADELIE_HIP_RELU_SWEEP: off Z's compressed columns and the packed
mask) agrees with the compressed-column sweep of the expansion and is bit-reproducible, and the solver takes it (counter
n_sweeps_factor).  The references are matrix._relu_expand_sparse, numpy's dense expansion E and this project's own
matrix.sparse(expansion, resident="csc") / oracle.dense(E)."""
import warnings

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import adelie_amd as ad
from adelie_amd.matrix import _csc_download, _relu_expand, _relu_expand_sparse, _relu_sparse_sweep_shape
from matrix_checks import run_naive
from relu_sparse_checks import canonical, make_inputs, stored_entries
from test_gpu_factor import naive_tol, to_dense
from util import assert_same_path

pytestmark = pytest.mark.gpu

NS = [1, 5, 257, 1031]
DMS = [(3, 1), (17, 19), (5, 37), (2, 70)]   # the last two cross a 32- and a 64-gate mask word
HOOK = "ADELIE_HIP_RELU_SWEEP"
TILE_MAJOR = dict(n=2 * 16384 + 37, d=4, m=3, density=0.5)   # large enough for csc_finish's tile-major copy (design_csc.hpp)


def nnz_of(X):
    return int(X._backend.fn("design_nnz")(X._handle))


def build(Z, mask, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ad.matrix.convex_relu(Z, mask, resident="csc", **kw)


def sparse_csc(S):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ad.matrix.sparse(S, resident="csc")


def assert_equals_canonical(arrays, S, dtype):
    C, R = canonical(S, dtype)
    c_ptr, c_idx, c_val, r_ptr, r_idx, r_val = arrays
    assert c_val.dtype == dtype and r_val.dtype == dtype
    assert np.array_equal(c_ptr, C.indptr) and np.array_equal(c_idx, C.indices) and np.array_equal(c_val, C.data)
    assert np.array_equal(r_ptr, R.indptr) and np.array_equal(r_idx, R.indices) and np.array_equal(r_val, R.data)


def assert_same_arrays(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


# ---- 1. the build ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d,m", DMS)
@pytest.mark.parametrize("n", NS)
def test_build_equals_the_canonical_compressed_forms(hip, n, d, m, dtype, gated):
    Z, mask = make_inputs(n, d, m, dtype, dead_row=gated)
    X = build(Z, mask, gated=gated)
    P = (1 if gated else 2) * m * d
    assert X.shape == (n, P) and X.dtype == dtype and X._kind == "sparse" and X._device == 0
    assert X._gated is gated and X._mask_shape == (n, m)
    with pytest.raises(AttributeError):
        X._gated = not gated
    with pytest.raises(AttributeError):
        X._mask_shape = (n, m)
    assert X._scipy_host is None                                       # no host copy of the expansion at creation
    S = _relu_expand_sparse(Z, mask, gated)
    arrays = _csc_download(X)
    assert_equals_canonical(arrays, S, dtype)
    assert nnz_of(X) == stored_entries(Z, mask, gated) == S.nnz
    assert_same_arrays(arrays, _csc_download(build(Z, mask, gated=gated)))                   # a second build: identical
    assert_same_arrays(arrays, _csc_download(ad.matrix.convex_relu(sparse_csc(Z), mask, gated=gated)))   # a resident handle
    H = X._scipy                                                       # downloaded on first use
    assert (H != S).nnz == 0 and X._scipy is H


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_masked_out_entries_are_not_stored_whatever_z_holds(hip, dtype, gated):
    Z, mask = make_inputs(257, 3, 2, dtype)
    Zd = Z.toarray()
    mask[:, 1] = True
    mask[[0, 100, 256], :] = False
    Zd[0, 0], Zd[100, 2], Zd[256, 2] = np.inf, -np.inf, np.nan          # stored, in rows that every gate masks out
    Zd[7, 0] = np.inf                                                  # stored in a masked-in row: stays as it is
    mask[7, :] = True
    Z = csc_matrix(Zd)
    X = build(Z, mask, gated=gated)
    arrays = _csc_download(X)
    assert np.isinf(arrays[2]).sum() == (2 if gated else 4) * 1 and not np.isnan(arrays[2]).any()
    assert not np.isin(arrays[1], [0, 100, 256]).any()
    assert_equals_canonical(arrays, _relu_expand_sparse(Z, mask, gated), dtype)
    assert nnz_of(X) == stored_entries(Z, mask, gated)


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_build_without_a_single_entry(hip, dtype, gated):
    """An all-false mask: the build's counts sum to nothing, the six arrays are those of an empty csc_matrix, mul gives zeros
    (test_structured_sweep_of_an_all_false_mask_is_zero builds such a design too, signed and at three row tiles, for the sweep)."""
    n, d, m = 5, 3, 1
    Z, _ = make_inputs(n, d, m, dtype)
    mask = np.zeros((n, m), dtype=bool)
    X = build(Z, mask, gated=gated)
    P = (1 if gated else 2) * m * d
    assert X.shape == (n, P) and nnz_of(X) == 0
    assert_equals_canonical(_csc_download(X), csc_matrix((n, P), dtype=dtype), dtype)
    out = np.full(P, 7, dtype=dtype)
    X.mul(np.arange(1, n + 1, dtype=dtype), np.ones(n, dtype=dtype), out)
    assert not out.any()


@pytest.fixture(scope="module")
def tile_major():
    """The case whose expansion gets the tile-major copy of csc_finish: nt = 3 tiles of 16384 rows, at least 2^16 entries and
    four or more per (tile, column)."""
    t = TILE_MAJOR
    Z, mask = make_inputs(t["n"], t["d"], t["m"], np.float64, density=t["density"])
    out = {}
    for gated in (True, False):
        S = _relu_expand_sparse(Z, mask, gated)
        assert S.nnz >= 1 << 16 and S.nnz // (3 * S.shape[1]) >= 4
        out[gated] = S
    return Z, mask, out


@pytest.mark.parametrize("gated", [True, False])
def test_build_with_the_tile_major_copy(hip, tile_major, gated):
    Z, mask, S = tile_major
    X = build(Z, mask, gated=gated)
    arrays = _csc_download(X)
    assert_equals_canonical(arrays, S[gated], np.float64)
    assert nnz_of(X) == stored_entries(Z, mask, gated)
    assert_same_arrays(arrays, _csc_download(build(Z, mask, gated=gated)))


# ---- 2. every operation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [5, 257, 1031])
def test_all_operations(hip, n, dtype, gated):
    Z, mask = make_inputs(n, 17, 19, dtype, dead_row=gated)
    run_naive(build(Z, mask, gated=gated), _relu_expand(Z.toarray(), mask, gated), dtype)


# ---- 3. the structured sweep ----------------------------------------------------------------------------------------------
SWEEP_N = 2 * 4096 + 37   # three row tiles under the kernel's own shape function, the last a partial one


def check_sweep(monkeypatch, X, E, n, dtype, gated, md):
    rng = np.random.RandomState(3)
    v, w = rng.normal(size=n).astype(dtype), rng.uniform(0, 1, n).astype(dtype)
    ref = (v.astype(np.float64) * w) @ E.astype(np.float64)
    tol = naive_tol(E, dtype)
    outs = {}
    for hook in ("1", "1", "0"):
        monkeypatch.setenv(HOOK, hook)
        out = np.empty(E.shape[1], dtype=dtype)
        X.mul(v, w, out)
        err = np.abs(out - ref).max()
        print(f"n={n} P={E.shape[1]} gated={gated} {np.dtype(dtype).name} hook={hook}: max|mul - numpy| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol
        outs.setdefault(hook, []).append(out)
    assert np.array_equal(outs["1"][0], outs["1"][1])   # order-deterministic: identical bits
    dd = np.abs(outs["1"][0] - outs["0"][0]).max()
    print(f"max|structured - compressed columns| = {dd:.3e}")
    assert dd <= tol
    if not gated:
        s = outs["1"][0]
        assert np.array_equal(s[md:], -s[:md])          # the signed half is the exact negation
    return outs["1"][0]


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d,m", DMS)
def test_structured_sweep(hip, monkeypatch, d, m, dtype, gated):
    n = SWEEP_N
    assert _relu_sparse_sweep_shape(n, m)[1] >= 3 and n % 64
    Z, mask = make_inputs(n, d, m, dtype, dead_row=gated)
    check_sweep(monkeypatch, build(Z, mask, gated=gated), _relu_expand(Z.toarray(), mask, gated), n, dtype, gated, m * d)


@pytest.mark.parametrize("gated", [True, False])
def test_structured_sweep_with_the_tile_major_copy(hip, monkeypatch, tile_major, gated):
    Z, mask, S = tile_major
    n, d, m = Z.shape[0], Z.shape[1], mask.shape[1]
    assert _relu_sparse_sweep_shape(n, m)[1] >= 3
    check_sweep(monkeypatch, build(Z, mask, gated=gated), S[gated].toarray(), n, np.float64, gated, m * d)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_structured_sweep_of_an_all_false_mask_is_zero(hip, monkeypatch, dtype):
    n, d, m = SWEEP_N, 5, 37
    Z, _ = make_inputs(n, d, m, dtype)
    X = build(Z, np.zeros((n, m), dtype=bool))
    assert nnz_of(X) == 0
    v = np.random.RandomState(1).normal(size=n).astype(dtype)
    for hook in ("1", "0"):
        monkeypatch.setenv(HOOK, hook)
        out = np.full(2 * m * d, 7, dtype=dtype)
        X.mul(v, np.ones(n, dtype=dtype), out)
        assert not out.any()


# ---- 4. the solver --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_1031():
    """The recipe of test_gpu_relu.py with Z thinned to about 40 % density: Z (1031, 6), a mask of 7 columns, the expansions
    (scipy and dense) and a response that two hidden units generate."""
    n, d, m = 1031, 6, 7
    rng = np.random.RandomState(5)
    Zd = np.asfortranarray(rng.normal(size=(n, d)))
    Zd = np.asfortranarray(Zd * (rng.uniform(size=(n, d)) < 0.4))
    mask = np.asfortranarray(Zd @ rng.normal(size=(d, m)) >= 0)
    Z = csc_matrix(Zd)
    S = {g: _relu_expand_sparse(Z, mask, g) for g in (True, False)}
    E = {g: _relu_expand(Zd, mask, g) for g in (True, False)}
    Y = E[True]
    beta = np.zeros(m * d)
    beta[1 * d:2 * d] = rng.normal(size=d)
    beta[4 * d:5 * d] = rng.normal(size=d)
    eta = Y @ beta
    y = eta + 0.3 * eta.std() * rng.normal(size=n)
    return dict(Z=Z, mask=mask, d=d, m=m, eta=eta, y=y, E=E, S=S)


def _solve4(oracle, monkeypatch, b, gated, glm, bit_equal, **kw):
    """grpnet on the relu design (hook on, then off), on sparse(scipy expansion) and on the oracle."""
    X, E, d = build(b["Z"], b["mask"], gated=gated), b["E"][gated], b["d"]
    kw = dict(groups=np.arange(0, E.shape[1], d), progress_bar=False, **kw)
    monkeypatch.setenv(HOOK, "1")
    s_on = ad.grpnet(X, glm(), **kw)
    s_ref_on = ad.grpnet(sparse_csc(b["S"][gated]), glm(), **kw)
    monkeypatch.setenv(HOOK, "0")
    s_off = ad.grpnet(X, glm(), **kw)
    s_ref = ad.grpnet(sparse_csc(b["S"][gated]), glm(), **kw)
    monkeypatch.delenv(HOOK)
    s_orc = ad.grpnet(oracle.dense(E), glm(), **kw)
    assert s_on.counters["n_sweeps_factor"] > 0, s_on.counters
    assert s_off.counters["n_sweeps_factor"] == 0 and s_ref.counters["n_sweeps_factor"] == 0
    assert s_ref_on.counters["n_sweeps_factor"] == 0                 # (the scipy-built design has no structure, hook or not)
    for nm, s in (("hook=1", s_on), ("hook=0", s_off)):
        for rn, r in (("sparse(expanded)", s_ref), ("oracle", s_orc)):
            db = np.abs(s.betas.toarray() - r.betas.toarray()).max()
            di = np.abs(np.asarray(s.intercepts) - np.asarray(r.intercepts)).max()
            print(f"gated={gated} {nm} vs {rn}: max|dbeta| = {db:.3e}, max|dintercept| = {di:.3e}, n_sweeps_factor = "
                  f"{s.counters['n_sweeps_factor']}, active = {s.active_set_size}")
    if bit_equal:   # same arrays, same deterministic engines
        assert np.array_equal(s_off.betas.toarray(), s_ref.betas.toarray())
        assert np.array_equal(np.asarray(s_off.intercepts), np.asarray(s_ref.intercepts))
    for s in (s_on, s_off):
        assert_same_path(s, s_ref, 1e-6)
        assert_same_path(s, s_orc, 1e-6)
    assert s_on.active_set_size >= 2                                 # not a one-group path
    return s_on


PATH = dict(tol=1e-10, lmda_path_size=30, early_exit=False, min_ratio=5e-2)


def test_solver_gated_gaussian(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    st = _solve4(oracle, monkeypatch, b, True, lambda: ad.glm.gaussian(b["y"]), True, alpha=1, **PATH)
    assert len(st.lmdas) == 30


# Signed: the columns Y_g and -Y_g are exactly collinear, so only the elastic net has a unique split between the two signs.
def test_solver_signed_gaussian(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    _solve4(oracle, monkeypatch, b, False, lambda: ad.glm.gaussian(b["y"]), True, alpha=0.5, **PATH)


def test_solver_gated_binomial(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    z = (b["eta"] - b["eta"].mean()) / b["eta"].std()
    yb = np.random.RandomState(11).binomial(1, 1 / (1 + np.exp(-1.5 * z))).astype(float)
    _solve4(oracle, monkeypatch, b, True, lambda: ad.glm.binomial(yb), False, alpha=1, irls_tol=1e-10, **PATH)   # (to rounding only)


# ---- 5. views and CV ------------------------------------------------------------------------------------------------------
def test_cv_and_aliases_keep_the_structure(hip, monkeypatch, base_1031):
    b = base_1031
    monkeypatch.setenv(HOOK, "1")
    X, d = build(b["Z"], b["mask"], gated=True), b["d"]
    groups = np.arange(0, X.shape[1], d)
    kw = dict(n_folds=3, seed=0, groups=groups, lmda_path_size=20)
    cv = ad.cv_grpnet(X, ad.glm.gaussian(b["y"]), **kw)
    cv_ref = ad.cv_grpnet(sparse_csc(b["S"][True]), ad.glm.gaussian(b["y"]), **kw)
    assert np.allclose(cv.avg_losses, cv_ref.avg_losses)
    fit = cv.fit(X, ad.glm.gaussian(b["y"]), groups=groups, lmda_path_size=20)
    assert fit.error == "" and fit.counters["n_sweeps_factor"] > 0, fit.counters
    sa = ad.grpnet(X.alias(), ad.glm.gaussian(b["y"]), groups=groups, lmda_path_size=10, progress_bar=False)
    assert sa.error == "" and sa.counters["n_sweeps_factor"] > 0, sa.counters


def test_subset_concatenate_and_standardize_are_plain_sparse_designs(hip, monkeypatch, base_1031):
    b = base_1031
    monkeypatch.setenv(HOOK, "1")                                    # (even with the hook on: these have no structure left)
    X, E = build(b["Z"], b["mask"]), b["E"][False]
    P = E.shape[1]
    for Y, Ey in [(ad.matrix.subset(X, np.arange(3, 40), axis=1), E[:, 3:40]),
                  (ad.matrix.subset(X, np.array([5, 3, 70, P - 1]), axis=1), E[:, [5, 3, 70, P - 1]]),
                  (ad.matrix.concatenate([X, X], axis=1), np.concatenate([E, E], axis=1)),
                  (ad.matrix.subset(X, np.arange(0, 1031, 3), axis=0), E[::3])]:
        assert Y.shape == Ey.shape and not hasattr(Y, "_gated") and Y._kind == "sparse"
        assert np.array_equal(to_dense(Y), Ey)
    groups = np.arange(0, P, b["d"])
    kw = dict(groups=groups, alpha=0.5, lmda_path_size=8, progress_bar=False)
    Xs = ad.matrix.standardize(X)
    assert not hasattr(Xs, "_gated")
    s = ad.grpnet(Xs, ad.glm.gaussian(b["y"]), **kw)
    s_ref = ad.grpnet(ad.matrix.standardize(sparse_csc(b["S"][False])), ad.glm.gaussian(b["y"]), **kw)
    assert s.error == "" and s_ref.error == "" and s.counters["n_sweeps_factor"] == 0
    assert np.abs(s.betas.toarray() - s_ref.betas.toarray()).max() < 1e-8


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_inputs_are_checked(hip):
    Z, mask = make_inputs(5, 3, 2, np.float64)
    Zr = sparse_csc(Z)
    with pytest.raises(RuntimeError, match="resident dense"):
        ad.matrix.convex_relu(ad.matrix.standardize(Zr, centers=np.zeros(3), scales=np.ones(3)), mask)   # a standardized sparse view
    with pytest.raises(RuntimeError, match="resident dense"):
        ad.matrix.convex_relu(ad.matrix.snp_calldata(np.zeros((5, 3), dtype=np.int8)), mask, resident="csc")
    with pytest.raises(RuntimeError, match="no compressed arrays"):
        ad.matrix.convex_relu(ad.matrix.dense(np.asfortranarray(Z.toarray())), mask, resident="csc")
    for bad in (mask[:4], mask[:, 0], np.ones((6, 2), dtype=bool)):
        with pytest.raises(RuntimeError, match=r"mask must be \(n, m\) where mat is \(n, d\)\."):
            ad.matrix.convex_relu(Zr, bad)
        with pytest.raises(RuntimeError, match=r"mask must be \(n, m\) where mat is \(n, d\)\."):
            ad.matrix.convex_relu(Z, bad, resident="csc")
    X = ad.matrix.convex_relu(Z, mask.astype(np.int8) * 3, resident="csc")           # the mask is coerced to bool
    assert (X._scipy != _relu_expand_sparse(Z, mask, False)).nnz == 0
    # 2 * 2^15 * 2^16 = 2^32 columns do not fit the solver's 32-bit column indices: sizes alone decide (one row of Z)
    wide_Z, wide_mask = csc_matrix(([1.0], ([0], [0])), shape=(1, 1 << 16)), np.ones((1, 1 << 15), dtype=bool)
    with pytest.raises(RuntimeError, match=r"4294967296 columns \(65536 stored entries at most\).*32-bit column indices"):
        ad.matrix.convex_relu(wide_Z, wide_mask, resident="csc")
    # the default route is unchanged: a csc_matrix is densified
    Xd = ad.matrix.convex_relu(Z, mask)
    assert Xd._kind == "dense" and np.array_equal(to_dense(Xd), _relu_expand(Z.toarray(), mask, False))
