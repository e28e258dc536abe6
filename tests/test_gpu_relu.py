"""matrix.convex_relu on the device: the expansion kernel is exact, every MatrixNaiveBase operation matches numpy on the
expanded matrix, the structured full sweep (ADELIE_HIP_RELU_SWEEP: Z^T (mask o v) on the matrix cores) agrees with the dense one
and is bit-reproducible, and the solver takes it (counter n_sweeps_factor).  The references are numpy's expansion E of
(Z, mask) and this project's own matrix.dense(E) / oracle.dense(E)."""
import warnings

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import adelie_amd as ad
from adelie_amd.matrix import _RELU_RUN, _relu_sweep_shape
from matrix_checks import run_naive
from test_gpu_factor import naive_tol, to_dense
from util import assert_same_path

pytestmark = pytest.mark.gpu

NS = [1, 5, 257, 1031]
DMS = [(3, 1), (17, 19)]
HOOK = "ADELIE_HIP_RELU_SWEEP"


# ---- numpy restatement (in the dtype of Z: entries are 0, a value of Z or its negation) --------------------------------------
def np_relu(Z, mask, gated):
    n, d = Z.shape
    cols = [np.where(mask[:, jm], Z[:, jd], Z.dtype.type(0)) for jm in range(mask.shape[1]) for jd in range(d)]
    Y = np.stack(cols, axis=1) if cols else np.zeros((n, 0), dtype=Z.dtype)
    return np.asfortranarray(Y if gated else np.concatenate([Y, -Y], axis=1))


def make_inputs(n, d, m, dtype, order="F", seed=0):
    """Z and a mask whose column 0 is all false and (from two columns on) whose last column is all true."""
    rng = np.random.RandomState(seed + n + 7 * d)
    Z = rng.normal(size=(n, d)).astype(dtype)
    mask = rng.uniform(size=(n, m)) < 0.5
    if m >= 2:
        mask[:, 0], mask[:, m - 1] = False, True
    return (np.asfortranarray(Z) if order == "F" else np.ascontiguousarray(Z)), mask


def build(Z, mask, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (the C-order warning has its own test)
        return ad.matrix.convex_relu(Z, mask, **kw)


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d,m", DMS)
@pytest.mark.parametrize("n", NS)
def test_expansion_is_exact(hip, n, d, m, dtype, order, gated):
    Z, mask = make_inputs(n, d, m, dtype, order)
    if m == 1:
        mask[:, 0] = np.arange(n) % 3 != 1           # a single column: neither all false nor all true
    X = build(Z, mask, gated=gated)
    E = np_relu(Z, mask, gated)
    P = (1 if gated else 2) * m * d
    assert X.shape == E.shape == (n, P) and X.dtype == dtype
    assert np.array_equal(to_dense(X), E)
    assert X._gated is gated and X._mask_shape == (n, m)
    with pytest.raises(AttributeError):
        X._gated = not gated
    with pytest.raises(AttributeError):
        X._mask_shape = (n, m)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_all_false_and_all_true_mask_columns(hip, dtype):
    Z, mask = make_inputs(257, 17, 19, dtype)
    D = to_dense(build(Z, mask))
    assert not D[:, :17].any()                                        # mask column 0 is all false
    assert np.array_equal(D[:, 18 * 17:19 * 17], Z)                   # mask column 18 is all true
    assert np.array_equal(D[:, 19 * 17 + 18 * 17:], -Z)


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_masked_out_rows_are_zero_whatever_z_holds(hip, dtype, gated):
    Z, mask = make_inputs(257, 3, 2, dtype)
    mask[:, 1] = True
    mask[[0, 100, 256], :] = False
    Z[0, 0], Z[100, 1], Z[256, 2] = np.inf, -np.inf, np.nan
    D = to_dense(build(Z, mask, gated=gated))
    assert np.isfinite(D).all() and not D[[0, 100, 256], :].any()
    Zf = np.where(np.isfinite(Z), Z, 0).astype(dtype)
    assert np.array_equal(D, np_relu(Zf, mask, gated))


def test_inputs_are_checked(hip):
    Zc, mask = make_inputs(5, 3, 2, np.float64, "C")
    with pytest.warns(UserWarning, match="Detected matrix to be C-contiguous. Performance may improve with F-contiguous matrix."):
        ad.matrix.convex_relu(Zc, mask)
    Z = np.asfortranarray(Zc)
    E = np_relu(Z, mask, False)
    assert np.array_equal(to_dense(ad.matrix.convex_relu(ad.matrix.dense(Z), mask)), E)   # a resident dense design as Z
    Zs = Z * (np.abs(Z) > 0.5)
    Xs = ad.matrix.convex_relu(csc_matrix(Zs), mask, gated=True)                           # a csc Z is densified
    assert np.array_equal(to_dense(Xs), to_dense(ad.matrix.convex_relu(Zs, mask, gated=True)))
    assert np.array_equal(to_dense(Xs), np_relu(Zs, mask, True))
    X = ad.matrix.convex_relu(Z, mask.astype(np.int8) * 3)                                 # the mask is coerced to bool
    assert np.array_equal(to_dense(X), E)
    for bad in (mask[:4], mask[:, 0], np.ones((6, 2), dtype=bool)):
        with pytest.raises(RuntimeError, match=r"mask must be \(n, m\) where mat is \(n, d\)\."):
            ad.matrix.convex_relu(Z, bad)
    with pytest.raises(RuntimeError, match="n_threads must be >= 1"):
        ad.matrix.convex_relu(Z, mask, n_threads=0)
    with pytest.raises(RuntimeError, match="resident dense"):
        ad.matrix.convex_relu(ad.matrix.snp_calldata(np.zeros((5, 3), dtype=np.int8)), mask)
    # 2 * 2^15 * 2^16 = 2^32 columns do not fit the solver's 32-bit column indices: sizes alone decide (one row of Z)
    wide_Z, wide_mask = np.zeros((1, 1 << 16), order="F"), np.ones((1, 1 << 15), dtype=bool)
    with pytest.raises(RuntimeError, match=r"4294967296 columns \(.* GiB of values\).*32-bit column indices"):
        ad.matrix.convex_relu(wide_Z, wide_mask)
    with pytest.raises(RuntimeError, match=r"2147483648 columns \(.* GiB"):
        ad.matrix.convex_relu(wide_Z, wide_mask, gated=True)


# ---- 2. every operation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_all_operations(hip, n, dtype, gated):
    Z, mask = make_inputs(n, 17, 19, dtype, "F" if n % 2 else "C")
    run_naive(build(Z, mask, gated=gated), np_relu(Z, mask, gated), dtype)


# ---- 3. the structured sweep ----------------------------------------------------------------------------------------------
def sweep_n(d, m):
    """The smallest n that gives at least 3 row slices under the kernel's own shape function and is no multiple of a lane's
    row run (the last step is a partial one)."""
    n = next(n for n in range(1, 70002) if _relu_sweep_shape(n, d, m)[2] >= 3 and n % _RELU_RUN)
    assert n <= 70001
    return n


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d,m", DMS)
def test_structured_sweep(hip, monkeypatch, d, m, dtype, gated):
    n = sweep_n(d, m)
    Z, mask = make_inputs(n, d, m, dtype)
    X, E = ad.matrix.convex_relu(Z, mask, gated=gated), np_relu(Z, mask, gated)
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
        print(f"n={n} d={d} m={m} gated={gated} {np.dtype(dtype).name} hook={hook}: slices = {_relu_sweep_shape(n, d, m)[2]}, "
              f"max|mul - numpy| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol
        outs.setdefault(hook, []).append(out)
    assert np.array_equal(outs["1"][0], outs["1"][1])   # order-deterministic: identical bits
    dd = np.abs(outs["1"][0] - outs["0"][0]).max()
    print(f"max|structured - dense| = {dd:.3e}")
    assert dd <= tol
    if not gated:
        s = outs["1"][0]
        assert np.array_equal(s[m * d:], -s[:m * d])    # the signed half is the negated copy


# ---- 4. the solver --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_1031():
    """Z (1031, 6), a mask of 7 columns, the two expansions and a response that two hidden units generate."""
    n, d, m = 1031, 6, 7
    rng = np.random.RandomState(5)
    Z = np.asfortranarray(rng.normal(size=(n, d)))
    mask = np.asfortranarray(Z @ rng.normal(size=(d, m)) >= 0)      # D_k = 1[Z u_k >= 0], as the convex reformulation draws them
    Y = np_relu(Z, mask, True)
    beta = np.zeros(m * d)
    beta[1 * d:2 * d] = rng.normal(size=d)
    beta[4 * d:5 * d] = rng.normal(size=d)
    eta = Y @ beta
    y = eta + 0.3 * eta.std() * rng.normal(size=n)
    return dict(Z=Z, mask=mask, d=d, m=m, eta=eta, y=y, E={True: Y, False: np_relu(Z, mask, False)})


def _solve4(oracle, monkeypatch, b, gated, glm, **kw):
    """grpnet on the relu design (hook on, then off), on dense(expanded) and on the oracle."""
    X, E, d = ad.matrix.convex_relu(b["Z"], b["mask"], gated=gated), b["E"][gated], b["d"]
    kw = dict(groups=np.arange(0, E.shape[1], d), progress_bar=False, **kw)
    monkeypatch.setenv(HOOK, "1")
    s_on = ad.grpnet(X, glm(), **kw)
    monkeypatch.setenv(HOOK, "0")
    s_off = ad.grpnet(X, glm(), **kw)
    monkeypatch.delenv(HOOK)
    s_dense = ad.grpnet(ad.matrix.dense(E), glm(), **kw)
    s_orc = ad.grpnet(oracle.dense(E), glm(), **kw)
    assert s_on.counters["n_sweeps_factor"] > 0, s_on.counters
    assert s_off.counters["n_sweeps_factor"] == 0 and s_dense.counters["n_sweeps_factor"] == 0
    for nm, s in (("hook=1", s_on), ("hook=0", s_off)):
        for rn, r in (("dense(expanded)", s_dense), ("oracle", s_orc)):
            db = np.abs(s.betas.toarray() - r.betas.toarray()).max()
            di = np.abs(np.asarray(s.intercepts) - np.asarray(r.intercepts)).max()
            print(f"gated={gated} {nm} vs {rn}: max|dbeta| = {db:.3e}, max|dintercept| = {di:.3e}, n_sweeps_factor = "
                  f"{s.counters['n_sweeps_factor']}, active = {s.active_set_size}")
    for s in (s_on, s_off):
        assert_same_path(s, s_dense, 1e-6)
        assert_same_path(s, s_orc, 1e-6)
    assert s_on.active_set_size >= 2                                 # not a one-group path
    return s_on


def _binomial_y(b):
    z = (b["eta"] - b["eta"].mean()) / b["eta"].std()
    return np.random.RandomState(11).binomial(1, 1 / (1 + np.exp(-1.5 * z))).astype(float)


PATH = dict(tol=1e-10, lmda_path_size=30, early_exit=False, min_ratio=5e-2)


def test_solver_gated_gaussian(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    st = _solve4(oracle, monkeypatch, b, True, lambda: ad.glm.gaussian(b["y"]), alpha=1, **PATH)
    assert len(st.lmdas) == 30


def test_solver_gated_binomial(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    yb = _binomial_y(b)
    _solve4(oracle, monkeypatch, b, True, lambda: ad.glm.binomial(yb), alpha=1, irls_tol=1e-10, **PATH)


# Signed: the columns Y_g and -Y_g are exactly collinear, so only the elastic net has a unique split between the two signs
# (at alpha = 1 two correct solvers may legitimately differ).
def test_solver_signed_gaussian(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    _solve4(oracle, monkeypatch, b, False, lambda: ad.glm.gaussian(b["y"]), alpha=0.5, **PATH)


def test_solver_signed_binomial(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    yb = _binomial_y(b)
    _solve4(oracle, monkeypatch, b, False, lambda: ad.glm.binomial(yb), alpha=0.5, irls_tol=1e-10, **PATH)


# ---- 5. views and CV ------------------------------------------------------------------------------------------------------
def test_cv_and_aliases_keep_the_structure(hip, monkeypatch, base_1031):
    b = base_1031
    monkeypatch.setenv(HOOK, "1")
    X, E, d = ad.matrix.convex_relu(b["Z"], b["mask"], gated=True), b["E"][True], b["d"]
    groups = np.arange(0, E.shape[1], d)
    kw = dict(n_folds=3, seed=0, groups=groups, lmda_path_size=20)
    cv = ad.cv_grpnet(X, ad.glm.gaussian(b["y"]), **kw)
    cv_ref = ad.cv_grpnet(ad.matrix.dense(E), ad.glm.gaussian(b["y"]), **kw)
    assert np.allclose(cv.avg_losses, cv_ref.avg_losses)
    fit = cv.fit(X, ad.glm.gaussian(b["y"]), groups=groups, lmda_path_size=20)
    assert fit.error == "" and fit.counters["n_sweeps_factor"] > 0, fit.counters
    sa = ad.grpnet(X.alias(), ad.glm.gaussian(b["y"]), groups=groups, lmda_path_size=10, progress_bar=False)
    assert sa.error == "" and sa.counters["n_sweeps_factor"] > 0, sa.counters


def test_subset_and_concatenate_are_plain_dense_designs(hip, monkeypatch, base_1031):
    b = base_1031
    monkeypatch.setenv(HOOK, "1")                                    # (even with the hook on: these have no structure left)
    X, E = ad.matrix.convex_relu(b["Z"], b["mask"]), b["E"][False]
    P = E.shape[1]
    rng = np.random.RandomState(2)
    v, w = rng.normal(size=1031), rng.uniform(0, 1, 1031)
    for Y, Ey in [(ad.matrix.subset(X, np.arange(3, 40), axis=1), E[:, 3:40]),
                  (ad.matrix.subset(X, np.array([5, 3, 70, P - 1]), axis=1), E[:, [5, 3, 70, P - 1]]),
                  (ad.matrix.concatenate([X, X], axis=1), np.concatenate([E, E], axis=1)),
                  (ad.matrix.subset(X, np.arange(0, 1031, 3), axis=0), E[::3])]:
        assert Y.shape == Ey.shape and not hasattr(Y, "_gated")
        vv, ww = (v, w) if Y.shape[0] == 1031 else (v[::3], w[::3])
        out = np.empty(Ey.shape[1])
        Y.mul(vv, ww, out)
        assert np.abs(out - (vv * ww) @ Ey).max() <= naive_tol(Ey, np.float64)
        assert np.array_equal(to_dense(Y), Ey)
    # a standardized view and a multi-response family run on the design as on any dense one
    groups = np.arange(0, P, b["d"])
    kw = dict(groups=groups, alpha=0.5, lmda_path_size=8, progress_bar=False)
    s = ad.grpnet(ad.matrix.standardize(X), ad.glm.gaussian(b["y"]), **kw)
    s_ref = ad.grpnet(ad.matrix.standardize(ad.matrix.dense(E)), ad.glm.gaussian(b["y"]), **kw)
    assert s.error == "" and s.counters["n_sweeps_factor"] == 0
    assert np.abs(s.betas.toarray() - s_ref.betas.toarray()).max() < 1e-8
    yk = np.stack([b["y"], b["eta"]], axis=1)
    s = ad.grpnet(X, ad.glm.multigaussian(yk), alpha=0.5, lmda_path_size=5, progress_bar=False)
    s_ref = ad.grpnet(ad.matrix.dense(E), ad.glm.multigaussian(yk), alpha=0.5, lmda_path_size=5, progress_bar=False)
    assert s.error == "" and s.betas.shape[1] == P * 2
    assert np.abs(s.betas.toarray() - s_ref.betas.toarray()).max() < 1e-8
