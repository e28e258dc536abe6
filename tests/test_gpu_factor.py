"""matrix.one_hot / matrix.interaction on the device: the expansion kernel is exact, every MatrixNaiveBase operation matches
numpy on the expanded matrix, the structured full sweep (ADELIE_HIP_FACTOR_SWEEP) agrees with the dense one and is
bit-reproducible, and the solver takes it (counter n_sweeps_factor).  The expansion is restated in numpy below, as
tests/test_reference_known_answers.py does (reference matrix_naive_one_hot.ipp, matrix_naive_interaction.ipp)."""
import warnings

import numpy as np
import pytest
from scipy.sparse import identity

import adelie_amd as ad
from matrix_checks import run_naive
from util import assert_same_path

pytestmark = pytest.mark.gpu

LEVELS = np.array([0, 1, 3, 0, 70, 2])
INTR_MAP = {0: None, 2: [4, 5], 4: [3]}   # cont-cont, cont-disc, disc-cont, disc-disc, and a 3 x 70 = 210-column block
PAIRS = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (2, 4), (2, 5), (4, 3)]
SIZES = [2, 6, 3, 140, 4, 210, 6, 140]
NS = [1, 5, 257, 1031]


# ---- numpy restatement (in the dtype of Z: entries are 0, 1, a value of Z or one product of two values of Z) ---------------
def _basis(Z, j, L):
    one = np.ones(Z.shape[0], dtype=Z.dtype)
    return [one, Z[:, j]] if L <= 0 else [(Z[:, j] == l).astype(Z.dtype) for l in range(L)]


def np_one_hot(Z, levels):
    cols, groups = [], []
    for j, L in enumerate(levels):
        groups.append(len(cols))
        cols.extend([Z[:, j]] if L <= 0 else _basis(Z, j, L))
    return np.asfortranarray(np.stack(cols, axis=1)), np.array(groups)


def np_interaction(Z, pairs, levels):
    cols, groups = [], []
    for i, j in pairs:
        A, B = _basis(Z, i, levels[i]), _basis(Z, j, levels[j])
        blk = [a * b for b in B for a in A]            # A's columns run fastest
        if levels[i] <= 0 and levels[j] <= 0:
            blk = blk[1:]                              # [Z_i, Z_j, Z_i Z_j]
        groups.append(len(cols))
        cols.extend(blk)
    return np.asfortranarray(np.stack(cols, axis=1)), np.array(groups)


def make_Z(n, dtype, order="F", seed=0):
    rng = np.random.RandomState(seed + n)
    Z = np.empty((n, len(LEVELS)), dtype=dtype)
    for j, L in enumerate(LEVELS):
        Z[:, j] = rng.normal(size=n) if L <= 0 else rng.randint(0, L, size=n)
    return np.asfortranarray(Z) if order == "F" else np.ascontiguousarray(Z)


def build(ctor, Z, *args):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (the C-order warning has its own test)
        return ctor(Z, *args)


def to_dense(X):
    """X^T through sp_tmul with an identity CSR: every stored entry comes back as 1.0 * x + 0."""
    n, p = X.shape
    out = np.empty((p, n), dtype=X.dtype)
    X.sp_tmul(identity(p, dtype=X.dtype, format="csr"), out)
    return out.T


def naive_tol(X, dtype):
    """The bound of matrix_checks.run_naive for one dot product over the rows of X."""
    n = X.shape[0]
    xmax = max(1.0, np.abs(X).max())
    return 1e-12 * xmax * n if dtype == np.float64 else 1e-4 * xmax * np.sqrt(n) * 10


@pytest.fixture(scope="module")
def base_1031():
    """Z (n = 1031, f64), the two numpy expansions and a response with signal in all four kinds of blocks."""
    Z = make_Z(1031, np.float64)
    E_oh, g_oh = np_one_hot(Z, LEVELS)
    E_in, g_in = np_interaction(Z, PAIRS, LEVELS)
    rng = np.random.RandomState(7)
    beta = np.zeros(E_in.shape[1])
    for g in (1, 2, 6, 7):                              # (0,2) cont-disc, (0,3) cont-cont, (2,5) disc-disc, (4,3) disc-cont
        beta[g_in[g]:g_in[g] + SIZES[g]] = rng.normal(size=SIZES[g])
    eta = E_in @ beta
    y = eta + 0.5 * eta.std() * rng.normal(size=1031)
    return dict(Z=Z, E_oh=E_oh, g_oh=g_oh, E_in=E_in, g_in=g_in, y=y, eta=eta)


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["F", "C"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_expansion_is_exact(hip, n, dtype, order):
    Z = make_Z(n, dtype, order)
    X = build(ad.matrix.one_hot, Z, LEVELS)
    E, g = np_one_hot(Z, LEVELS)
    assert X.shape == E.shape == (n, 78) and X.dtype == dtype
    assert np.array_equal(to_dense(X), E)
    assert np.array_equal(X.groups, g) and np.array_equal(X.group_sizes, np.diff(np.append(g, 78)))
    assert np.array_equal(X._levels, LEVELS)
    X = build(ad.matrix.interaction, Z, INTR_MAP, LEVELS)
    E, g = np_interaction(Z, PAIRS, LEVELS)
    assert X.shape == E.shape == (n, 511)
    assert np.array_equal(to_dense(X), E)
    assert np.array_equal(X.groups, g) and X.group_sizes.tolist() == SIZES
    assert [tuple(r) for r in X._pairs] == PAIRS and np.array_equal(X._levels, LEVELS)
    assert X.groups.dtype.kind == "i" and not X.groups.flags.writeable
    with pytest.raises(AttributeError):
        X.groups = g


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_values_outside_the_levels_give_zero_rows(hip, dtype):
    Z = make_Z(257, dtype)
    Z[3, 2], Z[100, 2], Z[256, 2] = -1, 3, 0.5          # column 2 has 3 levels
    Z[7, 4] = 70                                        # column 4 has 70
    for X, (E, g) in [(ad.matrix.one_hot(Z, LEVELS), np_one_hot(Z, LEVELS)),
                      (ad.matrix.interaction(Z, INTR_MAP, LEVELS), np_interaction(Z, PAIRS, LEVELS))]:
        D = to_dense(X)
        assert np.array_equal(D, E)
        blocks2 = [2] if D.shape[1] == 78 else [1, 5, 6]   # the blocks that column 2 takes part in
        for b in blocks2:
            sl = slice(g[b], g[b] + X.group_sizes[b])
            assert not D[[3, 100, 256], sl].any() and D[[4, 101], sl].any()
        b4 = 4 if D.shape[1] == 78 else 3
        assert not D[7, g[b4]:g[b4] + X.group_sizes[b4]].any()


def test_c_order_warns_like_dense_and_inputs_are_checked(hip):
    Zc = make_Z(5, np.float64, "C")
    with pytest.warns(UserWarning, match="Detected matrix to be C-contiguous. Performance may improve with F-contiguous matrix."):
        ad.matrix.one_hot(Zc, LEVELS)
    with pytest.warns(UserWarning, match="Detected matrix to be C-contiguous"):
        ad.matrix.interaction(Zc, INTR_MAP, LEVELS)
    Z = make_Z(5, np.float64)
    X = ad.matrix.one_hot(Z)                            # levels=None: every column continuous
    assert np.array_equal(to_dense(X), Z) and X.group_sizes.tolist() == [1] * 6
    Xd = ad.matrix.one_hot(ad.matrix.dense(Z), LEVELS)  # a resident dense design is accepted as the table
    assert np.array_equal(to_dense(Xd), np_one_hot(Z, LEVELS)[0])
    with pytest.raises(RuntimeError, match="n_threads must be >= 1"):
        ad.matrix.interaction(Z, INTR_MAP, LEVELS, n_threads=0)
    with pytest.raises(ValueError, match="No valid pairs exist"):
        ad.matrix.interaction(Z, {1: [1]}, LEVELS)
    with pytest.raises(RuntimeError, match="resident dense"):
        ad.matrix.one_hot(ad.matrix.snp_calldata(np.zeros((5, 6), dtype=np.int8)), LEVELS)
    with pytest.raises(RuntimeError, match=r"GiB"):    # 2^20 x 2^20 levels: P does not fit the 32-bit column indices
        ad.matrix.interaction(Z, {4: [5]}, np.array([0, 0, 0, 0, 1 << 20, 1 << 20]))


# ---- 2. every operation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", NS)
def test_all_operations(hip, n, dtype):
    Z = make_Z(n, dtype, "F" if n % 2 else "C")
    run_naive(build(ad.matrix.one_hot, Z, LEVELS), np_one_hot(Z, LEVELS)[0], dtype)
    run_naive(build(ad.matrix.interaction, Z, INTR_MAP, LEVELS), np_interaction(Z, PAIRS, LEVELS)[0], dtype)


# ---- 3. the structured sweep ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("ctor", ["one_hot", "interaction"])
def test_structured_sweep(hip, monkeypatch, ctor, dtype):
    n = 70001                                           # several row slices
    Z = make_Z(n, dtype)
    Z[11, 2], Z[12, 4] = 5, 0.25                        # rows that belong to no level
    if ctor == "one_hot":
        X, E = ad.matrix.one_hot(Z, LEVELS), np_one_hot(Z, LEVELS)[0]
    else:
        X, E = ad.matrix.interaction(Z, INTR_MAP, LEVELS), np_interaction(Z, PAIRS, LEVELS)[0]
    rng = np.random.RandomState(3)
    v, w = rng.normal(size=n).astype(dtype), rng.uniform(0, 1, n).astype(dtype)
    ref = (v.astype(np.float64) * w) @ E.astype(np.float64)
    tol = naive_tol(E, dtype)
    outs = {}
    for hook in ("1", "1", "0"):
        monkeypatch.setenv("ADELIE_HIP_FACTOR_SWEEP", hook)
        out = np.empty(E.shape[1], dtype=dtype)
        X.mul(v, w, out)
        err = np.abs(out - ref).max()
        print(f"{ctor} {np.dtype(dtype).name} hook={hook}: max|mul - numpy| = {err:.3e} (bound {tol:.3e})")
        assert err <= tol
        outs.setdefault(hook, []).append(out)
    assert np.array_equal(outs["1"][0], outs["1"][1])   # order-deterministic: identical bits
    d = np.abs(outs["1"][0] - outs["0"][0]).max()
    print(f"{ctor} {np.dtype(dtype).name}: max|structured - dense| = {d:.3e}")
    assert d <= tol


# ---- 4. the solver --------------------------------------------------------------------------------------------------------
def _solve3(oracle, monkeypatch, b, glm, **kw):
    """grpnet on the interaction design (hook on, then off), on dense(expanded) and on the oracle."""
    X = ad.matrix.interaction(b["Z"], INTR_MAP, LEVELS)
    kw = dict(groups=X.groups, progress_bar=False, **kw)
    monkeypatch.setenv("ADELIE_HIP_FACTOR_SWEEP", "1")
    s_on = ad.grpnet(X, glm(), **kw)
    monkeypatch.setenv("ADELIE_HIP_FACTOR_SWEEP", "0")
    s_off = ad.grpnet(X, glm(), **kw)
    monkeypatch.delenv("ADELIE_HIP_FACTOR_SWEEP")
    s_dense = ad.grpnet(ad.matrix.dense(b["E_in"]), glm(), **kw)
    s_orc = ad.grpnet(oracle.dense(b["E_in"]), glm(), **kw)
    assert s_on.counters["n_sweeps_factor"] > 0, s_on.counters
    assert s_off.counters["n_sweeps_factor"] == 0 and s_dense.counters["n_sweeps_factor"] == 0
    for nm, s in (("hook=1", s_on), ("hook=0", s_off)):
        for rn, r in (("dense(expanded)", s_dense), ("oracle", s_orc)):
            db = np.abs(s.betas.toarray() - r.betas.toarray()).max()
            di = np.abs(np.asarray(s.intercepts) - np.asarray(r.intercepts)).max()
            print(f"{nm} vs {rn}: max|dbeta| = {db:.3e}, max|dintercept| = {di:.3e}, n_sweeps_factor = "
                  f"{s.counters['n_sweeps_factor']}, active = {s.active_set_size}")
    for s in (s_on, s_off):
        assert_same_path(s, s_dense, 1e-6)
        assert_same_path(s, s_orc, 1e-6)
    return s_on


def test_solver_gaussian(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    st = _solve3(oracle, monkeypatch, b, lambda: ad.glm.gaussian(b["y"]), tol=1e-10, lmda_path_size=30, early_exit=False,
                 min_ratio=5e-2)
    # (the intercept is on: the `sub_vec` epilogue ran in every full sweep.)  The path is not a one-group path: the signal of
    # the (4, 3) block is a function of Z_4, Z_3 and that of the other three blocks of Z_0, Z_2, Z_5, so no single group
    # explains both.  It need not use all four generating groups: the blocks overlap (the span of the (2, 5) block holds the
    # indicators of Z_2 that the (0, 2) block starts with), and a group lasso may serve two of them with one group.
    assert len(st.lmdas) == 30 and st.active_set_size >= 2


def test_solver_binomial(hip, oracle, monkeypatch, base_1031):
    b = base_1031
    rng = np.random.RandomState(11)
    z = (b["eta"] - b["eta"].mean()) / b["eta"].std()
    yb = rng.binomial(1, 1 / (1 + np.exp(-1.5 * z))).astype(float)
    _solve3(oracle, monkeypatch, b, lambda: ad.glm.binomial(yb), tol=1e-10, irls_tol=1e-10, lmda_path_size=30,
            early_exit=False, min_ratio=5e-2)


# ---- 5. examples.ipynb cells 4-24 through the front door -------------------------------------------------------------------
def _replay_examples_notebook_front_door():
    n, d_cont, d_disc = 1000, 10, 10
    np.random.seed(1)                                                                  # cell 4
    Z_cont = np.random.normal(0, 1, (n, d_cont))
    levels = np.random.choice(10, d_disc, replace=True) + 1
    Z_disc = np.array([np.random.choice(lvl, n, replace=True) for lvl in levels]).T
    Z_cont = (Z_cont - np.mean(Z_cont, axis=0)) / np.std(Z_cont, axis=0, ddof=0)       # cell 6
    Z = np.asfortranarray(np.concatenate([Z_cont, Z_disc], axis=1))                    # cell 8
    levels = np.concatenate([np.zeros(d_cont), levels])
    Z_one_hot_0 = np.zeros((n, int(levels[d_cont])))                                   # cell 10
    Z_one_hot_0[np.arange(n), Z_disc[:, 0].astype(int)] = 1
    Z_cont_0 = Z_cont[:, 0][:, None]
    Z_sub = np.concatenate([Z_cont_0, Z_one_hot_0, Z_cont_0 * Z_one_hot_0], axis=1)
    beta = np.random.normal(0, 1, Z_sub.shape[1])
    y = Z_sub @ beta + np.random.normal(0, 1, n)
    X_intr = ad.matrix.interaction(Z, {0: None}, levels)                               # cell 12
    pairs = X_intr._pairs
    pair_levels = levels[pairs]                                                        # cell 14
    is_cc = np.prod(pair_levels == 0, axis=1).astype(bool)
    cc = Z[:, pairs[is_cc][:, 0]] * Z[:, pairs[is_cc][:, 1]]
    centers, scales = np.zeros(X_intr.shape[1]), np.ones(X_intr.shape[1])
    centers[X_intr.groups[is_cc] + 2] = np.mean(cc, axis=0)
    scales[X_intr.groups[is_cc] + 2] = np.std(cc, axis=0, ddof=0)
    X_intr_std = ad.matrix.standardize(X_intr, centers=centers, scales=scales)
    X_one_hot = ad.matrix.one_hot(Z, levels)                                           # cell 16
    X = ad.matrix.concatenate([X_one_hot, X_intr_std], axis=1)
    groups = np.concatenate([X_one_hot.groups, X_one_hot.shape[1] + X_intr.groups])    # cell 18
    is_cd = np.logical_xor(pair_levels[:, 0], pair_levels[:, 1])
    pen = np.ones(len(X_intr.groups))
    pen[is_cc] = np.sqrt(3)
    pen[is_cd] = np.sqrt(2)
    penalty = np.concatenate([np.ones(len(X_one_hot.groups)), pen])
    st = ad.grpnet(X, ad.glm.gaussian(y), groups=groups, penalty=penalty, progress_bar=False)   # cell 20
    assert st.error == ""
    p_oh = X_one_hot.shape[1]
    first_intr = p_oh + st.betas[16, p_oh:].indices[0]                                 # cell 24
    rel = np.argmax(groups == first_intr) - len(X_one_hot.groups)
    return dict(n_lmdas=len(st.lmdas), dev=100 * st.devs[-1], support13=st.betas[13, :p_oh].indices.tolist(),
                first_pair=pairs[rel].tolist(), group_sizes=np.diff(np.append(groups, X.shape[1])), state=st)


def test_examples_notebook_through_the_front_door(hip):
    import test_reference_known_answers as ka

    out = _replay_examples_notebook_front_door()
    ka._check_examples(out)   # 100 lambdas, dev 71.1, support [0, 10..14] at 13, first pair [0, 10] at 16
    ref = ka._replay_examples_notebook(ad.matrix.dense)
    assert np.array_equal(out["group_sizes"], ref["group_sizes"])
    db = np.abs(out["state"].betas.toarray() - ref["state"].betas.toarray()).max()
    dd = np.abs(out["state"].devs - ref["state"].devs).max()
    print(f"front door vs dense replay: max|dbeta| = {db:.3e}, max|ddev| = {dd:.3e}")
    assert db < 1e-4
    assert np.allclose(out["state"].devs, ref["state"].devs, atol=1e-7)


# ---- 6. handles -----------------------------------------------------------------------------------------------------------
def _is_structured(X):
    return X._backend.fn("design_factor_groups")(X._handle, None, None, 0) >= 0


def test_cv_and_aliases_keep_the_structure(hip, monkeypatch, base_1031):
    b = base_1031
    monkeypatch.setenv("ADELIE_HIP_FACTOR_SWEEP", "1")
    X = ad.matrix.one_hot(b["Z"], LEVELS)
    y = b["E_oh"] @ np.random.RandomState(5).normal(size=78) + b["y"]
    kw = dict(n_folds=3, seed=0, groups=X.groups, lmda_path_size=20)
    cv = ad.cv_grpnet(X, ad.glm.gaussian(y), **kw)
    cv_ref = ad.cv_grpnet(ad.matrix.dense(b["E_oh"]), ad.glm.gaussian(y), **kw)
    assert np.allclose(cv.avg_losses, cv_ref.avg_losses)
    fit = cv.fit(X, ad.glm.gaussian(y), groups=X.groups, lmda_path_size=20)
    assert fit.error == "" and fit.counters["n_sweeps_factor"] > 0, fit.counters
    Xa = X.alias()
    assert _is_structured(X) and _is_structured(Xa)
    sa = ad.grpnet(Xa, ad.glm.gaussian(y), groups=X.groups, lmda_path_size=10, progress_bar=False)
    assert sa.error == "" and sa.counters["n_sweeps_factor"] > 0, sa.counters


def test_subset_and_concatenate_are_plain_dense_designs(hip, base_1031):
    b = base_1031
    X, E = ad.matrix.interaction(b["Z"], INTR_MAP, LEVELS), b["E_in"]
    rng = np.random.RandomState(2)
    v, w = rng.normal(size=1031), rng.uniform(0, 1, 1031)
    for Y, Ey in [(ad.matrix.subset(X, np.arange(3, 40), axis=1), E[:, 3:40]),
                  (ad.matrix.subset(X, np.array([5, 3, 200, 510]), axis=1), E[:, [5, 3, 200, 510]]),
                  (ad.matrix.concatenate([X, X], axis=1), np.concatenate([E, E], axis=1)),
                  (ad.matrix.subset(X, np.arange(0, 1031, 3), axis=0), E[::3])]:
        assert Y.shape == Ey.shape and not _is_structured(Y)
        vv, ww = (v, w) if Y.shape[0] == 1031 else (v[::3], w[::3])
        out = np.empty(Ey.shape[1])
        Y.mul(vv, ww, out)
        assert np.abs(out - (vv * ww) @ Ey).max() <= naive_tol(Ey, np.float64)
    # multi-response families run on the design as on any dense one
    K = 2
    yk = np.stack([b["y"], b["eta"]], axis=1)
    s = ad.grpnet(X, ad.glm.multigaussian(yk), lmda_path_size=5, progress_bar=False)
    s_ref = ad.grpnet(ad.matrix.dense(E), ad.glm.multigaussian(yk), lmda_path_size=5, progress_bar=False)
    assert s.error == "" and s.betas.shape[1] == 511 * K
    assert np.abs(s.betas.toarray() - s_ref.betas.toarray()).max() < 1e-8
