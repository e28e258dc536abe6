"""css_cov on the device against the numpy restatement of tests/css_checks.py (itself checked against brute force in
test_css_host.py).  Subsets must agree exactly wherever no decision of the restatement hangs on rounding; S_resid and L_T must
be as close to a longdouble (float32: float64) run of the restatement as a correct implementation in the format can be
expected to be: within 8x the restatement's own error in that format (another operation order) plus eps * max|S|."""
import os
import sys

import numpy as np
import pytest

import adelie_amd as ad

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import css_checks as cc  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [("wishart", p, k) for p, k in [(1, 1), (5, 0), (5, 1), (5, 3), (5, 5), (20, 5)]] + \
         [("cluster", p, k) for p, k in [(67, 7), (130, 9), (257, 12)]] + [("cluster", 20, 5)]
METHODS = ("greedy", "swapping", "swapping_tail")
SEEDS = range(3)
GAP64 = 1e-9
# above p * updates * eps_f32 ~ 257 * 40 * 6e-8 ~ 6e-4
GAP32 = 1e-3


def solve(S, k, loss, method):
    if method == "greedy":
        return ad.css_cov(S, k, method="greedy", loss=loss)
    if method == "swapping":
        return ad.css_cov(S, k, method="swapping", loss=loss)
    p = S.shape[0] if isinstance(S, np.ndarray) else S.cols()
    return ad.css_cov(S, subset=np.arange(p - k, p), method="swapping", loss=loss)


def lower_err(a, b):
    if a.size == 0 and b.size == 0:
        return 0.0
    assert a.shape == b.shape
    i = np.tril_indices(a.shape[0])
    return float(np.max(np.abs(a[i].astype(np.longdouble) - b[i].astype(np.longdouble))))


def check_close(state, own, truth, S, eps):
    """state vs truth within 8x (own vs truth) + eps * max|S|, for S_resid (lower triangle) and L_T."""
    scale = float(np.max(np.abs(S)))
    if truth.S_resid is None:
        assert state.S_resid.shape == (0, 0) and state.L_T.shape == (0, 0)
        return
    e_own = lower_err(np.asarray(own.S_resid), np.asarray(truth.S_resid))
    e_dev = lower_err(state.S_resid, np.asarray(truth.S_resid))
    print(f"S_resid: device {e_dev:.3e}, restatement {e_own:.3e}, eps*max|S| {eps * scale:.3e}")
    assert e_dev <= 8 * e_own + eps * scale
    assert np.array_equal(state.S_resid, state.S_resid.T)
    if truth.L_T is not None:
        e_own = lower_err(np.asarray(own.L_T), np.asarray(truth.L_T))
        e_dev = lower_err(state.L_T, np.asarray(truth.L_T))
        print(f"L_T: device {e_dev:.3e}, restatement {e_own:.3e}")
        assert e_dev <= 8 * e_own + eps * scale
        assert state.L_T.shape == truth.L_T.shape


@pytest.mark.parametrize("gen, p, k", SHAPES)
@pytest.mark.parametrize("loss", cc.LOSSES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("seed", SEEDS)
def test_float64_grid(gen, p, k, loss, method, seed):
    S = cc.make_input(gen, p, k, seed)
    own = cc.cached_run(gen, p, k, seed, loss, method, "float64")
    if 0 < k < p:  # on every such case the restatement's decisions are clear of rounding (smallest gap 2e-7): none is skipped
        assert own.min_gap >= GAP64
    state = solve(S, k, loss, method)
    assert state.error == own.error == ""
    assert state.subset.dtype == np.int64 and state.subset.shape == (k,)
    if k == p:  # the last picks are made on a residual of pure rounding (subset_factor: exact ties)
        assert sorted(state.subset) == list(range(p))
    if own.min_gap < GAP64:
        return
    assert list(state.subset) == list(own.subset)
    truth = cc.cached_run(gen, p, k, seed, loss, method, "longdouble")
    assert list(truth.subset) == list(own.subset)
    assert state.S_resid.dtype == np.float64
    check_close(state, own, truth, S, np.finfo(np.float64).eps)
    assert state.n_updates == own.n_updates and state.n_swaps == own.n_swaps


def qualifies32(gen, p, k, seed, loss, method):
    return cc.cached_run(gen, p, k, seed, loss, method, "float64", True).min_gap >= GAP32


def test_float32_grid_is_not_empty():
    """Skipping may not hide a failure: the small wishart cases all qualify under least_squares and min_det, and every loss
    and method keeps at least one cluster case of more than one wavefront."""
    for gen, p, k in SHAPES:
        if gen == "wishart" and p <= 5:
            for loss in ("least_squares", "min_det"):
                for method in METHODS:
                    for seed in SEEDS:
                        assert qualifies32(gen, p, k, seed, loss, method), (p, k, loss, method, seed)
    for loss in cc.LOSSES:
        for method in ("greedy", "swapping_tail"):
            assert any(qualifies32(gen, p, k, seed, loss, method)
                       for gen, p, k in SHAPES if gen == "cluster" and p >= 67 for seed in SEEDS), (loss, method)


@pytest.mark.parametrize("gen, p, k", SHAPES)
@pytest.mark.parametrize("loss", cc.LOSSES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("seed", SEEDS)
def test_float32_grid(gen, p, k, loss, method, seed):
    if not qualifies32(gen, p, k, seed, loss, method):
        return  # a decision within float32 rounding of a tie: nothing to compare (test_float32_grid_is_not_empty)
    S32 = cc.make_input(gen, p, k, seed).astype(np.float32)
    truth = cc.cached_run(gen, p, k, seed, loss, method, "float64", True)
    own = cc.cached_run(gen, p, k, seed, loss, method, "float32", True)
    state = solve(S32, k, loss, method)
    assert state.error == truth.error == ""
    if k == p:
        assert sorted(state.subset) == list(range(p))
    else:
        assert list(state.subset) == list(truth.subset)
    if list(own.subset) != list(truth.subset):
        return  # the float32 restatement itself went another way: no error estimate for this case
    if truth.S_resid is not None:
        assert state.S_resid.dtype == np.float32
    check_close(state, own, truth, S32, np.finfo(np.float32).eps)


def test_inputs_agree():
    gen, p, k, seed, loss = "cluster", 67, 7, 1, "least_squares"
    S = cc.make_input(gen, p, k, seed)
    own = cc.cached_run(gen, p, k, seed, loss, "swapping", "float64")
    resident = ad.matrix.dense(S, method="cov")
    states = [ad.css_cov(np.asfortranarray(S), k, loss=loss), ad.css_cov(np.ascontiguousarray(S), k, loss=loss),
              ad.css_cov(resident, k, loss=loss)]
    for st in states:
        assert st.error == ""
        assert list(st.subset) == list(own.subset)
        assert np.array_equal(st.S_resid, states[0].S_resid)
    back = np.empty((p, p), order="F")
    resident.to_dense(0, p, back)
    assert np.array_equal(back, S)

    X = np.asfortranarray(np.linalg.cholesky(S).T)  # a (p, p) design with X^T X = S up to rounding
    A = ad.matrix.lazy_cov(ad.matrix.dense(X))
    G = np.empty((p, p), order="F")
    A.to_dense(0, p, G)
    before = G.copy()
    want = cc.run(G, k, loss, "swapping", np.float64)
    assert want.min_gap >= GAP64
    got = ad.css_cov(A, k, loss=loss)
    assert got.error == "" and list(got.subset) == list(want.subset) == list(own.subset)
    check_close(got, want, cc.run(G, k, loss, "swapping", np.longdouble), G, np.finfo(np.float64).eps)
    A.to_dense(0, p, G)
    assert np.array_equal(G, before)


def test_reproducible():
    S = cc.make_input("cluster", 257, 12, 0)
    a = ad.css_cov(S, 12, loss="subset_factor")
    b = ad.css_cov(S, 12, loss="subset_factor")
    assert np.array_equal(a.subset, b.subset)
    assert np.array_equal(a.S_resid, b.S_resid)
    assert np.array_equal(a.L_T, b.L_T)


@pytest.mark.parametrize("loss", cc.LOSSES)
def test_swapping_trivial_sizes_return_the_input(loss):
    S = cc.wishart(5, 0)
    st = ad.css_cov(S, subset=np.empty(0, dtype=int), method="swapping", loss=loss)
    assert st.subset.size == 0 and st.error == "" and st.n_updates == 0
    start = np.array([3, 1, 4, 0, 2])
    st = ad.css_cov(S, subset=start, method="swapping", loss=loss)
    assert list(st.subset) == list(start) and st.error == "" and st.n_updates == 0


def test_zero_column_is_never_selected():
    S = cc.wishart(8, 1)
    S[:, 2] = 0
    S[2, :] = 0
    st = ad.css_cov(S, 3, method="greedy", loss="least_squares")
    own = cc.greedy(S, 3, "least_squares", np.float64)
    assert 2 not in st.subset
    assert list(st.subset) == list(own.subset)


def test_dependent_initial_subset_is_reported():
    X = np.random.RandomState(0).normal(size=(30, 6))
    X[:, 4] = X[:, 1]
    S = np.asfortranarray(X.T @ X / 30)
    st = ad.css_cov(S, subset=[1, 4], method="swapping", loss="least_squares")  # logged, not raised
    assert "Initial subset are not linearly independent columns." in st.error
    assert cc.swapping(S, [1, 4], "least_squares", np.float64).error != ""


def _needs_second_cycle():
    """A case of the grid whose swapping search (explicit start) is still swapping in its second cycle."""
    for gen, p, k in SHAPES:
        for seed in SEEDS:
            if 0 < k < p:
                r = cc.cached_run(gen, p, k, seed, "least_squares", "swapping_tail", "float64")
                if r.n_cycles >= 2 and r.error == "":
                    return gen, p, k, seed
    raise AssertionError("no case of the grid needs a second cycle")


def test_max_iters_is_reported():
    gen, p, k, seed = _needs_second_cycle()
    S = cc.make_input(gen, p, k, seed)
    st = ad.css_cov(S, subset=np.arange(p - k, p), method="swapping", loss="least_squares", max_iters=1)
    assert "Maximum swapping cycles reached!" in st.error
    assert st.error.startswith("adelie_core solver: ")
    want = cc.swapping(S, np.arange(p - k, p), "least_squares", np.float64, max_iters=1)
    assert want.error != "" and list(st.subset) == list(want.subset)
    assert st.n_updates == want.n_updates


@pytest.mark.parametrize("method", METHODS)
def test_n_updates_counts_the_passes(method):
    gen, p, k, seed, loss = "cluster", 130, 9, 2, "min_det"
    own = cc.cached_run(gen, p, k, seed, loss, method, "float64")
    st = solve(cc.make_input(gen, p, k, seed), k, loss, method)
    assert st.n_updates == own.n_updates > 0
    assert st.n_swaps == own.n_swaps


def test_block_diag_input():
    S = cc.make_input("cluster", 20, 5, 0)
    A = ad.matrix.block_diag([S[:8, :8], S[8:, 8:]], method="cov")
    full = np.zeros((20, 20), order="F")
    full[:8, :8], full[8:, 8:] = S[:8, :8], S[8:, 8:]
    want = cc.run(full, 4, "least_squares", "swapping", np.float64)
    assert want.min_gap >= GAP64
    assert list(ad.css_cov(A, 4).subset) == list(want.subset)


@pytest.mark.parametrize("s, planted", [(100, [5, 7, 10]), (102, [2, 7, 10])])
def test_model_selection_finds_the_planted_columns(s, planted):
    rng = np.random.RandomState(s)
    n, p, k = 400, 12, 3
    F = rng.normal(size=(n, k))
    B = rng.normal(size=(k, p - k))
    X = np.hstack([F, F @ B + 0.5 * rng.normal(size=(n, p - k))])[:, rng.permutation(p)]
    m = ad.sklearn.CSSModelSelection(alpha=0.05, n_inits=3, n_sims=2000, seed=s - 100).fit(X)
    assert sorted(m.subset_) == planted
    assert np.isfinite(m.score(X))
