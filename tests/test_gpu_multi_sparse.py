"""Multi-response fits on a design kept sparse without expanding it (``kernels_multi_sparse.hip``): the view
``[1 (x) I_K, X (x) I_K]`` keeps the compressed columns as its base.  Paths against the expanded route
(``set_configs("multi_keep_sparse", False)``: the view over the dense copy) and against the CPU oracle."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adelie_amd as ad

pytestmark = pytest.mark.gpu

N, P, K = 300, 40, 3


@pytest.fixture(scope="module")
def problem():
    rng = np.random.RandomState(31)
    D = rng.normal(size=(N, P)) * (rng.uniform(size=(N, P)) < 0.15)
    B = np.zeros((P, K))
    B[rng.choice(P, 6, replace=False)] = 2 * rng.normal(size=(6, K))
    eta = D @ B
    Y = eta + 0.3 * rng.normal(size=(N, K))
    cls = np.eye(K)[np.argmax(eta + rng.gumbel(size=(N, K)), axis=1)]
    return D, Y, cls


def _csc(D):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ad.matrix.sparse(sp.csc_matrix(D), resident="csc")


@pytest.fixture
def expanded_route():
    """Calls its argument with the expanded route switched on, and always restores the default."""
    def run(f):
        ad.set_configs("multi_keep_sparse", False)
        try:
            return f()
        finally:
            ad.set_configs("multi_keep_sparse")
    return run


@pytest.mark.parametrize("family,kw", [
    ("multigaussian", dict()),
    ("multigaussian", dict(intercept=False)),
    ("multigaussian", dict(groups=np.arange(0, P, 4), alpha=0.6)),
    ("multinomial", dict()),
    ("multinomial", dict(intercept=False)),
])
def test_paths_agree_with_the_expanded_route(hip, problem, expanded_route, family, kw):
    D, Y, cls = problem
    glm = (lambda: ad.glm.multigaussian(Y)) if family == "multigaussian" else (lambda: ad.glm.multinomial(cls))
    kw = dict(kw, tol=1e-12, early_exit=False, lmda_path_size=10, min_ratio=0.1, progress_bar=False)
    if family == "multinomial":
        kw.update(irls_tol=1e-11)
    a = ad.grpnet(_csc(D), glm(), **kw)
    b = expanded_route(lambda: ad.grpnet(_csc(D), glm(), **kw))
    assert a.error == "" and b.error == ""
    tol = 1e-9 if family == "multigaussian" else 1e-7
    assert np.abs(a.betas.toarray() - b.betas.toarray()).max() < tol
    assert np.abs(a.intercepts - b.intercepts).max() < tol


def test_multigaussian_path_agrees_with_the_oracle(hip, oracle, problem):
    D, Y, _ = problem
    kw = dict(tol=1e-12, early_exit=False, lmda_path_size=12, min_ratio=0.05, progress_bar=False)
    a = ad.grpnet(_csc(D), ad.glm.multigaussian(Y), **kw)
    b = ad.grpnet(oracle.dense(np.asfortranarray(D)), ad.glm.multigaussian(Y), **kw)
    assert a.error == "" and b.error == ""
    assert np.abs(a.betas.toarray() - b.betas.toarray()).max() < 1e-9
    assert np.abs(a.intercepts - b.intercepts).max() < 1e-9


def test_the_view_keeps_the_sparse_base(hip, problem, expanded_route):
    Xs = _csc(problem[0])
    assert ad.matrix.kronecker_eye(Xs, 2)._base is Xs
    v = expanded_route(lambda: ad.matrix.kronecker_eye(Xs, 2))
    assert v._base is not Xs and v._base._kind == "dense"
    rng = np.random.RandomState(2)
    n, s, A = 24, 5, 3
    Xp = ad.matrix.snp_phased_calldata(rng.randint(0, 2, size=(n, 2 * s)).astype(np.int8),
                                       rng.randint(0, A, size=(n, 2 * s)).astype(np.int8), A)
    assert ad.matrix.kronecker_eye(Xp, 2)._base is Xp
    v = expanded_route(lambda: ad.matrix.kronecker_eye(Xp, 2))
    assert v._base is not Xp and v._base._kind == "dense"


def test_cv_grpnet_agrees_with_the_expanded_route(hip, problem, expanded_route):
    D, _, cls = problem
    kw = dict(n_folds=3, seed=1, lmda_path_size=8, min_ratio=0.1, progress_bar=False)
    a = ad.cv_grpnet(_csc(D), ad.glm.multinomial(cls), **kw)
    b = expanded_route(lambda: ad.cv_grpnet(_csc(D), ad.glm.multinomial(cls), **kw))
    assert np.abs(a.losses - b.losses).max() < 1e-7 * max(1.0, np.abs(b.losses).max())
