"""glm.cox on the device: the family's kernels (adelie_hip_glm_cox_eval) against the numpy family, and grpnet / cv_grpnet with
the family evaluated on the device against the same family reached through the host-callback route (GlmBase64 subclass),
against a brute-force restatement (KKT) and against a Newton solve of the partial likelihood."""
import numpy as np
import pytest
import scipy.sparse

import adelie_amd as ad
from test_cox import brute, case

pytestmark = pytest.mark.gpu


def numpy_eval(fam, eta):
    n = len(eta)
    g = np.empty(n)
    h = np.empty(n)
    fam.gradient(eta, g)
    fam.hessian(eta, g, h)
    return g, h, float(fam.loss(eta))


def big_case(n, n_strata, ties, seed, dtype=np.float64, spread=None):
    rng = np.random.default_rng(seed)
    start = np.round(rng.exponential(1, n), 2)
    stop = start + np.round(rng.exponential(2, n), 2) + 0.01
    if ties:  # stop times rounded to `ties` distinct values: tie groups of ~n / ties rows straddling many tiles
        grid = np.linspace(0.5, 8, ties)
        stop = grid[np.minimum(np.searchsorted(grid, stop), ties - 1)]
        start = np.minimum(start, stop - 0.25)
    status = (rng.uniform(size=n) > 0.3).astype(dtype)
    if n_strata == "pairs":
        strata = np.arange(n) // 2
    else:
        strata = rng.integers(0, n_strata, n)
        strata = np.unique(strata, return_inverse=True)[1]
    w = rng.uniform(0.5, 2, n) * (rng.uniform(size=n) > 0.05)
    eta = rng.normal(0, 1, n)
    if spread is not None:  # exp(eta) of stratum 1 larger by `spread` than stratum 0's
        eta = eta + np.log(spread) * (strata == 1)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w, dtype=dtype)
    return fam, eta.astype(dtype)


def assert_close(a, b, rtol, floor):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.max(np.abs(b)), floor)
    err = np.max(np.abs(a - b))
    assert err <= rtol * scale, (err, scale)


EVAL_CASES = [
    (1, 1, 0), (2, 1, 0), (2, 1, 1), (1000, 1, 0), (1000, 7, 10), (1000, "pairs", 0),
    (200_003, 1, 10), (200_003, 7, 0), (200_003, "pairs", 10), (1_000_000, 1, 10), (1_000_000, 7, 0),
    (1_000_000, "pairs", 0),
]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,ns,ties", EVAL_CASES)
def test_device_eval_matches_numpy(hip, n, ns, ties, dtype):
    fam, eta = big_case(n, ns, ties, seed=n % 97, dtype=dtype)
    rtol = 1e-12 if dtype == np.float64 else 1e-5
    g, h, lo = fam._device_eval(eta)
    gr, hr, lr = numpy_eval(fam, eta)
    floor = float(fam.weights.max())
    assert_close(g, gr, rtol, floor)
    assert_close(h, hr, rtol, floor)
    assert_close(lo, lr, rtol, 1.0)
    g2, h2, lo2 = fam._device_eval(eta)
    assert np.array_equal(g, g2) and np.array_equal(h, h2) and lo == lo2  # deterministic: bit-identical


@pytest.mark.parametrize("tie_method", ["efron", "breslow"])
def test_device_eval_strata_of_very_different_magnitude(hip, tie_method):
    fam, eta = big_case(50_000, 2, 10, seed=5, spread=1e8)
    fam = fam.reweight(fam.weights) if tie_method == "efron" else ad.glm.cox(
        fam.start, fam.stop, fam.status, strata=fam.strata, weights=fam.weights, tie_method="breslow")
    g, h, lo = fam._device_eval(eta)
    gr, hr, lr = numpy_eval(fam, eta)
    for m in (0, 1):  # each stratum on its own scale
        s = fam.strata == m
        assert_close(g[s], gr[s], 1e-12, float(fam.weights[s].max()))
        assert_close(h[s], hr[s], 1e-12, float(fam.weights[s].max()))
    assert_close(lo, lr, 1e-12, 1.0)


def test_device_eval_matches_brute_force(hip):
    start, stop, status, strata, w, eta = case(300, 21, n_strata=4, n_times=6, zero_w=0.1)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    g, h, lo = fam._device_eval(eta)
    lr, gr, hr, _ = brute(start, stop, status, strata, fam.weights, "efron", eta)
    floor = float(fam.weights.max())
    assert_close(g, gr, 1e-12, floor)
    assert_close(h, hr, 1e-12, floor)
    assert_close(lo, lr, 1e-12, 1.0)


class CoxByCallback(ad.glm.GlmBase64):
    """The same family as a user-defined GLM: the solver reaches it through host callbacks."""

    def __init__(self, fam):
        self.fam = fam
        ad.glm.GlmBase64.__init__(self, "cox_cb", fam.status, fam.weights)

    def gradient(self, eta, grad):
        self.fam.gradient(eta, grad)

    def hessian(self, eta, grad, hess):
        self.fam.hessian(eta, grad, hess)

    def loss(self, eta):
        return self.fam.loss(eta)

    def loss_full(self):
        return self.fam.loss_full()


def design(kind, Xd, seed):
    if kind == "dense":
        return ad.matrix.dense(np.asfortranarray(Xd))
    if kind == "sparse":
        return ad.matrix.sparse(scipy.sparse.csc_matrix(Xd), resident="csc")
    if kind == "std":
        return ad.matrix.standardize(ad.matrix.dense(np.asfortranarray(Xd)), lazy=True)
    raise ValueError(kind)


def snp_data(n, p, seed):
    rng = np.random.default_rng(seed)
    cd = rng.choice([0, 1, 2, -9], size=(n, p), p=[0.6, 0.25, 0.1, 0.05]).astype(np.int8)
    valid = cd >= 0
    imp = np.where(valid, cd, 0).sum(0) / np.maximum(valid.sum(0), 1)
    return np.asfortranarray(cd), np.where(valid, cd, imp[None]).astype(np.float64)


def path_pair(Xa, Xb, fam, **kw):
    kw = dict(progress_bar=False, **kw)
    s_dev = ad.grpnet(Xa, fam, **kw)
    s_cb = ad.grpnet(Xb, CoxByCallback(fam), **kw)
    assert s_dev.error == "" and s_cb.error == "", (s_dev.error, s_cb.error)
    return s_dev, s_cb


def assert_same_path(s_dev, s_cb, tol=1e-9):
    """Same lambdas and solutions.  The two routes round the family differently (summation order), so an IRLS loop may stop
    one iteration apart at some lambda: `tol` bounds that, not the family."""
    assert len(s_dev.lmdas) == len(s_cb.lmdas) and len(s_dev.lmdas) > 1
    np.testing.assert_allclose(s_dev.lmdas, s_cb.lmdas, rtol=1e-12)
    db = np.abs(s_dev.betas.toarray() - s_cb.betas.toarray()).max()
    assert db <= tol, db
    # the Cox loss is shift-invariant: the intercept's gradient is identically zero and its value is whatever rounding leaves
    # after the first IRLS step; the two routes may differ by a constant, which no prediction or loss can see
    di = np.asarray(s_dev.intercepts) - np.asarray(s_cb.intercepts)
    assert np.ptp(di[1:]) <= tol if len(di) > 2 else True
    assert np.abs(di).max() <= 1e-4
    np.testing.assert_allclose(s_dev.devs, s_cb.devs, rtol=0, atol=tol / 10)


PATH_CASES = [
    dict(kind="dense", gs=1, alpha=1.0, intercept=True, tie="efron", strata=1),
    dict(kind="dense", gs=5, alpha=0.5, intercept=False, tie="breslow", strata=3, pf=True, offsets=True),
    dict(kind="snp", gs=1, alpha=1.0, intercept=True, tie="breslow", strata=1),
    dict(kind="snp", gs=5, alpha=0.5, intercept=False, tie="efron", strata=2),
    dict(kind="sparse", gs=1, alpha=1.0, intercept=True, tie="efron", strata=2, offsets=True),
    dict(kind="sparse", gs=5, alpha=1.0, intercept=False, tie="breslow", strata=1, pf=True),
    dict(kind="std", gs=1, alpha=1.0, intercept=True, tie="efron", strata=3),
    dict(kind="std", gs=1, alpha=0.5, intercept=True, tie="breslow", strata=1, pf=True),
]


@pytest.mark.parametrize("c", PATH_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_path_parity_with_callback_route(hip, c):
    n, p = 400, 40
    rng = np.random.default_rng(PATH_CASES.index(c))
    if c["kind"] == "snp":
        cd, Xd = snp_data(n, p, 1)
        Xa, Xb = ad.matrix.snp_calldata(cd), ad.matrix.snp_calldata(cd)
    else:
        Xd = rng.normal(0, 1, (n, p))
        if c["kind"] == "sparse":
            Xd = Xd * (rng.uniform(size=(n, p)) < 0.2)
        Xa, Xb = design(c["kind"], Xd, 0), design(c["kind"], Xd, 0)
    beta = rng.normal(0, 1, p) * (rng.uniform(size=p) < 0.2)
    Xs = (Xd - Xd.mean(0)) / np.maximum(Xd.std(0), 1e-12)
    eta_true = Xs @ beta * 0.3
    start = np.round(rng.exponential(1, n), 1)
    stop = start + np.round(np.exp(-eta_true + rng.normal(0, 1, n)), 1) + 0.1
    status = (rng.uniform(size=n) > 0.25).astype(float)
    strata = rng.integers(0, c["strata"], n)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=rng.uniform(0.5, 1.5, n), tie_method=c["tie"])
    G = p // c["gs"]
    kw = dict(groups=np.arange(G) * c["gs"], alpha=c["alpha"], intercept=c["intercept"], lmda_path_size=30,
              early_exit=False, tol=1e-12, irls_tol=1e-12)
    if c.get("pf"):
        kw["penalty"] = rng.uniform(0.5, 2, G)
    if c.get("offsets"):
        kw["offsets"] = rng.normal(0, 0.2, n)
    s_dev, s_cb = path_pair(Xa, Xb, fam, **kw)
    assert_same_path(s_dev, s_cb, tol=1e-7)


def test_path_parity_warm_start_and_constraint(hip):
    n, p = 300, 20
    start, stop, status, strata, w, _ = case(n, 31, n_strata=2, n_times=8)
    X = np.random.default_rng(2).normal(0, 1, (n, p))
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    kw = dict(lmda_path_size=20, early_exit=False, tol=1e-12, irls_tol=1e-12)
    a, b = path_pair(ad.matrix.dense(np.asfortranarray(X)), ad.matrix.dense(np.asfortranarray(X)), fam, **kw)
    assert_same_path(a, b, tol=1e-7)
    # warm start from the 10th saved lambda on, continuing the path
    lm = a.lmdas[9:]
    a2 = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), fam, warm_start=a, lmda_path=lm, progress_bar=False, **kw)
    b2 = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), CoxByCallback(fam), warm_start=b, lmda_path=lm,
                   progress_bar=False, **kw)
    assert_same_path(a2, b2, tol=1e-7)
    cons = [ad.constraint.lower(np.zeros(1)) if j % 3 == 0 else None for j in range(p)]
    a3 = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), fam, constraints=cons, progress_bar=False, **kw)
    cons = [ad.constraint.lower(np.zeros(1)) if j % 3 == 0 else None for j in range(p)]
    b3 = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), CoxByCallback(fam), constraints=cons, progress_bar=False, **kw)
    assert_same_path(a3, b3, tol=1e-7)
    B = a3.betas.toarray()
    assert np.all(B[:, ::3] >= -1e-12)


def test_no_host_callback_during_solve(hip):
    """The numpy members wrapped in counting spies: `hessian` is never called and `gradient` once, by the preamble."""
    n, p = 500, 30
    start, stop, status, strata, w, _ = case(n, 41, n_strata=2, n_times=10)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    calls = {"gradient": 0, "hessian": 0, "loss": 0}
    for name in calls:
        f = getattr(fam, name)

        def spy(*a, _f=f, _n=name):
            calls[_n] += 1
            return _f(*a)
        setattr(fam, name, spy)
    X = np.asfortranarray(np.random.default_rng(0).normal(0, 1, (n, p)))
    s = ad.grpnet(ad.matrix.dense(X), fam, lmda_path_size=20, progress_bar=False)
    assert s.error == "" and len(s.lmdas) > 1
    assert calls == {"gradient": 1, "hessian": 0, "loss": 0}, calls


def test_kkt_against_brute_force_gradient(hip):
    n, p = 300, 15
    start, stop, status, strata, w, _ = case(n, 51, n_strata=3, n_times=12)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    X = np.random.default_rng(3).normal(0, 1, (n, p))
    s = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), fam, lmda_path_size=25, early_exit=False, tol=1e-12,
                  irls_tol=1e-12, intercept=False, progress_bar=False)
    B = s.betas.toarray()
    for k, lm in enumerate(s.lmdas):
        eta = X @ B[k]
        _, g, _, _ = brute(start, stop, status, strata, fam.weights, "efron", eta)
        xg = X.T @ g
        act = B[k] != 0
        assert np.all(np.abs(xg[~act]) <= lm * (1 + 1e-4)), k
        assert np.allclose(xg[act], lm * np.sign(B[k][act]), rtol=0, atol=1e-4 * lm), k


def test_unpenalised_limit_matches_newton_solve(hip):
    import scipy.optimize

    n, p = 300, 5
    rng = np.random.default_rng(61)
    X = rng.normal(0, 1, (n, p))
    b_true = np.array([0.8, -0.5, 0.3, 0.0, 0.2])
    start = np.round(rng.exponential(0.5, n), 2)
    stop = start + np.round(rng.exponential(np.exp(-X @ b_true)), 2) + 0.01
    status = (rng.uniform(size=n) > 0.2).astype(float)
    strata = rng.integers(0, 2, n)
    fam = ad.glm.cox(start, stop, status, strata=strata)
    s0 = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), fam, lmda_path_size=0, progress_bar=False, intercept=False)
    path = s0.lmda_max * np.logspace(0, -9, 40)
    s = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), fam, lmda_path=path, early_exit=False, tol=1e-14,
                  irls_tol=1e-14, intercept=False, progress_bar=False)
    assert s.error == "" and len(s.lmdas) == 40
    bd = s.betas.toarray()[-1]

    def f(b):
        loss, g, _, _ = brute(start, stop, status, strata, fam.weights, "efron", X @ b)
        return loss, -(X.T @ g)
    res = scipy.optimize.minimize(f, np.zeros(p), jac=True, method="BFGS", options=dict(gtol=1e-12, maxiter=1000))
    assert np.max(np.abs(bd - res.x)) <= 1e-6, (bd, res.x)


def test_f32_path_matches_f64(hip):
    n, p = 2000, 40
    rng = np.random.default_rng(71)
    X = rng.normal(0, 1, (n, p))
    X = (X - X.mean(0)) / X.std(0)
    beta = rng.normal(0, 1, p) * (rng.uniform(size=p) < 0.2)
    # times on a 1/8 grid: exact in f32, so both dtypes see the same tie groups and risk sets
    start = np.round(rng.exponential(1, n) * 8) / 8
    stop = start + np.round(np.exp(-0.3 * X @ beta + rng.normal(0, 1, n)) * 8) / 8 + 0.125
    status = (rng.uniform(size=n) > 0.3).astype(float)
    kw = dict(lmda_path_size=20, early_exit=False, progress_bar=False)
    s64 = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), ad.glm.cox(start, stop, status), **kw)
    s32 = ad.grpnet(ad.matrix.dense(np.asfortranarray(X, dtype=np.float32)),
                    ad.glm.cox(start, stop, status.astype(np.float32)), **kw)
    assert len(s32.lmdas) == len(s64.lmdas)
    # the deviance agrees to 1e-4; the coefficients to 1e-2 of the largest (the f32 IRLS stops at its own resolution)
    np.testing.assert_allclose(s32.devs, s64.devs, rtol=1e-4, atol=1e-6)
    B64, B32 = s64.betas.toarray(), s32.betas.toarray()
    assert np.max(np.abs(B32 - B64)) <= 1e-2 * max(np.max(np.abs(B64)), 1.0)


def test_cv_grpnet_cox(hip, monkeypatch):
    n, p = 600, 30
    start, stop, status, strata, w, _ = case(n, 81, n_strata=2, n_times=15)
    X = np.asfortranarray(np.random.default_rng(4).normal(0, 1, (n, p)))
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    kw = dict(n_folds=4, lmda_path_size=15, seed=0)
    r1 = ad.cv_grpnet(ad.matrix.dense(X), fam, **kw)
    r2 = ad.cv_grpnet(ad.matrix.dense(X), fam, **kw)
    assert np.all(np.isfinite(r1.losses))
    assert np.array_equal(r1.losses, r2.losses)  # bit-identical reruns
    monkeypatch.setenv("ADELIE_HIP_CV_SOLVE_MANY", "0")
    r3 = ad.cv_grpnet(ad.matrix.dense(X), fam, **kw)
    np.testing.assert_allclose(r3.losses, r1.losses, rtol=1e-10, atol=1e-12)
    # the sequential fold loop (one fold at a time) computes the same losses
    r4 = ad.cv_grpnet(ad.matrix.dense(X), fam, n_concurrent=1, **kw)
    np.testing.assert_allclose(r4.losses, r1.losses, rtol=1e-10, atol=1e-12)
    # predict / coefficient / diagnostic on a Cox state
    s = r1.fit(ad.matrix.dense(X), fam, lmda_path_size=15, progress_bar=False)
    assert s.error == ""
    eta = ad.diagnostic.predict(ad.matrix.dense(X), s.betas, s.intercepts)
    assert eta.shape == (len(s.lmdas), n)
    np.testing.assert_allclose(eta[-1], X @ s.betas[-1].toarray().ravel() + s.intercepts[-1], atol=1e-10)
    b, b0 = ad.diagnostic.coefficient(lmda=s.lmdas[-1], betas=s.betas, intercepts=s.intercepts, lmdas=s.lmdas)
    assert b.shape == (1, p)
    ad.diagnostic.diagnostic(s)


def test_large_path_completes(hip):
    import torch

    n, p = 200_000, 5_000
    torch.manual_seed(0)
    Xt = torch.randn(n, p, device="cuda", dtype=torch.float64).t().contiguous().t()  # column-major on the device
    rng = np.random.default_rng(91)
    start = np.round(rng.exponential(1, n), 1)
    stop = start + np.round(rng.exponential(2, n), 1) + 0.1
    status = (rng.uniform(size=n) > 0.3).astype(np.float64)
    strata = rng.integers(0, 3, n)
    fam = ad.glm.cox(start, stop, status, strata=strata)
    s = ad.grpnet(ad.matrix.dense(Xt), fam, lmda_path_size=50, early_exit=False, tol=1e-10, progress_bar=False)
    assert s.error == "" and len(s.lmdas) == 50
    b = s.betas[-1].toarray().ravel()
    eta = (Xt @ torch.from_numpy(b).cuda()).cpu().numpy()
    g = np.empty(n)
    fam.gradient(eta, g)  # the numpy family at the solution
    xg = (Xt.t() @ torch.from_numpy(g).cuda()).cpu().numpy()
    lm = s.lmdas[-1]
    act = b != 0
    assert np.all(np.abs(xg[~act]) <= lm * 1.01)
    assert np.allclose(xg[act], lm * np.sign(b[act]), atol=0.01 * lm)
