"""scikit-learn style estimator over the grpnet path — mirrors ``adelie.sklearn.GroupElasticNet`` (reference
``adelie/sklearn.py:43-250``): the same constructor parameters, fitted attributes (``glm_``, ``state_``, ``coef_``,
``intercept_``, ``lambda_``), error types and messages.  It is a thin caller of ``grpnet`` / ``cv_grpnet`` +
``CVGrpnetResult.fit`` + ``diagnostic.predict``; every numeric step runs on the device behind the C ABI.
``CSSModelSelection`` (``:253-464``) runs its swapping searches through ``solver.css_cov`` on one resident covariance."""
import numpy as np
from sklearn.base import BaseEstimator, RegressorMixin

from . import glm as _glm
from .cv import CVGrpnetResult, cv_grpnet
from .diagnostic import predict as _predict
from . import matrix as _matrix
from .solver import css_cov, grpnet

_FAMILIES = {
    "gaussian": _glm.gaussian,
    "binomial": _glm.binomial,
    "poisson": _glm.poisson,
    "multigaussian": _glm.multigaussian,
    "multinomial": _glm.multinomial,
}
_SOLVERS = {"grpnet": grpnet, "cv_grpnet": cv_grpnet}


class GroupElasticNet(BaseEstimator, RegressorMixin):
    """Group elastic net estimator.

    Parameters
    ----------
    solver : ``"grpnet"`` (whole path) or ``"cv_grpnet"`` (cross-validate, then refit down to the best lambda).
    family : ``"gaussian"``, ``"binomial"``, ``"poisson"``, ``"multigaussian"`` or ``"multinomial"``.
    """

    def __init__(self, solver: str = "grpnet", family: str = "gaussian"):
        self.solver = solver
        self.family = family

    def fit(self, X, y, **kwargs):
        """Fits the path (or the cross-validated model); ``kwargs`` go to the solver (reference ``sklearn.py:82-150``)."""
        self._validate_params()
        self.glm_ = _FAMILIES[self.family](y)
        self.state_ = _SOLVERS[self.solver](X=X, glm=self.glm_, **kwargs)
        if isinstance(self.state_, CVGrpnetResult):
            self.state_ = self.state_.fit(X=X, glm=self.glm_, **kwargs)
            self.coef_ = self.state_.betas[-1]
            self.intercept_ = np.array([self.state_.intercepts[-1]])
            self.lambda_ = np.array([self.state_.lmdas[-1]])
        else:
            self.coef_ = self.state_.betas
            self.intercept_ = self.state_.intercepts
            self.lambda_ = self.state_.lmdas
        return self

    def _linear(self, X):
        if not hasattr(self, "state_"):
            raise RuntimeError("The model has not been fitted yet. Call fit() first.")
        return _predict(X, self.coef_, self.intercept_)

    def predict_proba(self, X):
        """Class probabilities (binomial: two columns; multinomial: K), reference ``sklearn.py:152-186``."""
        if not hasattr(self, "state_"):
            raise RuntimeError("The model has not been fitted yet. Call fit() first.")
        if self.family not in ("binomial", "multinomial"):
            raise ValueError("predict_proba is only available for \"binomial\" and \"multinomial\" families.")
        eta = self._linear(X)
        if self.family == "binomial":
            pr = 0.5 * (1 + np.tanh(0.5 * eta))  # the logistic function, stable for either sign
            return np.stack((1 - pr, pr), axis=-1).squeeze()
        e = np.exp(eta - np.max(eta, axis=-1, keepdims=True))
        return (e / np.sum(e, axis=-1, keepdims=True)).squeeze()

    def predict(self, X):
        """Class labels for the binomial / multinomial families, linear predictions otherwise (``sklearn.py:188-214``)."""
        if self.family in ("binomial", "multinomial"):
            return np.argmax(self.predict_proba(X), axis=-1).squeeze()
        return self._linear(X).squeeze()

    def score(self, X, y):
        """R-squared of ``predict(X)`` clipped to [0, 1] (``sklearn.py:216-237``)."""
        yhat = self.predict(X)
        ss_res = np.sum((y - yhat) ** 2)
        ss_tot = np.sum((y - np.mean(y)) ** 2)
        return np.clip(1 - ss_res / ss_tot, 0, 1)

    def _validate_params(self):
        if self.solver not in _SOLVERS:
            raise ValueError(f"Unknown solver: {self.solver}")
        if self.family not in _FAMILIES:
            raise ValueError(f"Unknown family: {self.family}")


class CSSModelSelection(BaseEstimator, RegressorMixin):
    """Model selection by column subset selection (reference ``adelie.sklearn.CSSModelSelection``, ``sklearn.py:253-464``,
    and the per-``k`` routine of ``py_sklearn.cpp:16-141``): the finite-sample test for Gaussian features is run for
    ``k = 0, 1, ...`` until a subset of size ``k`` is not rejected at level ``alpha``; subsets are searched with the swapping
    method under the subset factor loss from ``n_inits`` random starts.

    Parameters
    ----------
    alpha : nominal level of the test.
    n_inits : random starts per ``k``.
    n_sims : Monte Carlo samples for the critical values.
    n_threads : accepted for signature parity.
    seed : seeds numpy's global generator for the chi-square draws and derives the seed of each ``k``'s starts exactly as the
        reference does.  The starts are drawn with ``numpy.random.RandomState`` seeded with the value the reference hands to
        ``std::mt19937``; ``RandomState.choice`` and ``std::sample`` consume the stream differently, so the starts themselves
        cannot equal the reference's (the searches started from them usually end in the same subset).

    All starts of every ``k`` run on one resident copy of ``S``; per start only the diagonal of the residual covariance and the
    ``(k, k)`` factor ``L_T`` come back to the host."""

    def __init__(self, alpha: float, n_inits: int = 1, n_sims: int = int(1e4), n_threads: int = 1, seed: int = None):
        self.alpha = alpha
        self.n_inits = n_inits
        self.n_sims = n_sims
        self.n_threads = n_threads
        self.seed = seed

    def fit(self, X, y=None):
        """Fits on the feature matrix ``X`` ``(n, p)``: ``fit_cov(X^T X / n, n)``.  ``y`` is unused."""
        X = np.asarray(X)
        n = X.shape[0]
        return self.fit_cov(X.T @ X / n, n)

    def _fit_k(self, S_dev, p, k, S_logdet, cutoff, n_inits, seed_k):
        """Smallest test statistic over up to ``n_inits`` random size-``k`` starts (stops at the first that does not reject)."""
        rng = np.random.RandomState(((int(seed_k) + 1) * 7 * n_inits) % 10007)
        best_T, best_subset = np.inf, np.empty(0, dtype=int)
        for _ in range(n_inits):
            start = np.sort(rng.choice(p, k, replace=False))
            state = css_cov(S_dev, subset=start, method="swapping", loss="subset_factor", max_iters=100000)
            T = -np.inf  # a failed solve counts as "not rejected", as the reference's catch-all does
            if state.error == "":
                rest = np.ones(p, dtype=bool)
                rest[state.subset] = False
                d = np.asarray(state.S_resid_diag, dtype=np.float64)[rest]
                if np.all(d > 0):
                    T = 2 * np.sum(np.log(np.diagonal(state.L_T).astype(np.float64))) - S_logdet + np.sum(np.log(d))
            if T < best_T:
                best_T, best_subset = T, np.array(state.subset, dtype=int)
            if not T > cutoff:
                break
        return best_T, best_subset

    def fit_cov(self, S, n: int):
        """Fits on a positive semi-definite ``(p, p)`` matrix ``S`` estimated from ``n`` samples (``sklearn.py:354-424``)."""
        S = np.asfortranarray(S)
        p = S.shape[1]
        assert p > 0 and n >= p
        S_logdet = np.linalg.slogdet(S)[1]
        if self.seed is not None:
            np.random.seed(self.seed)
        seeds = np.random.choice(int(1e7), p, replace=False)
        order = np.arange(1, p)
        chi2_1 = np.random.chisquare(order, (self.n_sims, order.size))
        chi2_2 = np.random.chisquare(n - p - 1 + order[::-1], (self.n_sims, order.size))
        S_dev = None
        best_subset = np.arange(p - 1)  # k = p - 1 never rejects
        for k in range(p - 1):
            ratio = chi2_1[:, :p - k - 1] / chi2_2[:, k + 1 - p:]
            cutoff = np.quantile(np.sum(np.log1p(ratio), axis=-1), 1 - self.alpha)
            if k == 0:
                T, subset = np.sum(np.log(np.diag(S))) - S_logdet, np.empty(0, dtype=int)
            else:
                if S_dev is None:
                    S_dev = _matrix.dense(S, method="cov", n_threads=self.n_threads)
                seed_k = seeds[k] if self.seed is None else (p * (k + 1) + self.seed) % 100007
                T, subset = self._fit_k(S_dev, p, k, S_logdet, cutoff, 1 if k == 1 else self.n_inits, seed_k)
            if not T > cutoff:
                best_subset = subset
                break
        self.subset_ = best_subset
        return self

    def score(self, X, y=None, sample_weight=None):
        """Negative subset factor loss of the fitted subset on ``X``: ``-(log|S_T| + sum log diag(S_rest | T))`` with
        ``S = X^T X / n`` (``-inf`` loss, i.e. ``+inf`` score, where it is undefined)."""
        X = np.asarray(X)
        n, p = X.shape
        T = np.asarray(self.subset_, dtype=int)
        rest = np.setdiff1d(np.arange(p), T)
        S = X.T @ X / n
        with np.errstate(all="ignore"):
            if T.size:
                S_TT = S[np.ix_(T, T)]
                resid = np.diag(S)[rest] - np.einsum("it,ti->i", S[np.ix_(rest, T)], np.linalg.solve(S_TT, S[np.ix_(T, rest)]))
                loss = np.linalg.slogdet(S_TT)[1] + np.sum(np.log(resid))
            else:
                loss = np.sum(np.log(np.diag(S)))
        return -(-np.inf if np.isnan(loss) else loss)
