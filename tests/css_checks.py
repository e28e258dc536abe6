"""Yardsticks for ``css_cov`` (helper module, not a test).

* a numpy restatement of the search (scores per loss with the reference's guards, the full symmetric rank-one update, greedy,
  swapping with the reference's stopping rules) that runs in any ``dtype`` -- ``float32`` / ``float64`` to estimate the error a
  correct implementation in that format makes, ``np.longdouble`` as the truth.  The ``k x k`` solves of swapping are done in
  ``float64``, or in the run's dtype when that is wider (so that the ``longdouble`` run is a truth for them too).  Every
  decision records the relative gap ``(top1 - top2) / |top1|`` of the masked scores: a comparison against another
  implementation is meaningful only where no decision hangs on rounding;
* a brute-force evaluation of the three losses straight from their definitions, with the greedy and swapping searches on
  top of it (what the reference's own tests compare against);
* the two input generators of the tests.
"""
import functools

import numpy as np

EPS = 1e-10
LOSSES = ("least_squares", "subset_factor", "min_det")


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def wishart(p, seed):
    X = np.random.RandomState(seed).normal(size=(2 * p, p))
    return np.asfortranarray(X.T @ X / p)


def cluster(p, k, seed):
    """k latent factors, every column one factor plus noise whose scale grows with the column's block: wide score gaps."""
    rng = np.random.RandomState(seed)
    n = 4 * p
    Z = rng.normal(size=(n, k))
    E = rng.normal(size=(n, p))
    X = np.empty((n, p))
    for i in range(p):
        X[:, i] = Z[:, i % k] + 0.3 * 1.3 ** (i // k) * E[:, i]
    return np.asfortranarray(X.T @ X / n)


def make_input(gen, p, k, seed):
    return wishart(p, seed) if gen == "wishart" else cluster(p, k, seed)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def scores(S, member, loss):
    """Scores of all columns of the residual covariance ``S`` (in ``S.dtype``) and the early-exit flag.  Members get the lowest
    score.  For ``subset_factor`` every column is evaluated; the reference stops at the first ``+inf``, which gives the same
    arg-max (the lowest-index ``+inf``) and the same swap decision."""
    dtype = S.dtype.type
    p = S.shape[0]
    d = np.diagonal(S).copy()
    eps = dtype(EPS)
    if loss == "least_squares":
        out = np.zeros(p, dtype=dtype)
        ok = ~member & (d > 0)
        out[ok] = np.sum(S[:, ok] * S[:, ok], axis=0) / d[ok]
        return out, False
    if loss == "min_det":
        out = -np.maximum(d, dtype(0))
        for j in range(p):
            if not member[j] and out[j] >= -eps:
                out[j] = 0
                return out, True
        return out, False
    out = np.full(p, -np.inf, dtype=dtype)
    early = False
    rows = ~member
    for j in np.flatnonzero(~member):
        if d[j] <= 0:
            out[j] = np.inf
            early = True
            continue
        sel = rows.copy()
        sel[j] = False
        r = d[sel] - S[sel, j] * S[sel, j] / d[j]
        if np.any(r <= eps):
            out[j] = np.inf
            early = True
        else:
            out[j] = -np.log(d[j]) - np.sum(np.log(r))
    return out, early


def masked_argmax(sc, member):
    """Arg-max over the non-members (ties to the lowest index) and the relative gap to the runner-up."""
    m = np.where(member, -np.inf, sc)
    star = int(np.argmax(m))
    top1 = m[star]
    rest = np.delete(m, star)
    top2 = rest.max() if rest.size else -np.inf
    if not np.isfinite(top1) or not np.isfinite(top2):
        gap = np.inf if top1 > top2 else 0.0
    elif top1 == 0:
        gap = np.inf if top1 > top2 else 0.0
    else:
        gap = float((top1 - top2) / abs(top1))
    return star, gap


def rank_one(S, beta, c):
    """``S += c * beta beta^T`` on the full symmetric matrix, in ``S.dtype``."""
    S += S.dtype.type(c) * np.outer(beta, beta)


def fwd(S, i):
    """Adds column ``i`` to the set: no-op on a non-positive diagonal, as ``update_cov_resid_fwd``."""
    if S[i, i] <= 0:
        return
    beta = S[:, i].copy()
    rank_one(S, beta, -1 / S[i, i])


def _chol(M):
    k = M.shape[0]
    L = np.zeros_like(M)
    for a in range(k):
        for b in range(a + 1):
            s = M[a, b] - np.dot(L[a, :b], L[b, :b])
            if a == b:
                L[a, a] = np.sqrt(s) if s > 0 else 0
            else:
                L[a, b] = s / L[b, b] if L[b, b] > 0 else 0
    return L


def _solve_lower(L, b, trans=False):
    k = L.shape[0]
    x = b.copy()
    if not trans:
        for a in range(k):
            x[a] = (x[a] - np.dot(L[a, :a], x[:a])) / L[a, a]
    else:
        for a in range(k - 1, -1, -1):
            x[a] = (x[a] - np.dot(L[a + 1:, a], x[a + 1:])) / L[a, a]
    return x


class Result:
    def __init__(self, subset, S_resid, L_T=None, error=""):
        self.subset = np.array(subset, dtype=np.int64)
        self.S_resid = S_resid
        self.L_T = L_T
        self.error = error
        self.gaps = []
        self.n_updates = 0
        self.n_swaps = 0
        self.n_cycles = 0

    @property
    def min_gap(self):
        return min(self.gaps) if self.gaps else np.inf


def greedy(S, k, loss, dtype):
    Sr = np.array(S, dtype=dtype, order="F")
    p = Sr.shape[0]
    member = np.zeros(p, dtype=bool)
    res = Result([], Sr)
    subset = []
    for _ in range(k):
        sc, _early = scores(Sr, member, loss)
        star, gap = masked_argmax(sc, member)
        res.gaps.append(gap)
        member[star] = True
        subset.append(star)
        fwd(Sr, star)
        res.n_updates += 1
    res.subset = np.array(subset, dtype=np.int64)
    return res


def swapping(S, subset, loss, dtype, max_iters=1000):
    dtype = np.dtype(dtype).type
    small = np.float64 if np.finfo(dtype).eps >= np.finfo(np.float64).eps else dtype  # the k x k algebra
    S = np.array(S, dtype=dtype, order="F")
    Ss = S.astype(small)
    p = S.shape[0]
    subset = [int(j) for j in subset]
    k = len(subset)
    if k <= 0 or k >= p:
        return Result(subset, None)
    Sr = S.copy()
    res = Result(subset, Sr)
    dependent = "Initial subset are not linearly independent columns."
    for j in subset:
        if Sr[j, j] <= dtype(EPS):
            res.error = dependent
            return res
        fwd(Sr, j)
        res.n_updates += 1
    L_T = _chol(Ss[np.ix_(subset, subset)])
    res.L_T = L_T
    if np.any(np.diagonal(L_T) <= EPS):
        res.error = dependent
        return res
    member = np.zeros(p, dtype=bool)
    member[subset] = True
    n_keep = 0
    for it in range(max_iters):
        res.n_cycles = it + 1
        for jj in range(k):
            j = subset[jj]
            U = [subset[(jj + 1 + i) % k] for i in range(k - 1)]
            L_U = _chol(Ss[np.ix_(U, U)])
            v = _solve_lower(L_U, _solve_lower(L_U, Ss[U, j]), trans=True)
            beta = S[:, j] - S[:, U] @ v.astype(dtype)
            if beta[j] <= 0:
                return res
            rank_one(Sr, beta, 1 / beta[j])
            res.n_updates += 1
            member[j] = False
            sc, early = scores(Sr, member, loss)
            star, gap = masked_argmax(sc, member)
            res.gaps.append(gap)
            if sc[j] < sc[star]:
                subset[jj] = star
                n_keep = 0
                res.n_swaps += 1
            else:
                n_keep += 1
            jn = subset[jj]
            member[jn] = True
            x = _solve_lower(L_U, Ss[U, jn])
            last = np.sqrt(max(Ss[jn, jn] - np.dot(x, x), small(0)))
            L_T = np.zeros((k, k), dtype=small)
            L_T[:k - 1, :k - 1] = L_U
            L_T[k - 1, :k - 1] = x
            L_T[k - 1, k - 1] = last
            res.L_T = L_T
            res.subset = np.array(subset, dtype=np.int64)
            fwd(Sr, jn)
            res.n_updates += 1
            if n_keep >= k or early or last <= EPS:
                return res
    res.error = "Maximum swapping cycles reached!"
    return res


def run(S, k, loss, method, dtype):
    """``method``: ``"greedy"``, ``"swapping"`` (greedy start, as ``css_cov(subset=None)``) or ``"swapping_tail"`` (start
    ``arange(p - k, p)``).  Returns the result with the gaps of every decision taken on the way."""
    p = S.shape[0]
    if method == "greedy":
        return greedy(S, k, loss, dtype)
    if method == "swapping":
        g = greedy(S, k, loss, dtype)
        r = swapping(S, g.subset, loss, dtype)
        r.gaps = g.gaps + r.gaps
        return r
    return swapping(S, np.arange(p - k, p), loss, dtype)


@functools.lru_cache(maxsize=None)
def cached_run(gen, p, k, seed, loss, method, dtype_name, via32=False):
    """The restatement on a generated input, computed once per session.  ``via32``: the input is rounded to float32 first (the
    matrix a float32 solve sees)."""
    S = make_input(gen, p, k, seed)
    if via32:
        S = S.astype(np.float32)
    return run(S, k, loss, method, np.dtype(dtype_name).type)


# ---- brute force ----------------------------------------------------------------------------------------------------------------
class BruteForce:
    """The three losses evaluated from their definitions for an index set ``T`` (as logs where the definition is a product), and
    the two searches written directly on top of them."""

    def __init__(self, S, loss):
        self.S = np.asarray(S, dtype=np.float64)
        self.p = self.S.shape[0]
        self.kind = loss

    def loss(self, T):
        S, T = self.S, list(T)
        if not T:
            return {"least_squares": np.trace(S), "subset_factor": np.sum(np.log(np.diag(S))), "min_det": 0.0}[self.kind]
        S_TT = S[np.ix_(T, T)]
        if self.kind == "min_det":
            return np.linalg.slogdet(S_TT)[1]
        R = S - S[:, T] @ np.linalg.solve(S_TT, S[T, :])
        if self.kind == "least_squares":
            return np.trace(R)
        rest = np.setdiff1d(np.arange(self.p), T)
        return np.linalg.slogdet(S_TT)[1] + np.sum(np.log(np.diag(R)[rest]))

    def greedy(self, k):
        T = []
        for _ in range(k):
            vals = [np.inf if j in T else self.loss(T + [j]) for j in range(self.p)]
            T.append(int(np.argmin(vals)))
        return T

    def swapping(self, subset):
        T = [int(j) for j in subset]
        changed = True
        while changed and T:
            changed = False
            for pos in range(len(T)):
                keep = T[pos]
                others = T[:pos] + T[pos + 1:]
                vals = np.full(self.p, np.inf)
                for c in range(self.p):
                    if c not in others:
                        vals[c] = self.loss(others[:pos] + [c] + others[pos:])
                best = int(np.argmin(vals))
                if vals[best] < vals[keep]:
                    T[pos] = best
                    changed = True
        return T
