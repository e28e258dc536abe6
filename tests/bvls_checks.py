"""A numpy restatement of bounded-variable least squares as the reference solves it (solver_bvls.hpp: coordinate_descent,
solve_active, fit, kkt_screen, solve; the set-up of adelie/solver.py:961-1116), for the tests of adelie_amd.solver.bvls.

Per visit the gradient is g_k = (w * x_k) . r and a changed coefficient is followed by r -= del * x_k, all in the dtype the
caller names (float32, float64, longdouble).  Ties between equal violations go to the lower index (a stable sort of
0..p-1 every round; the reference's std::sort leaves them open).  The run records its trajectory (beta, resid, loss, iters,
n_kkt, the ordered screen and active sets, which exit was taken) and `min_gap`, the smallest relative margin by which any
of its decisions was taken:

  clamp      a visit with var_k > 0, per bound of magnitude below max_solver_value: |cand - bound| / max(|beta_old|, |step|)
  pass       passes with convg > 0: |convg - tol y_var| / (tol y_var)
  loss exit  ||d loss| - 1e-6 |y_var|| / (1e-6 |y_var|)
  sign       the non-screen coordinates whose sign decides a violation: |grad_j| / max|grad|
  order      neighbouring positive violations of non-screen coordinates: their difference / max|grad|

A device run in the same format may differ from this one by rounding only; where min_gap is far above that rounding, every
decision, hence the whole trajectory, must be the same."""
import functools

import numpy as np

MAX_SOLVER_VALUE = 1e100
MAX_ITERS_MSG = "adelie_core solver: bvls: max iterations reached!"


def gaussian(n, p, seed):
    """X ~ N(0, 1), y = X (2 N(0, 1)) + N(0, 1), bounds [-0.5, 1.5]."""
    rng = np.random.RandomState(seed)
    X = np.asfortranarray(rng.normal(size=(n, p)))
    y = X @ (2 * rng.normal(size=p)) + rng.normal(size=n)
    return X, y, np.full(p, -0.5), np.full(p, 1.5)


def ref_sparse(n, p, seed=0):
    """The inputs of the reference's own bvls test: uniform entries of which about 80 % are set to exactly zero, every column
    given the sign that makes it anti-correlated with one random direction, and a response that a point of the box fits
    exactly."""
    rs = np.random.RandomState(seed)
    X = rs.uniform(0, 1, (n, p))
    zero = rs.binomial(1, 0.8, X.size).astype(bool)
    X.ravel()[zero] = 0
    flip = (X.T @ rs.normal(0, 1, n)) >= 0
    X = np.asfortranarray(X * (1 - 2 * flip))
    coef = rs.normal(1, 1, p)
    y = X @ (flip * coef) / n
    return X, y, np.full(p, -0.5), np.full(p, 1.5)


def edge(seed, n=50, p=20):
    """gaussian(50, 20) with a zero column, a coordinate free below, one free above, one fixed, and uneven weights."""
    X, y, lower, upper = gaussian(n, p, seed)
    X[:, 3] = 0
    lower[0] = -np.inf
    upper[1] = np.inf
    lower[2] = upper[2] = 0.25
    w = np.random.RandomState(1000 + seed).uniform(0.5, 1.5, n)
    return X, y, lower, upper, w / w.sum()


class Result:
    pass


def objective(X, y, beta, weights=None):
    """1/2 sum w (y - X beta)^2 in float64."""
    X = np.asarray(X, dtype=np.float64)
    w = np.full(X.shape[0], 1 / X.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    r = np.asarray(y, dtype=np.float64) - X @ np.asarray(beta, dtype=np.float64)
    return 0.5 * float(np.sum(w * r * r))


def solve(X, y, lower, upper, dtype, *, weights=None, kappa=None, max_iters=int(1e5), tol=1e-7, warm_start=None):
    """adelie.solver.bvls + StateBVLS.solve(), every quantity in `dtype`."""
    dtype = np.dtype(dtype)
    dt = dtype.type
    n, p = X.shape
    with np.errstate(over="ignore"):
        X = np.asfortranarray(X, dtype=dtype)
        y = np.asarray(y, dtype=dtype)
        w = np.full(n, 1 / n) if weights is None else weights
        w = np.asarray(w, dtype=dtype)
        if kappa is None:
            kappa = min(n, p)
        lower = np.maximum(np.asarray(lower, dtype=np.float64), -MAX_SOLVER_VALUE).astype(dtype)
        upper = np.minimum(np.asarray(upper, dtype=np.float64), MAX_SOLVER_VALUE).astype(dtype)
    y_var = np.sum(y * y * w)
    WX = np.asfortranarray(w[:, None] * X)
    X_vars = np.sum(WX * X, axis=0)
    zero_col = ~np.any(X != 0, axis=0)
    res = Result()
    if warm_start is None:
        beta = np.where(np.abs(lower) < np.abs(upper), lower, upper).astype(dtype)
        active = []
    else:
        beta = np.array(warm_start.beta, dtype=dtype)
        active = list(warm_start.active)
    screen = list(active)
    is_screen = np.zeros(p, dtype=bool)
    is_screen[screen] = True
    is_active = is_screen.copy()
    resid = y - X @ beta
    st = dict(loss=dt(0.5) * np.sum(resid * resid * w), iters=0, n_kkt=0, gap=np.inf)
    tol_yvar = dt(tol) * y_var
    half = dt(0.5)
    finite_lo = np.abs(lower.astype(np.float64)) < MAX_SOLVER_VALUE
    finite_up = np.abs(upper.astype(np.float64)) < MAX_SOLVER_VALUE

    def note(g):
        if g < st["gap"]:
            st["gap"] = float(g)

    def descend(members, add):
        convg = dt(0)
        for k in members:
            vk, lk, uk, bk = X_vars[k], lower[k], upper[k], beta[k]
            gk = WX[:, k] @ resid
            step = dt(0) if vk <= 0 else gk / vk
            cand = bk + step
            if vk > 0:
                den = max(abs(bk), abs(step))
                for ok, bound in ((finite_lo[k], lk), (finite_up[k], uk)):
                    if ok:
                        num = abs(cand - bound)
                        if den > 0:
                            note(num / den)
                        elif num == 0:
                            note(0.0)
            bn = min(max(cand, lk), uk)
            if bn == bk:
                continue
            beta[k] = bn
            d = bn - bk
            sds = vk * d * d
            convg = max(convg, sds)
            st["loss"] = st["loss"] - (d * gk - half * sds)
            resid[:] = resid - d * X[:, k]
            if add and not is_active[k]:
                active.append(k)
                is_active[k] = True
        if convg > 0 and tol_yvar > 0:
            note(abs(convg - tol_yvar) / tol_yvar)
        return convg

    def prune():
        keep = [k for k in active if not (beta[k] <= lower[k] or beta[k] >= upper[k])]
        is_active[active] = False
        is_active[keep] = True
        active[:] = keep

    class MaxIters(Exception):
        pass

    def fit():
        while True:
            st["iters"] += 1
            convg = descend(list(screen), True)
            if st["iters"] >= max_iters:
                raise MaxIters
            if convg <= tol_yvar:
                prune()
                return
            while True:
                st["iters"] += 1
                convg = descend(list(active), False)
                if st["iters"] >= max_iters:
                    raise MaxIters
                if convg <= tol_yvar:
                    break
            prune()

    res.error, res.exit, res.grad = "", None, None
    try:
        while True:
            loss_prev = st["loss"]
            fit()
            if st["n_kkt"] > 0:
                thr = 1e-6 * abs(float(y_var))
                dl = float(abs(st["loss"] - loss_prev))
                if thr > 0:
                    note(abs(dl - thr) / thr)
                if dl < thr:
                    res.exit = "loss"
                    break
            st["n_kkt"] += 1
            grad = (WX.T @ resid).astype(dtype)
            viols = (np.maximum(grad, 0) * (beta < upper) - np.minimum(grad, 0) * (beta > lower)).astype(dtype)
            res.grad = viols
            gmax = float(np.max(np.abs(grad))) if p else 0.0
            if gmax > 0:
                out = ~is_screen & ~zero_col  # (the gradient of an all-zero column is exactly zero in every format)
                decides = out & ((beta < upper) | (beta > lower))
                if np.any(decides):
                    note(float(np.min(np.abs(grad[decides]))) / gmax)
                pos = np.sort(viols[out & (viols > 0)].astype(np.float64))
                if pos.size > 1:
                    note(float(np.min(np.diff(pos))) / gmax)
            order = np.argsort(-viols, kind="stable")
            n_old, passed = len(screen), True
            for k in order:
                if is_screen[k] or not viols[k] > 0:
                    continue
                passed = False
                if len(screen) >= n_old + kappa:
                    break
                screen.append(int(k))
                is_screen[k] = True
            if passed:
                res.exit = "kkt"
                break
    except MaxIters:
        res.exit, res.error = "max_iters", MAX_ITERS_MSG
    res.beta, res.resid, res.loss = beta, resid, st["loss"]
    res.iters, res.n_kkt, res.min_gap = st["iters"], st["n_kkt"], st["gap"]
    res.screen, res.active = list(screen), list(active)
    res.is_screen, res.is_active = is_screen, is_active
    res.y_var, res.X_vars = y_var, X_vars
    return res


GENERATORS = dict(gaussian=gaussian, ref_sparse=ref_sparse)


@functools.lru_cache(maxsize=None)
def cached_inputs(gen, n, p, seed):
    return GENERATORS[gen](n, p, seed)


@functools.lru_cache(maxsize=None)
def cached_run(gen, n, p, seed, kappa, dtype, round32=False, tol=1e-7, max_iters=int(1e5)):
    """The restatement on a generated problem; `round32`: inputs rounded to float32 first (what a float32 design holds)."""
    X, y, lower, upper = cached_inputs(gen, n, p, seed)
    if round32:
        X, y = X.astype(np.float32), y.astype(np.float32)
    return solve(X, y, lower, upper, np.dtype(dtype), kappa=kappa, tol=tol, max_iters=max_iters)
