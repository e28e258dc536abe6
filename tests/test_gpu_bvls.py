"""solver.bvls on the device against the numpy restatement of tests/bvls_checks.py (itself checked against scipy in
test_bvls_host.py).  Wherever no decision of the restatement hangs on rounding (its min_gap is far above the rounding of the
format) the device must reproduce the whole trajectory: the ordered screen and active sets, the flags, iters and n_kkt.
beta, resid and loss must be as close to a run of the restatement in the next wider format as a correct implementation in the
format can be expected to be: within 8x the restatement's own error (the margin of test_gpu_css.py) plus one rounding per
element of a Gram column in a gradient update.  Every test prints the figures it asserts on."""
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.optimize import lsq_linear

import adelie_amd as ad
from adelie_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvls_checks as bc  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, p, kappa): ns <= 10 | | ns ~ 85: more than one wavefront | p > n: singular Gram | ns ~ 200 | 26-27 KKT rounds, the Gram
# appended 7 at a time, ends by the loss exit | ns ~ 1355: more than one trip of a 1024-thread workgroup
GRID = [(40, 13, None), (200, 70, None), (300, 130, None), (30, 100, None), (64, 300, None), (64, 300, 7), (400, 2000, 2000)]
SEEDS = range(3)
GAP64 = 1e-9
# problems have n <= 400: a float32 gradient is good to about 2e-5 relative, which leaves a 40x margin
GAP32 = 1e-3
EPS64, EPS32 = np.finfo(np.float64).eps, np.finfo(np.float32).eps


def set_config(name, value):
    b = _abi.hip_backend()
    b.check(b.fn("set_config")(name.encode(), float(value)))


def sets_of(state):
    return (list(state.screen_set[:state.screen_set_size]), list(state.active_set[:state.active_set_size]))


def check_exact(state, own):
    screen, active = sets_of(state)
    assert screen == list(own.screen)
    assert active == list(own.active)
    assert np.array_equal(state.is_screen, own.is_screen)
    assert np.array_equal(state.is_active, own.is_active)
    assert state.iters == own.iters and state.n_kkt == own.n_kkt


def err(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def check_close(state, own, truth, y, eps, what=""):
    """device vs truth within 8x (own vs truth) + the additive rounding term; returns the largest dev / bound ratio."""
    ns = max(len(truth.screen), 1)
    y_var = float(truth.y_var)
    rows = [
        ("beta", err(state.beta, truth.beta), err(own.beta, truth.beta), ns * eps * max(1.0, float(np.max(np.abs(truth.beta))))),
        ("resid", err(state.resid, truth.resid), err(own.resid, truth.resid), ns * eps * float(np.max(np.abs(y)))),
        ("loss", err(state.loss, truth.loss), err(own.loss, truth.loss), truth.iters * eps * y_var),
    ]
    worst = 0.0
    for name, e_dev, e_own, add in rows:
        bound = 8 * e_own + add
        ratio = e_dev / bound if bound > 0 else (0.0 if e_dev == 0 else np.inf)
        worst = max(worst, ratio)
        print(f"{what}{name}: device {e_dev:.3e}, restatement {e_own:.3e}, additive {add:.3e}, device / bound {ratio:.3f}")
    for name, e_dev, e_own, add in rows:
        assert e_dev <= 8 * e_own + add, name
    return worst


def check_invariants(state, X, y, lower, upper, weights=None):
    """Box, residual and loss of the returned state, recomputed in float64."""
    dtype = state.beta.dtype
    eps = np.finfo(dtype).eps
    n, p = X.shape
    with np.errstate(over="ignore"):
        lo = np.maximum(lower, -bc.MAX_SOLVER_VALUE).astype(dtype)
        up = np.minimum(upper, bc.MAX_SOLVER_VALUE).astype(dtype)
    assert np.all(state.beta >= lo) and np.all(state.beta <= up)
    X64, y64, b64 = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), state.beta.astype(np.float64)
    w = np.full(n, 1 / n) if weights is None else np.asarray(weights, dtype=np.float64)
    ns = state.screen_set_size
    start = np.where(np.abs(lo) < np.abs(up), lo, up).astype(np.float64)
    # the residual is formed once from the start vertex (a p-term dot per row) and caught up once per fit by a dot of at most
    # ns + 1 terms per row
    scale = float(np.max(np.abs(y64) + np.abs(X64) @ (np.abs(b64) + np.abs(start))))
    r_err = err(state.resid, y64 - X64 @ b64)
    r_bound = (p + 1 + (state.n_kkt + 1) * (ns + 2)) * eps * scale
    # the loss moves by one rounded update per changed visit: at most iters * ns of them
    y_var = float(np.sum(w * y64 * y64))
    r64 = state.resid.astype(np.float64)
    l_err = abs(state.loss - 0.5 * float(np.sum(w * r64 * r64)))
    l_bound = max(state.iters * max(ns, 1), 1) * eps * y_var
    print(f"resid vs y - X beta: {r_err:.3e} (bound {r_bound:.3e}); loss vs 1/2 sum w r^2: {l_err:.3e} (bound {l_bound:.3e})")
    assert r_err <= r_bound
    assert l_err <= l_bound


def same_state(a, b):
    assert a.beta.tobytes() == b.beta.tobytes()
    assert a.resid.tobytes() == b.resid.tobytes()
    assert a.loss == b.loss and a.iters == b.iters and a.n_kkt == b.n_kkt
    assert sets_of(a) == sets_of(b)
    assert np.array_equal(a.is_screen, b.is_screen) and np.array_equal(a.is_active, b.is_active)
    assert a.grad.tobytes() == b.grad.tobytes()


@pytest.mark.parametrize("n, p, kappa", GRID)
@pytest.mark.parametrize("seed", SEEDS)
def test_float64_grid(hip, n, p, kappa, seed):
    X, y, lower, upper = bc.cached_inputs("gaussian", n, p, seed)
    own = bc.cached_run("gaussian", n, p, seed, kappa, "float64")
    print(f"restatement: ns {len(own.screen)}, active {len(own.active)}, iters {own.iters}, n_kkt {own.n_kkt}, exit {own.exit}, "
          f"min_gap {own.min_gap:.3e}")
    assert own.min_gap >= GAP64  # every grid case qualifies: nothing is skipped
    state = ad.bvls(X, y, lower, upper, kappa=kappa)
    assert state.error == own.error == ""
    assert state.beta.dtype == np.float64 and state.beta.shape == (p,) and state.resid.shape == (n,)
    check_exact(state, own)
    truth = bc.cached_run("gaussian", n, p, seed, kappa, "longdouble")
    assert truth.screen == own.screen and truth.active == own.active and truth.iters == own.iters
    check_close(state, own, truth, y, EPS64)
    check_invariants(state, X, y, lower, upper)
    same_state(state, ad.bvls(X, y, lower, upper, kappa=kappa))


@pytest.mark.parametrize("n, p, kappa", [(64, 300, None), (400, 2000, 2000)])
def test_global_storage_gives_the_same_bits(hip, n, p, kappa):
    X, y, lower, upper = bc.cached_inputs("gaussian", n, p, 0)
    in_lds = ad.bvls(X, y, lower, upper, kappa=kappa)
    try:
        set_config("bvls_lds_max_ns", 16)
        in_global = ad.bvls(X, y, lower, upper, kappa=kappa)
    finally:
        set_config("bvls_lds_max_ns", 0)
    assert in_lds.screen_set_size > 16
    same_state(in_lds, in_global)
    check_exact(in_global, bc.cached_run("gaussian", n, p, 0, kappa, "float64"))


def truth32(n, p, seed, kappa):
    return bc.cached_run("gaussian", n, p, seed, kappa, "float64", True)


def test_float32_small_cases_qualify():
    """Skipping may not hide a failure: the three (40, 13) cases are clear of float32 rounding."""
    for seed in SEEDS:
        assert truth32(40, 13, seed, None).min_gap >= GAP32, seed


@pytest.mark.parametrize("n, p, kappa", GRID)
@pytest.mark.parametrize("seed", SEEDS)
def test_float32_grid(hip, n, p, kappa, seed):
    X, y, lower, upper = bc.cached_inputs("gaussian", n, p, seed)
    X32, y32 = np.asfortranarray(X, dtype=np.float32), y.astype(np.float32)
    truth = truth32(n, p, seed, kappa)
    own = bc.cached_run("gaussian", n, p, seed, kappa, "float32", True)
    state = ad.bvls(X32, y32, lower, upper, kappa=kappa)
    assert state.error == ""
    assert state.beta.dtype == np.float32 and state.resid.dtype == np.float32
    check_invariants(state, X32, y32, lower, upper)
    same_state(state, ad.bvls(X32, y32, lower, upper, kappa=kappa))
    print(f"float64 restatement on the rounded inputs: min_gap {truth.min_gap:.3e}")
    if truth.min_gap >= GAP32:
        assert own.screen == truth.screen and own.active == truth.active
        check_exact(state, truth)
        check_close(state, own, truth, y32, EPS32)
    if (n, p) != (400, 2000):
        f = lambda beta: bc.objective(X32, y32, beta)  # noqa: E731
        f_dev, f_own, f_truth = f(state.beta), f(own.beta), f(truth.beta)
        bound = 8 * abs(f_own - f_truth) + EPS32 * float(truth.y_var)
        print(f"objective: device - truth {f_dev - f_truth:.3e}, restatement - truth {f_own - f_truth:.3e}, bound {bound:.3e}")
        assert abs(f_dev - f_truth) <= bound


@pytest.mark.parametrize("n, p", [(10, 50), (40, 13), (100, 1000)])
def test_reference_generator(hip, n, p):
    """The reference's own test: inputs full of exact ties and zero columns, so only the objectives are compared."""
    X, y, lower, upper = bc.ref_sparse(n, p, 0)
    state = ad.bvls(X, y, lower, upper, tol=1e-9)
    assert state.error == ""
    sw = np.sqrt(1 / n)
    expected = bc.objective(X, y, lsq_linear(X * sw, y * sw, bounds=(lower, upper), method="bvls", tol=1e-14).x)
    actual = bc.objective(X, y, state.beta)
    print(f"objective: device {actual:.3e}, scipy {expected:.3e}")
    assert np.allclose(actual, expected)
    check_invariants(state, X, y, lower, upper)


@pytest.mark.parametrize("kappa", [None, 1, 3])
@pytest.mark.parametrize("seed", SEEDS)
def test_edge_inputs(hip, kappa, seed):
    """A zero column, a coordinate without a lower bound, one without an upper bound, a fixed one, uneven weights."""
    X, y, lower, upper, w = bc.edge(seed)
    own = bc.solve(X, y, lower, upper, np.float64, weights=w, kappa=kappa)
    truth = bc.solve(X, y, lower, upper, np.longdouble, weights=w, kappa=kappa)
    print(f"restatement: ns {len(own.screen)}, iters {own.iters}, n_kkt {own.n_kkt}, min_gap {own.min_gap:.3e}")
    assert own.min_gap >= GAP64
    state = ad.bvls(X, y, lower, upper, weights=w, kappa=kappa)
    assert state.error == ""
    check_exact(state, own)
    assert truth.screen == own.screen and truth.active == own.active
    check_close(state, own, truth, y, EPS64)
    check_invariants(state, X, y, lower, upper, w)
    assert not state.is_screen[3] and state.beta[2] == 0.25
    same_state(state, ad.bvls(X, y, lower, upper, weights=w, kappa=kappa))


def test_warm_start(hip):
    X, y, lower, upper = bc.cached_inputs("gaussian", 200, 70, 0)
    first = ad.bvls(X, y, lower, upper)
    again = ad.bvls(X, y, lower, upper, warm_start=first)
    own1 = bc.cached_run("gaussian", 200, 70, 0, None, "float64")
    own2 = bc.solve(X, y, lower, upper, np.float64, warm_start=own1)
    truth2 = bc.solve(X, y, lower, upper, np.longdouble, warm_start=bc.cached_run("gaussian", 200, 70, 0, None, "longdouble"))
    print(f"restatement of the warm start: iters {own2.iters}, n_kkt {own2.n_kkt}, exit {own2.exit}, min_gap {own2.min_gap:.3e}")
    assert own2.min_gap >= GAP64
    check_exact(first, own1)
    assert again.error == ""
    check_exact(again, own2)
    assert truth2.screen == own2.screen and truth2.active == own2.active
    check_close(again, own2, truth2, y, EPS64)
    check_invariants(again, X, y, lower, upper)


def test_max_iters(hip):
    X, y, lower, upper = bc.cached_inputs("gaussian", 64, 300, 0)
    own = bc.solve(X, y, lower, upper, np.float64, max_iters=3)
    truth = bc.solve(X, y, lower, upper, np.longdouble, max_iters=3)
    assert own.exit == "max_iters" and own.min_gap >= GAP64
    state = ad.bvls(X, y, lower, upper, max_iters=3)
    assert state.error == own.error == "adelie_core solver: bvls: max iterations reached!"
    check_exact(state, own)
    check_close(state, own, truth, y, EPS64)
    check_invariants(state, X, y, lower, upper)


def test_gram_limit(hip):
    X, y, lower, upper = bc.cached_inputs("gaussian", 400, 2000, 0)
    try:
        set_config("bvls_gram_limit_mb", 1)
        state = ad.bvls(X, y, lower, upper, kappa=2000)
    finally:
        set_config("bvls_gram_limit_mb", 16384)
    m = re.fullmatch(r"adelie_core solver: bvls: screen set of (\d+) coordinates exceeds the device Gram limit", state.error)
    assert m, state.error
    assert int(m.group(1)) ** 2 * 8 > 1 << 20
    assert state.n_kkt == 1 and state.screen_set_size == 0  # the state reached: one KKT round, nothing admitted
    check_invariants(state, X, y, lower, upper)
    assert ad.bvls(X, y, lower, upper, kappa=2000).error == ""


def test_argument_checks(hip):
    X, y, lower, upper = bc.cached_inputs("gaussian", 40, 13, 0)
    good = ad.bvls(X, y, lower, upper)
    kw = dict(X=X, y_var=good.y_var, X_vars=good.X_vars, lower=lower, upper=upper, weights=good.weights, kappa=13,
              max_iters=100, tol=1e-7, screen_set_size=0, screen_set=np.zeros(13, dtype=int), is_screen=np.zeros(13, dtype=bool),
              active_set_size=0, active_set=np.zeros(13, dtype=int), is_active=np.zeros(13, dtype=bool), beta=lower,
              resid=y - X @ lower, grad=np.zeros(13), loss=0.0)
    with pytest.raises(RuntimeError, match=re.escape("adelie_core solver: lower must be (p,) where X is (n, p). ")):
        ad.state.bvls(**dict(kw, lower=lower[:-1]))
    with pytest.raises(RuntimeError, match=re.escape("adelie_core solver: kappa must be > 0. ")):
        ad.state.bvls(**dict(kw, kappa=0))
    # the same checks behind the C entry point
    st = ad.state.bvls(**kw)
    b = st.X._backend
    args = _abi.BvlsArgs(
        X_vars=_abi.ptr(st.X_vars), lower=_abi.ptr(st.lower), upper=_abi.ptr(st.upper), weights=_abi.ptr(st.weights),
        beta=_abi.ptr(st.beta), resid=_abi.ptr(st.resid), grad=_abi.ptr(st.grad), n_X_vars=13, n_lower=12, n_upper=13,
        n_weights=40, n_beta=13, n_resid=40, n_grad=13, screen_set=None, screen_set_size=0, active_set=None, active_set_size=0,
        n_active_set=13, n_is_active=13, y_var=st.y_var, loss=st.loss, kappa=13, max_iters=100, tol=1e-7)
    handle = _abi.C.c_void_p()
    assert b.fn("bvls_solve")(st.X._handle, _abi.C.byref(args), handle) != 0
    assert b.fn("last_error")().decode() == "adelie_core solver: lower must be (p,) where X is (n, p). "


class UserDense(ad.matrix.MatrixNaiveBase64):
    def __init__(self, mat):
        self.mat = mat
        ad.matrix.MatrixNaiveBase64.__init__(self)

    def ctmul(self, j, v, out):
        out[...] += self.mat[:, j] * v

    def rows(self):
        return self.mat.shape[0]

    def cols(self):
        return self.mat.shape[1]


def test_inputs_agree(hip):
    X, y, lower, upper = bc.cached_inputs("gaussian", 200, 70, 1)
    base = ad.bvls(X, y, lower, upper)
    for other in (np.ascontiguousarray(X), ad.matrix.dense(X), UserDense(X)):
        same_state(base, ad.bvls(other, y, lower, upper))


def read_back(M):
    n, p = M.rows(), M.cols()
    out = np.zeros((n, p), order="F")
    for j in range(p):
        M.ctmul(j, 1.0, out[:, j])
    return out


def generic_designs(seed):
    rng = np.random.RandomState(100 + seed)
    X = bc.cached_inputs("gaussian", 40, 13, seed)[0]
    calls = rng.choice([0, 1, 2], size=(40, 13), p=[0.5, 0.35, 0.15]).astype(np.int8)
    return dict(
        snp=lambda: ad.matrix.snp_calldata(calls),
        sparse=lambda: ad.matrix.sparse(sp.csc_matrix(X * (np.abs(X) > 0.8)), resident="csc"),
        standardized=lambda: ad.matrix.standardize(ad.matrix.dense(X), lazy=True),
    )


@pytest.mark.parametrize("kind", ["snp", "sparse", "standardized"])
@pytest.mark.parametrize("seed", SEEDS)
def test_generic_route(hip, kind, seed):
    """Designs the native route does not take run the same loop through their cmul / ctmul / mul."""
    _, y, lower, upper = bc.cached_inputs("gaussian", 40, 13, seed)
    M = generic_designs(seed)[kind]()
    assert not ad.state._bvls_native(M)
    Xd = read_back(M)
    own = bc.solve(Xd, y, lower, upper, np.float64)
    truth = bc.solve(Xd, y, lower, upper, np.longdouble)
    print(f"restatement: ns {len(own.screen)}, iters {own.iters}, n_kkt {own.n_kkt}, min_gap {own.min_gap:.3e}")
    assert own.min_gap >= GAP64
    state = ad.bvls(M, y, lower, upper)
    assert state.error == ""
    check_exact(state, own)
    assert truth.screen == own.screen and truth.active == own.active
    check_close(state, own, truth, y, EPS64)
    check_invariants(state, Xd, y, lower, upper)
