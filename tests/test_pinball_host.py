"""pinball without a device: the numpy restatement the GPU tests compare against (tests/pinball_checks.py) is itself checked
against an independent solver (scipy's L-BFGS-B on the split form) and a KKT certificate; solver.pinball through its Python
route (a numpy-backed MatrixConstraintBase subclass) must walk the restatement's trajectory; and the public surface (export,
signatures, messages, the ctypes mirror of the C arguments) is what the reference and include/adelie_hip.h say."""
import ctypes
import inspect
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
from scipy.optimize import minimize

import adelie_amd as ad
from adelie_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinball_checks as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [(m, d) for m in (3, 5, 10, 20) for d in (1, 5, 10)]


def _host_class(base):
    class HostConstraint(base):
        """The MatrixConstraintBase operations on a numpy array (no device)."""

        def __init__(self, A):
            self.A = np.ascontiguousarray(A, dtype=self.dtype)

        def rows(self):
            return self.A.shape[0]

        def cols(self):
            return self.A.shape[1]

        def rmmul(self, j, Q, out):
            out[...] = self.A[j] @ np.asarray(Q, dtype=self.dtype)

        def rvmul(self, j, v):
            return self.A[j] @ v

        def rvtmul(self, j, v, out):
            out += v * self.A[j]

        def mul(self, v, out):
            out[...] = np.asarray(v, dtype=self.dtype) @ self.A

        def tmul(self, v, out):
            out[...] = self.A @ v

        def cov(self, Q, out):
            out[...] = self.A @ Q @ self.A.T

        def sp_mul(self, indices, values, out):
            out[...] = np.asarray(values, dtype=self.dtype) @ self.A[np.asarray(indices, dtype=int)]

    return HostConstraint


Host64 = _host_class(ad.matrix.MatrixConstraintBase64)
Host32 = _host_class(ad.matrix.MatrixConstraintBase32)


def scipy_beta(A, S, v, pneg, ppos):
    """min over (b+, b-) >= 0 of the objective at beta = b+ - b-, by L-BFGS-B with its analytic gradient."""
    m = A.shape[0]

    def f(x):
        b = x[:m] - x[m:]
        t = A.T @ b
        St = S @ t
        g = A @ (St - v)
        return 0.5 * t @ St - v @ t + ppos @ x[:m] + pneg @ x[m:], np.concatenate([g + ppos, -g + pneg])

    sol = minimize(f, np.zeros(2 * m), jac=True, method="L-BFGS-B", bounds=[(0, None)] * (2 * m),
                   options=dict(maxiter=100000, maxfun=1000000, ftol=1e-16, gtol=1e-13, maxcor=30))
    return sol.x[:m] - sol.x[m:]


@pytest.mark.parametrize("m, d", GRID)
def test_restatement_against_scipy_and_kkt(m, d):
    """The reference's own test grid and input (tests/test_solver.py, test_pinball: n = 10, tol = 1e-24, ten seeds) and its two
    criteria: the objective no worse than the independent solver's times (1 + 1e-7) in the signed sense, and resid equal to
    v - S A' beta to atol 1e-7.

    The KKT certificate, with g = A (v - S A' beta): -l <= g <= u where beta = 0, g = u where beta > 0, g = -l where beta < 0.
    Bound.  Every run here ends by the KKT exit (asserted), so no coordinate outside the screen set had a positive violation
    at the last full gradient, and nothing changed after it.  Inside the screen set the last pass changed every coordinate by
    v_j del_j^2 <= tol y_var.  A visit leaves its own coordinate stationary; the later visits of the pass move g_k by
    sum_j |H_kj del_j| <= sqrt(v_k) sum_j sqrt(v_j del_j^2) <= sqrt(v_k) ns sqrt(tol y_var)  (H is positive semi-definite, so
    |H_kj| <= sqrt(v_k v_j)).  To that comes the rounding of recomputing g in float64 here against the solver's running
    residual: 64 eps (|A| (|v| + |S| |A' beta|))_k covers the d-term dots and the accumulated residual updates (at most a few
    thousand visits)."""
    tol = 1e-24
    eps = np.finfo(np.float64).eps
    for seed in range(10):
        A, S, v, pneg, ppos = pc.gen(m, d, seed, 1.0, n=10)
        res = pc.solve(A, S, v, pneg, ppos, np.float64, tol=tol)
        assert res.error == "" and res.exit == "kkt"
        actual = pc.objective(A, S, v, pneg, ppos, res.beta)
        expected = pc.objective(A, S, v, pneg, ppos, scipy_beta(A, S, v, pneg, ppos))
        assert actual <= expected * (1 + np.sign(expected) * 1e-7), (seed, actual, expected)
        beta = np.asarray(res.beta, dtype=np.float64)
        resid = v - S @ (A.T @ beta)
        assert np.allclose(res.resid, resid, atol=1e-7)
        g = A @ resid
        diag = np.einsum("ij,jk,ik->i", A, S, A)
        bound = np.sqrt(np.maximum(diag, 0)) * len(res.screen) * np.sqrt(tol * float(res.y_var))
        bound = bound + 64 * eps * (np.abs(A) @ (np.abs(v) + np.abs(S) @ np.abs(A.T @ beta)))
        miss = np.where(beta > 0, np.abs(g - ppos), np.where(beta < 0, np.abs(g + pneg), np.maximum(np.maximum(g - ppos, -pneg - g), 0)))
        print(f"seed {seed}: objective {actual:.6e} vs {expected:.6e}, worst KKT miss / bound {np.max(miss / bound):.2e}")
        assert np.all(miss <= bound), (seed, np.max(miss / bound))
        # the bookkeeping the device is compared with is consistent in itself
        assert sorted(np.flatnonzero(res.is_screen)) == sorted(res.screen)
        assert sorted(np.flatnonzero(res.is_active)) == sorted(res.active)
        assert set(res.active) <= set(res.screen)


def same_trajectory(state, res):
    assert list(state.screen_set[:state.screen_set_size]) == res.screen
    assert list(state.active_set[:state.active_set_size]) == res.active
    assert np.array_equal(state.is_screen, res.is_screen) and np.array_equal(state.is_active, res.is_active)
    assert (state.iters, state.n_kkt) == (res.iters, res.n_kkt)


def same_numbers(state, res):
    """The Python route does the restatement's arithmetic through the matrix interface, on the same arrays: bit-equal."""
    assert state.beta.dtype == res.beta.dtype
    assert np.array_equal(state.beta, res.beta) and np.array_equal(state.resid, res.resid)
    assert state.loss == float(res.loss)
    if res.grad is not None:
        assert np.array_equal(state.grad, res.grad)
    mem = res.screen
    assert np.array_equal(state.screen_AS[mem], res.screen_AS[mem])
    assert np.array_equal(state.screen_ASAT_diag[mem], res.screen_ASAT_diag[mem])


@pytest.mark.parametrize("host, dtype", [(Host64, np.float64), (Host32, np.float32)])
@pytest.mark.parametrize("m, d", GRID + [("edge", 0)])
def test_python_route_walks_the_restatement(host, dtype, m, d):
    for seed in range(10 if m != "edge" else 3):
        A, S, v, pneg, ppos = pc.edge(seed) if m == "edge" else pc.gen(m, d, seed, 1.0, n=10)
        res = pc.solve(A, S, v, pneg, ppos, dtype)
        state = ad.solver.pinball(host(A), S, v, pneg, ppos)
        assert state.error == res.error == ""
        same_trajectory(state, res)
        same_numbers(state, res)
        assert isinstance(state, ad.state.pinball) and state.total_time > 0


@pytest.mark.parametrize("host, dtype", [(Host64, np.float64), (Host32, np.float32)])
def test_infinite_penalties_fix_the_sign(host, dtype):
    for seed in range(3):
        A, S, v, pneg, ppos = pc.edge(seed)
        state = ad.solver.pinball(host(A), S, v, pneg, ppos)
        assert state.error == ""
        assert np.all(state.beta[::2] >= 0) and np.all(state.beta[1::4] <= 0)
        assert state.beta[5] == 0  # the zero row is never changed
        assert np.any(state.beta > 0) and np.any(state.beta < 0)


def test_warm_start_max_iters_and_kappa():
    A, S, v, pneg, ppos = pc.gen(130, 40, 0, 0.3)
    coarse = ad.solver.pinball(Host64(A), S, v, pneg, ppos, tol=1e-4)
    own = pc.solve(A, S, v, pneg, ppos, np.float64, tol=1e-4)
    same_trajectory(coarse, own)
    fine = ad.solver.pinball(Host64(A), S, v, pneg, ppos, tol=1e-9, warm_start=coarse)
    warm = pc.solve(A, S, v, pneg, ppos, np.float64, tol=1e-9, warm_start=own)
    assert fine.error == ""
    same_trajectory(fine, warm)
    same_numbers(fine, warm)
    again = ad.solver.pinball(Host64(A), S, v, pneg, ppos, tol=1e-9, warm_start=fine)
    assert again.n_kkt <= 1 and again.screen_set_size == fine.active_set_size  # no admissions from the solution

    cut = ad.solver.pinball(Host64(A), S, v, pneg, ppos, max_iters=3)
    ref = pc.solve(A, S, v, pneg, ppos, np.float64, max_iters=3)
    assert cut.error == ref.error == "adelie_core solver: pinball: max iterations reached!"
    same_trajectory(cut, ref)
    same_numbers(cut, ref)

    one = ad.solver.pinball(Host64(A), S, v, pneg, ppos, kappa=1)
    ref1 = pc.solve(A, S, v, pneg, ppos, np.float64, kappa=1)
    assert one.n_kkt > 2
    same_trajectory(one, ref1)
    same_numbers(one, ref1)


def test_surface():
    assert ad.pinball is ad.solver.pinball
    assert callable(ad.state.pinball)
    for name in ("MatrixConstraintBase", "MatrixConstraintBase64", "MatrixConstraintBase32"):
        assert inspect.isclass(getattr(ad.matrix, name))
    assert ad.matrix.MatrixConstraintBase64.dtype == np.float64 and ad.matrix.MatrixConstraintBase32.dtype == np.float32
    E = inspect.Parameter.empty
    sig = [(p.name, p.default) for p in inspect.signature(ad.solver.pinball).parameters.values()]
    assert sig == [("A", E), ("S", E), ("v", E), ("penalty_neg", E), ("penalty_pos", E), ("kappa", None),
                   ("max_iters", int(1e5)), ("tol", 1e-7), ("n_threads", 1), ("warm_start", None)]
    kinds = [p.kind for p in inspect.signature(ad.solver.pinball).parameters.values()]
    assert kinds[:5] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 5 and set(kinds[5:]) == {inspect.Parameter.KEYWORD_ONLY}
    names = ["A", "y_var", "S", "penalty_neg", "penalty_pos", "kappa", "max_iters", "tol", "screen_set_size", "screen_set",
             "is_screen", "screen_ASAT_diag", "screen_AS", "active_set_size", "active_set", "is_active", "beta", "resid", "grad",
             "loss"]
    assert [p.name for p in inspect.signature(ad.state.pinball).parameters.values()] == names
    A, S, v, pneg, ppos = pc.gen(5, 3, 0)
    state = ad.solver.pinball(Host64(A), S, v, pneg, ppos)
    for name in names + ["iters", "n_kkt", "error", "total_time", "benchmark"]:
        assert hasattr(state, name), name
    assert state.screen_AS.shape == (5, 3) and state.screen_ASAT_diag.shape == (5,)
    assert Host64(A).shape == (5, 3) and Host64(A).ndim == 2


def test_method_message():
    with pytest.raises(ValueError, match="method must be one of 'naive', 'cov' or 'constraint'."):
        ad.matrix.dense(np.zeros((2, 2)), method="bogus")


def _state_kwargs(m=6, d=4):
    A, S, v, pneg, ppos = pc.gen(m, d, 0)
    return dict(A=Host64(A), y_var=1.0, S=S, penalty_neg=pneg, penalty_pos=ppos, kappa=2, max_iters=100, tol=1e-7,
                screen_set_size=0, screen_set=np.zeros(m, dtype=int), is_screen=np.zeros(m, dtype=bool),
                screen_ASAT_diag=np.zeros(m), screen_AS=np.zeros((m, d)), active_set_size=0, active_set=np.zeros(m, dtype=int),
                is_active=np.zeros(m, dtype=bool), beta=np.zeros(m), resid=np.array(v), grad=np.zeros(m), loss=0.5)


@pytest.mark.parametrize("change, message", [
    (dict(S=np.eye(3)), "S must be (d, d) where A is (m, d). "),
    (dict(penalty_neg=np.zeros(5)), "penalty_neg must be (m,) where A is (m, d). "),
    (dict(penalty_pos=np.zeros(7)), "penalty_pos must be (m,) where A is (m, d). "),
    (dict(kappa=0), "kappa must be > 0. "),
    (dict(tol=-1.0), "tol must be >= 0."),
    (dict(screen_set_size=7), "screen_set_size must be <= m where A is (m, d). "),
    (dict(screen_set=np.zeros(5, dtype=int)), "screen_set must be (m,) where A is (m, d). "),
    (dict(is_screen=np.zeros(5, dtype=bool)), "is_screen must be (m,) where A is (m, d). "),
    (dict(screen_ASAT_diag=np.zeros(5)), "screen_ASAT_diag must be (m,) where A is (m, d). "),
    (dict(screen_AS=np.zeros((6, 3))), "screen_AS must be (m, d) where A is (m, d). "),
    (dict(active_set_size=7), "active_set_size must be <= m where A is (m, d). "),
    (dict(active_set=np.zeros(5, dtype=int)), "active_set must be (m,) where A is (m, d). "),
    (dict(is_active=np.zeros(5, dtype=bool)), "is_active must be (m,) where A is (m, d). "),
    (dict(beta=np.zeros(5)), "beta must be (m,) where A is (m, d). "),
    (dict(resid=np.zeros(5)), "resid must be (d,) where A is (m, d). "),
    (dict(grad=np.zeros(5)), "grad must be (m,) where A is (m, d). "),
])
def test_validation_messages(change, message):
    """state_pinball.ipp:15-94, in its order and with its words."""
    ad.state.pinball(**_state_kwargs())
    with pytest.raises(RuntimeError) as e:
        ad.state.pinball(**dict(_state_kwargs(), **change))
    assert str(e.value) == "adelie_core solver: " + message


def test_constraint_matrix_is_no_design():
    A = Host64(np.ones((3, 2)))
    with pytest.raises(RuntimeError, match="constraint matrix"):
        ad.matrix.as_design(A)
    for call in (lambda: ad.matrix.standardize(A), lambda: ad.matrix.subset(A, np.arange(2), axis=0),
                 lambda: ad.matrix.concatenate([A, A], axis=0), lambda: ad.matrix.kronecker_eye(A, 2)):
        with pytest.raises(RuntimeError, match="not a constraint matrix"):
            call()
    with pytest.raises(ValueError, match="MatrixConstraintBase"):
        ad.solver.pinball([[1.0]], np.eye(1), np.ones(1), np.ones(1), np.ones(1))


def test_linear_constraint_takes_a_constraint_matrix():
    rs = np.random.RandomState(0)
    A = rs.normal(size=(4, 3))
    lower, upper = -rs.uniform(0.1, 1, 4), rs.uniform(0.1, 1, 4)
    quad = rs.uniform(0.5, 1, 3)
    linear = 3 * rs.normal(size=3)
    Q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    xs = []
    for mat in (A, Host64(A)):
        cnstr = ad.constraint.linear(mat, lower, upper)
        x = np.zeros(3)
        cnstr.solve(x, quad, linear, 0.1, 0.0, Q, None)
        xs.append(x)
    assert np.any(xs[0] != 0)
    assert np.array_equal(xs[0], xs[1])


def test_pinball_args_match_c_layout():
    fields = [f[0] for f in _abi.PinballArgs._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"adelie_hip.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(adelie_hip_pinball_args));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(adelie_hip_pinball_args, {f}));\n'
    prog += 'printf("%d\\n", ADELIE_HIP_PINBALL_SCREEN_AS);\nprintf("%d\\n", ADELIE_HIP_PINBALL_N_CHANGED);\n'
    prog += 'printf("%d\\n", ADELIE_HIP_CONS_TO_DENSE);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(_abi.PinballArgs)
    for f, off in zip(fields, out[1:]):
        assert getattr(_abi.PinballArgs, f).offset == off, f
    assert out[-3:] == [_abi.PINBALL_V["screen_AS"], _abi.PINBALL_S["n_changed"], _abi.CONS_OP["to_dense"]]
