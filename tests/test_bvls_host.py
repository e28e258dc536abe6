"""bvls without a device: the numpy restatement the GPU tests compare against (tests/bvls_checks.py) is itself checked against
scipy's active-set BVLS, and the public surface (export, signatures, the ctypes mirror of the C arguments, the ABI version)
is what the reference and include/adelie_hip.h say."""
import ctypes
import inspect
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
from scipy.optimize import lsq_linear

import adelie_amd as ad
from adelie_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvls_checks as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scipy_objective(X, y, lower, upper):
    n = X.shape[0]
    sw = np.sqrt(1 / n)  # the sqrt(w)-scaled problem, w = 1/n
    sol = lsq_linear(X * sw, y * sw, bounds=(lower, upper), method="bvls", tol=1e-14)
    return bc.objective(X, y, sol.x)


@pytest.mark.parametrize("n, p", [(10, 50), (40, 13), (100, 1000)])
def test_restatement_on_the_reference_generator(n, p):
    """The reference's own criterion (tests/test_solver.py::test_bvls): np.allclose of the two objectives, tol = 1e-9."""
    X, y, lower, upper = bc.ref_sparse(n, p, 0)
    res = bc.solve(X, y, lower, upper, np.float64, tol=1e-9)
    assert res.error == ""
    actual, expected = bc.objective(X, y, res.beta), scipy_objective(X, y, lower, upper)
    print(f"objective: restatement {actual:.3e}, scipy {expected:.3e}")
    assert np.allclose(actual, expected)
    assert np.all(res.beta >= lower) and np.all(res.beta <= upper)


@pytest.mark.parametrize("n, p", [(40, 13), (200, 70)])
@pytest.mark.parametrize("seed", range(3))
def test_restatement_on_gaussian(n, p, seed):
    """Objective gap over y_var.  The solver's coarsest stopping rule ends it when a whole fit moved the loss by less than
    1e-6 y_var; a run that ends by the KKT exit has no violator left and only the coordinate tolerance (1e-7 y_var per
    visit) between it and the optimum.  So 1e-6 bounds the gap of a correct run; measured: <= 3e-9."""
    X, y, lower, upper = bc.gaussian(n, p, seed)
    res = bc.solve(X, y, lower, upper, np.float64)
    assert res.error == ""
    gap = (bc.objective(X, y, res.beta) - scipy_objective(X, y, lower, upper)) / float(res.y_var)
    print(f"objective gap / y_var = {gap:.3e}")
    assert -1e-12 <= gap <= 1e-6
    assert np.all(res.beta >= lower) and np.all(res.beta <= upper)
    # the bookkeeping the device is compared with is consistent in itself
    assert sorted(np.flatnonzero(res.is_screen)) == sorted(res.screen)
    assert sorted(np.flatnonzero(res.is_active)) == sorted(res.active)
    assert set(res.active) <= set(res.screen)
    assert abs(float(res.loss) - bc.objective(X, y, res.beta)) <= 1e-12 * float(res.y_var) * res.iters


def test_exported():
    assert ad.bvls is ad.solver.bvls
    assert callable(ad.state.bvls)


def signature(f):
    return [(name, par.default) for name, par in inspect.signature(f).parameters.items()]


def test_solver_signature_is_the_reference():
    E = inspect.Parameter.empty
    assert signature(ad.solver.bvls) == [
        ("X", E), ("y", E), ("lower", E), ("upper", E), ("weights", None), ("kappa", None), ("max_iters", int(1e5)),
        ("tol", 1e-7), ("n_threads", 1), ("warm_start", None)]
    kinds = [par.kind for par in inspect.signature(ad.solver.bvls).parameters.values()]
    assert kinds[:4] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 4
    assert kinds[4:] == [inspect.Parameter.KEYWORD_ONLY] * 6


def test_state_signature_is_the_reference():
    E = inspect.Parameter.empty
    names = ["X", "y_var", "X_vars", "lower", "upper", "weights", "kappa", "max_iters", "tol", "screen_set_size", "screen_set",
             "is_screen", "active_set_size", "active_set", "is_active", "beta", "resid", "grad", "loss"]
    assert signature(ad.state.bvls) == [(name, E) for name in names]


def test_abi_version():
    assert _abi.ABI_VERSION == 14


def test_bvls_args_match_c_layout():
    fields = [f[0] for f in _abi.BvlsArgs._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"adelie_hip.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(adelie_hip_bvls_args));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(adelie_hip_bvls_args, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(_abi.BvlsArgs)
    for f, off in zip(fields, out[1:]):
        assert getattr(_abi.BvlsArgs, f).offset == off, f


class HostMatrix:
    """The matrix interface the generic route of state.bvls needs, on a numpy array (no device)."""

    _backend = None  # (what matrix.as_design recognises a design by)
    dtype = np.float64

    def __init__(self, X):
        self.X = X
        self.shape = X.shape

    def rows(self):
        return self.X.shape[0]

    def cols(self):
        return self.X.shape[1]

    def cmul(self, j, v, w):
        return self.X[:, j] @ (w * v)

    def ctmul(self, j, v, out):
        out += v * self.X[:, j]

    def mul(self, v, w, out):
        out[...] = self.X.T @ (w * v)

    def sq_mul(self, w, out):
        out[...] = (self.X ** 2).T @ w

    def sp_tmul(self, v, out):
        out[...] = v @ self.X.T


@pytest.mark.parametrize("n, p, kappa, max_iters", [(40, 13, None, int(1e5)), (64, 300, 7, int(1e5)), (64, 300, None, 3)])
def test_generic_route_follows_the_restatement(n, p, kappa, max_iters):
    """The loop over cmul / ctmul / mul that designs outside the native route take, run on a host matrix: the restatement's
    trajectory (its decisions are clear of rounding on these cases), warm start and max-iterations exit included."""
    X, y, lower, upper = bc.gaussian(n, p, 0)
    own = bc.solve(X, y, lower, upper, np.float64, kappa=kappa, max_iters=max_iters)
    assert own.min_gap >= 1e-9
    state = ad.bvls(HostMatrix(X), y, lower, upper, kappa=kappa, max_iters=max_iters)
    assert state.error == own.error
    assert list(state.screen_set[:state.screen_set_size]) == own.screen
    assert list(state.active_set[:state.active_set_size]) == own.active
    assert np.array_equal(state.is_screen, own.is_screen) and np.array_equal(state.is_active, own.is_active)
    assert state.iters == own.iters and state.n_kkt == own.n_kkt
    # the two runs round a visit's n-term dot in another order: n * eps per visit of a coordinate, one visit per pass
    slack = own.iters * n * np.finfo(np.float64).eps
    assert np.max(np.abs(state.beta - own.beta)) <= slack * max(1.0, float(np.max(np.abs(own.beta))))
    assert abs(state.loss - float(own.loss)) <= slack * float(own.y_var)
    if own.error == "":
        again = ad.bvls(HostMatrix(X), y, lower, upper, kappa=kappa, warm_start=state)
        warm = bc.solve(X, y, lower, upper, np.float64, kappa=kappa, warm_start=own)
        assert again.error == "" and (again.iters, again.n_kkt) == (warm.iters, warm.n_kkt)
        assert list(again.active_set[:again.active_set_size]) == warm.active


def test_state_argument_checks():
    X, y, lower, upper = bc.gaussian(40, 13, 0)
    kw = dict(X=HostMatrix(X), y_var=1.0, X_vars=np.ones(13), lower=lower, upper=upper, weights=np.full(40, 1 / 40), kappa=13,
              max_iters=100, tol=1e-7, screen_set_size=0, screen_set=np.zeros(13, dtype=int), is_screen=np.zeros(13, dtype=bool),
              active_set_size=0, active_set=np.zeros(13, dtype=int), is_active=np.zeros(13, dtype=bool), beta=lower,
              resid=y - X @ lower, grad=np.zeros(13), loss=0.0)
    ad.state.bvls(**kw)
    for change, msg in ((dict(lower=lower[:-1]), "lower must be (p,) where X is (n, p). "), (dict(kappa=0), "kappa must be > 0. "),
                        (dict(tol=-1.0), "tol must be >= 0."), (dict(weights=np.ones(39)), "weights must be (n,) where X is (n, p). "),
                        (dict(beta=lower[:-1]), "beta must be (p,) where X is (p, n). "),
                        (dict(active_set_size=14), "active_set_size must be <= p where X is (n, p). ")):
        with pytest.raises(RuntimeError) as e:
            ad.state.bvls(**dict(kw, **change))
        assert str(e.value) == "adelie_core solver: " + msg
