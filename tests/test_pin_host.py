"""``state.gaussian_pin_naive`` / ``state.gaussian_pin_cov`` without a GPU: what the constructors derive, ``check()``, the
refusals, and the new entry of the C ABI."""
import os
import re

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Backend:
    def __init__(self, *names):
        self.names = set(names)

    def has(self, name):
        return name in self.names


class _StubNaive(ad.matrix.MatrixNaiveBase64):
    """A host matrix with the two operations the constructor calls, behind a backend that claims the pin entry."""

    def __init__(self, X, backend=None):
        self.X = np.asarray(X, dtype=np.float64)
        self._backend = backend if backend is not None else _Backend("gaussian_pin_solve")

    def rows(self):
        return self.X.shape[0]

    def cols(self):
        return self.X.shape[1]

    def mul(self, v, weights, out):
        out[...] = (v * weights) @ self.X

    def cov(self, j, q, sqrt_weights, out):
        B = sqrt_weights[:, None] * self.X[:, j:j + q]
        out[...] = B.T @ B


class _StubCov(ad.matrix.MatrixCovBase64):
    def __init__(self, A, backend=None):
        self.A = np.asarray(A, dtype=np.float64)
        self._backend = backend if backend is not None else _Backend("gaussian_pin_solve")

    def cols(self):
        return self.A.shape[0]

    def to_dense(self, i, q, out):
        out[...] = self.A[i:i + q, i:i + q]


def _naive_args(**kw):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(8, 6))
    w = rng.uniform(1, 2, 8)
    w /= w.sum()
    args = dict(X=_StubNaive(X), y_mean=0.25, y_var=1.5, constraints=None, groups=[0, 1, 4], alpha=1.0,
                penalty=np.ones(3), weights=w, screen_set=[2, 0], lmda_path=[0.5, 0.25], rsq=0.0, resid=rng.normal(size=8),
                screen_beta=np.zeros(3), screen_is_active=[False, False], active_set_size=0, active_set=np.zeros(2, dtype=int),
                max_active_size=7)
    args.update(kw)
    return args, X, w


def test_constructor_derives_what_the_reference_derives():
    args, X, w = _naive_args()
    s = ad.state.gaussian_pin_naive(**args)
    assert s.group_sizes.tolist() == [1, 3, 2]
    assert s.screen_begins.tolist() == [0, 2]                      # group 2 has two coefficients, group 0 one
    assert s.max_active_size == 3                                  # min(7, G)
    assert np.isclose(s.resid_sum, np.sum(w * args["resid"]))
    xm = w @ X
    C = (X[:, 4:6] * w[:, None]).T @ X[:, 4:6] - np.outer(xm[4:6], xm[4:6])
    vals = np.linalg.eigvalsh(C)
    assert np.allclose(s.screen_vars[:2], np.maximum(vals, 0)) and len(s.screen_vars) == 3
    assert np.allclose(s.screen_vars[2], w @ X[:, 0] ** 2 - xm[0] ** 2)
    assert np.allclose(s.screen_X_means, np.concatenate([xm[4:6], xm[:1]]))
    assert [t.shape for t in s.screen_transforms] == [(2, 2), (1, 1)]
    assert np.allclose(s.screen_transforms[0] @ np.diag(vals) @ s.screen_transforms[0].T, C)
    assert s.betas.shape == (0, 6) and s.iters == 0 and s.error == ""
    assert s.check(method="assert")
    # without an intercept nothing is centred; a missing max_active_size is G
    s2 = ad.state.gaussian_pin_naive(**_naive_args(intercept=False, max_active_size=None)[0])
    assert np.allclose(s2.screen_vars[2], w @ X[:, 0] ** 2) and s2.max_active_size == 3


def test_cov_constructor_derives_vars_and_transforms():
    rng = np.random.default_rng(1)
    B = rng.normal(size=(9, 5))
    A = B.T @ B
    s = ad.state.gaussian_pin_cov(A=_StubCov(A), constraints=None, groups=[0, 2], alpha=0.5, penalty=np.ones(2), screen_set=[1],
                                  lmda_path=[1.0], rsq=0.0, screen_beta=np.zeros(3), screen_grad=np.ones(3),
                                  screen_is_active=[False], active_set_size=0, active_set=[0])
    assert s.group_sizes.tolist() == [2, 3] and s.screen_begins.tolist() == [0] and s.max_active_size == 2
    assert np.allclose(s.screen_vars, np.linalg.eigvalsh(A[2:, 2:])) and s.screen_transforms[0].shape == (3, 3)
    assert s.check(method="assert")


@pytest.mark.parametrize("change,message", [
    (dict(screen_set=[2, 2], screen_beta=np.zeros(4)), "screen_set has unique values"),
    (dict(screen_is_active=[True, False]), "screen_is_active is consistent with active_set"),
    (dict(screen_beta=np.zeros(4)), "screen_beta size"),
    (dict(lmda_path=[0.5, -0.1]), "lmda_path is non-negative"),
])
def test_check_raises_on_each_inconsistency(change, message):
    s = ad.state.gaussian_pin_naive(**_naive_args(**change)[0])
    assert not s.check()
    with pytest.raises(AssertionError, match=re.escape(message)):
        s.check(method="assert")


def test_refusals_say_what_to_use_instead():
    args, X, _ = _naive_args()
    with pytest.raises(RuntimeError, match="use grpnet"):
        ad.state.gaussian_pin_naive(**dict(args, constraints=[None, ad.constraint.lower(np.zeros(3)), None]))
    with pytest.raises(ValueError, match="X must be an instance of MatrixNaiveBase32 or MatrixNaiveBase64."):
        ad.state.gaussian_pin_naive(**dict(args, X=X))
    with pytest.raises(RuntimeError, match=r'backend\.has\("gaussian_pin_solve"\)'):
        ad.state.gaussian_pin_naive(**dict(args, X=_StubNaive(X, _Backend("grpnet_solve"))))
    cov = dict(A=_StubCov(np.eye(3)), constraints=None, groups=[0, 1, 2], alpha=1.0, penalty=np.ones(3), screen_set=[0],
               lmda_path=[1.0], rsq=0.0, screen_beta=[0.0], screen_grad=[1.0], screen_is_active=[False], active_set_size=0,
               active_set=[0])
    with pytest.raises(RuntimeError, match="use gaussian_cov"):
        ad.state.gaussian_pin_cov(**dict(cov, constraints=[ad.constraint.lower(np.zeros(1)), None, None]))
    with pytest.raises(ValueError, match="A must be an instance of MatrixCovBase32 or MatrixCovBase64."):
        ad.state.gaussian_pin_cov(**dict(cov, A=np.eye(3)))
    with pytest.raises(ValueError, match="A must be an instance"):
        ad.state.gaussian_pin_cov(**dict(cov, A=_StubNaive(X)))
    with pytest.raises(RuntimeError, match=r'backend\.has\("gaussian_pin_solve"\)'):
        ad.state.gaussian_pin_cov(**dict(cov, A=_StubCov(np.eye(3), _Backend())))


def test_cpu_backend_designs_are_refused(oracle):
    """A design of the CPU restatement (the tests' reference backend) has no pin entry: refused at construction."""
    args, X, _ = _naive_args()
    with pytest.raises(RuntimeError, match="gaussian_pin_solve"):
        ad.state.gaussian_pin_naive(**dict(args, X=oracle.dense(np.asfortranarray(X))))


def test_new_entry_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "adelie_hip.h")).read()
    assert re.search(r"\bint\s+adelie_hip_gaussian_pin_solve\s*\(", hdr)
    assert "gaussian_pin_solve" in _abi.HIP_SYMBOLS
    b = _abi.hip_backend()
    assert b.has("gaussian_pin_solve")
    # the accessors it adds are appended: nothing that existed moved
    assert (_abi.V["rsqs"], _abi.V["benchmark_active"], _abi.V["screen_grad"]) == (17, 18, 19)
    assert (_abi.I["active_begins"], _abi.I["active_order"]) == (112, 113)
    assert (_abi.S["pin_iters"], _abi.S["n_pin_launches"], _abi.S["pin_route"]) == (97, 98, 99)
    assert _abi.V["benchmark_invariance"] == 16 and _abi.I["constraint_dev_groups"] == 111 and _abi.S["engine_panel"] == 96
    assert re.search(r"#define\s+ADELIE_HIP_ABI_VERSION\s+14\b", hdr) and _abi.ABI_VERSION == 14
    # the config switch is known to the library (0 / 1, default on) and to ad.configs
    assert b.fn("set_config")(b"pin_path_launch", 0.0) == 0 and b.fn("set_config")(b"pin_path_launch", 1.0) == 0
    assert ad.configs.Configs.pin_path_launch is True
