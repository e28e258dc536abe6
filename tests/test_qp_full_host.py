"""adelie_amd.optimization without a device: the numpy restatement the GPU tests compare with (qp_full_checks.py) converges and
solves the problems it is given, the two host functions agree with brute force, and the module's surface is the reference's."""
import ctypes
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qp_full_checks as qc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "adelie_hip.h")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("n, d", qc.SHAPES)
def test_restatement_converges(n, d, kind, dtype):
    """A condition of the GPU tests, not a measurement: every problem they solve stops before max_iters (seeds 0-2; none had
    to be replaced)."""
    for seed in qc.SEEDS:
        R = qc.cached_run(kind, n, d, seed, dtype)
        assert R.converged and R.iters < qc.MAX_ITERS, (seed, R.iters)


@pytest.mark.parametrize("n, d", qc.SHAPES)
def test_nnqp_objective_equals_scipy_nnls(n, d):
    """The reference's own criterion.  (nnls takes about ten seconds per problem at d = 1100: one seed there.)"""
    from scipy.optimize import nnls

    for seed in (qc.SEEDS if d <= 200 else qc.SEEDS[:1]):
        P = qc.problem(n, d, seed, "float64")
        R = qc.cached_run("nnqp", n, d, seed, "float64")
        x_ref, _ = nnls(P.X, P.y, maxiter=100 * d)
        assert np.allclose(qc.objective("nnqp", P, R.x), qc.objective("nnqp", P, x_ref))


@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("n, d", qc.SHAPES)
def test_kkt_f64(n, d, kind):
    """At tol = 1e-12 the final grad satisfies the optimality conditions within sqrt(thr) sum_{j != i} |Q_ij| / sqrt(q_jj) + 1e-12:
    the first term is what the visits after i in the last sweep can have moved g_i by (each satisfied q_jj del_j^2 < thr), the
    second covers the rounding of grad against v - Q x (measured about 1e-15)."""
    tol = 1e-12
    for seed in qc.SEEDS:
        P = qc.problem(n, d, seed, "float64")
        R = qc.cached_run(kind, n, d, seed, "float64", tol)
        assert R.converged
        x, g, Q = R.x, R.grad, P.quad
        assert np.max(np.abs(g - (P.v - Q @ x))) < 1e-12
        thr = float(qc.threshold(kind, d, tol, P.y_var, "float64"))
        w = np.abs(Q) / np.sqrt(np.diag(Q))[None, :]
        np.fill_diagonal(w, 0)
        slack = np.sqrt(thr) * w.sum(axis=1) + 1e-12
        if kind == "nnqp":
            assert np.all(x >= 0)
            assert np.all(g[x == 0] <= slack[x == 0])
            assert np.all(np.abs(g[x > 0]) <= slack[x > 0])
        elif kind == "lasso":
            z = x == 0
            assert np.all(np.abs(g[z]) <= P.penalty[z] + slack[z])
            assert np.all(np.abs(g[~z] - P.penalty[~z] * np.sign(x[~z])) <= slack[~z])
        else:
            z, pos, neg = x == 0, x > 0, x < 0
            assert np.all(g[z] >= -P.penalty_neg[z] - slack[z]) and np.all(g[z] <= P.penalty_pos[z] + slack[z])
            assert np.all(np.abs(g[pos] - P.penalty_pos[pos]) <= slack[pos])
            assert np.all(np.abs(g[neg] + P.penalty_neg[neg]) <= slack[neg])


@pytest.mark.parametrize("n, seed", [(100, 0), (1000, 24), (234, 123), (2, 239)])
def test_search_pivot_against_per_pivot_regression(n, seed):
    rng = np.random.RandomState(seed)
    x = np.sort(rng.normal(0, 1, n))
    p = x[rng.choice(n)]
    y = rng.normal() + rng.normal() * (p - x) * (x <= p) + rng.normal(0, 0.1)
    idx, mses = ad.optimization.search_pivot(x, y)
    expected = np.empty(n)
    expected[0] = np.inf
    yc = y - y.mean()
    for j in range(1, n):
        t = (x[j] - x) * (x <= x[j])
        tc = t - t.mean()
        expected[j] = -((yc @ tc) / (tc @ tc)) ** 2 * (tc @ tc)
    assert np.allclose(mses, expected)
    assert idx == int(np.argmin(expected))


@pytest.mark.parametrize("n", [3, 5, 10, 20])
def test_symmetric_penalty_against_grid(n):
    ts = np.linspace(-2, 2, 10000)

    def f(t, x, alpha):
        r = x[:, None] - np.atleast_1d(t)[None]
        return np.sum(0.5 * (1 - alpha) * r ** 2 + alpha * np.abs(r), axis=0)

    for seed in range(5):
        rng = np.random.RandomState(seed)
        x = np.sort(rng.uniform(-1, 1, n))
        alpha = rng.uniform(0, 1)
        t_star = ad.optimization.symmetric_penalty(x, alpha)
        assert np.all(f(ts, x, alpha) >= f(t_star, x, alpha))
    assert ad.optimization.symmetric_penalty(x, 1.0) == np.median(x)
    assert ad.optimization.symmetric_penalty(x, 0.0) == np.mean(x)
    assert ad.optimization.symmetric_penalty(np.empty(0), 0.5) == 0.0


def test_surface():
    opt = ad.optimization
    args = lambda cls: list(inspect.signature(cls.__init__).parameters)[1:]
    assert args(opt.StateNNQPFull) == ["quad", "max_iters", "tol", "x", "grad"]
    assert args(opt.StateLassoFull) == ["quad", "penalty", "max_iters", "tol", "x", "grad"]
    assert args(opt.StatePinballFull) == ["quad", "penalty_neg", "penalty_pos", "y_var", "max_iters", "tol", "x", "grad"]
    assert not hasattr(opt, "StateLinQPFull")
    assert callable(opt.solve_many) and callable(opt.search_pivot) and callable(opt.symmetric_penalty)
    opt.solve_many([])  # a no-op, no device needed

    Q, z = np.asfortranarray(np.eye(3)), np.zeros(3)
    s = opt.StatePinballFull(Q, z + 1, z + 2, 3.0, 10, 1e-3, z.copy(), z.copy())
    assert s.quad is Q and s.max_iters == 10 and s.tol == 1e-3 and s.y_var == 3.0 and s.iters == 0 and s.time_elapsed == 0
    assert s.penalty_neg[0] == 1 and s.penalty_pos[0] == 2 and s.x.shape == s.grad.shape == (3,)
    with pytest.raises(AttributeError):
        s.x = z


def test_constructor_checks():
    opt = ad.optimization
    Q, z = np.asfortranarray(np.eye(3)), np.zeros(3)
    makers = {
        "nnqp": lambda quad=Q, tol=1e-3, x=z.copy(), grad=z.copy(), **kw: opt.StateNNQPFull(quad, 10, tol, x, grad),
        "lasso": lambda quad=Q, tol=1e-3, x=z.copy(), grad=z.copy(), penalty=z, **kw: opt.StateLassoFull(quad, penalty, 10, tol, x, grad),
        "pinball": lambda quad=Q, tol=1e-3, x=z.copy(), grad=z.copy(), penalty_neg=z, penalty_pos=z, **kw: opt.StatePinballFull(
            quad, penalty_neg, penalty_pos, 1.0, 10, tol, x, grad),
    }
    pre = "adelie_core solver: "
    for kind, make in makers.items():
        make()
        with pytest.raises(RuntimeError, match=re.escape(pre + "quad must be (d, d). ")):
            make(quad=np.asfortranarray(np.zeros((3, 4))))
        with pytest.raises(RuntimeError, match=re.escape(pre + "tol must be >= 0.")):
            make(tol=-1e-3)
        with pytest.raises(RuntimeError, match=re.escape(pre + "x must be (d,) where quad is (d, d). ")):
            make(x=np.zeros(4))
        with pytest.raises(RuntimeError, match=re.escape(pre + "grad must be (d,) where quad is (d, d). ")):
            make(grad=np.zeros(2))
        # as the reference's noconvert: nothing is converted
        with pytest.raises(TypeError):
            make(quad=Q.astype(np.float32))
        with pytest.raises(TypeError):
            make(quad=np.eye(6)[::2, ::2])
        with pytest.raises(TypeError):
            make(quad=np.eye(3, dtype=np.int64))
        ro = z.copy()
        ro.setflags(write=False)
        with pytest.raises(TypeError):
            make(x=ro)
        with pytest.raises(TypeError):
            make(grad=[0.0, 0.0, 0.0])
    for name in ("penalty",):
        with pytest.raises(RuntimeError, match=re.escape(pre + f"{name} must be (d,) where quad is (d, d). ")):
            makers["lasso"](**{name: np.zeros(4)})
    for name in ("penalty_neg", "penalty_pos"):
        with pytest.raises(RuntimeError, match=re.escape(pre + f"{name} must be (d,) where quad is (d, d). ")):
            makers["pinball"](**{name: np.zeros(4)})
    a = opt.StateNNQPFull(Q, 10, 1e-3, z.copy(), z.copy())
    b = opt.StateLassoFull(Q, z, 10, 1e-3, z.copy(), z.copy())
    with pytest.raises(TypeError):
        opt.solve_many([a, b])
    Q32, z32 = Q.astype(np.float32), z.astype(np.float32)
    with pytest.raises(TypeError):
        opt.solve_many([a, opt.StateNNQPFull(Q32, 10, 1e-3, z32.copy(), z32.copy())])


def test_abi_entry():
    assert "qp_full_solve" in _abi.HIP_SYMBOLS
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+adelie_hip_qp_full_solve\s*\(\s*const\s+adelie_hip_qp_full_args\s*\*", txt)
    assert _abi.hip_backend().has("qp_full_solve")
    # the malformed-argument route needs no device
    b = _abi.hip_backend()
    assert b.fn("qp_full_solve")(None) != 0
    args = _abi.QpFullArgs(kind=7, dtype=_abi.F64, n_problems=0)
    assert b.fn("qp_full_solve")(ctypes.byref(args)) != 0
    assert b"kind" in b.fn("last_error")()
    args = _abi.QpFullArgs(kind=0, dtype=_abi.F64, n_problems=0)
    assert b.fn("qp_full_solve")(ctypes.byref(args)) == 0
    # the config key that forces the block form's state into global memory
    assert b.fn("set_config")(b"qp_full_lds_max_d", 100.0) == 0
    assert b.fn("set_config")(b"qp_full_lds_max_d", 0.0) == 0


def test_ctypes_struct_matches_c_layout():
    fields = [f[0] for f in _abi.QpFullArgs._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"adelie_hip.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(adelie_hip_qp_full_args));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(adelie_hip_qp_full_args, {f}));\n'
    prog += 'printf("%d %d %d %d\\n", ADELIE_HIP_QP_FULL_NNQP, ADELIE_HIP_QP_FULL_LASSO, ADELIE_HIP_QP_FULL_PINBALL, ADELIE_HIP_QP_FULL_MAX_ITERS);\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(_abi.QpFullArgs)
    for f, off in zip(fields, out[1:]):
        assert getattr(_abi.QpFullArgs, f).offset == off, f
    k = _abi.QP_FULL_KIND
    assert out[-4:] == [k["nnqp"], k["lasso"], k["pinball"], _abi.QP_FULL_MAX_ITERS]
