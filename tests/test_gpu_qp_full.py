"""adelie_amd.optimization on the device against the numpy restatement of tests/qp_full_checks.py (itself checked in
test_qp_full_host.py): x, grad and iters must be equal BIT FOR BIT.  That is derived, not measured: every operation of a visit is
one correctly rounded IEEE operation with contraction off, in the reference's order, no reduction or atomic sits anywhere on the
path, and Q is an input, not something the device sums.  A mismatch is a bug in the kernel, not a tolerance to widen."""
import os
import re
import sys

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qp_full_checks as qc  # noqa: E402

pytestmark = pytest.mark.gpu

opt = ad.optimization
DTYPES = ["float64", "float32"]
CLASSES = dict(nnqp=opt.StateNNQPFull, lasso=opt.StateLassoFull, pinball=opt.StatePinballFull)


def set_config(name, value):
    b = _abi.hip_backend()
    b.check(b.fn("set_config")(name.encode(), float(value)))


def make_state(kind, P, *, quad=None, max_iters=qc.MAX_ITERS, tol=None, x=None, grad=None):
    """A state on problem P from x = 0, grad = v (or the given start)."""
    quad = P.quad if quad is None else quad
    tol = qc.tol_for(P.dtype) if tol is None else tol
    x = np.zeros(P.d, dtype=P.dtype) if x is None else x
    grad = P.v.copy() if grad is None else grad
    if kind == "nnqp":
        return opt.StateNNQPFull(quad, max_iters, tol, x, grad)
    if kind == "lasso":
        return opt.StateLassoFull(quad, P.penalty, max_iters, tol, x, grad)
    return opt.StatePinballFull(quad, P.penalty_neg, P.penalty_pos, P.y_var, max_iters, tol, x, grad)


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(qc.bits(a), qc.bits(b))


def assert_equals_run(state, R):
    assert state.iters == R.iters, (state.iters, R.iters)
    assert same_bits(state.x, R.x), int(np.sum(qc.bits(state.x) != qc.bits(R.x)))
    assert same_bits(state.grad, R.grad), int(np.sum(qc.bits(state.grad) != qc.bits(R.grad)))


def assert_same_state(a, b):
    assert a.iters == b.iters and same_bits(a.x, b.x) and same_bits(a.grad, b.grad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("n, d", qc.SHAPES)
def test_bit_equality(hip, n, d, kind, dtype):
    P = qc.problem(n, d, 0, dtype)
    quad_before = P.quad.copy()
    s = make_state(kind, P)
    x, grad = s.x, s.grad
    s.solve()
    assert s.x is x and s.grad is grad  # the caller's arrays, updated in place
    assert_equals_run(s, qc.cached_run(kind, n, d, 0, dtype))
    assert s.time_elapsed > 0
    assert np.array_equal(P.quad, quad_before)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", qc.KINDS)
def test_global_state_gives_the_same_bits(hip, kind, dtype):
    n, d = 400, 200
    P = qc.problem(n, d, 0, dtype)
    in_lds = make_state(kind, P)
    in_lds.solve()
    in_global = make_state(kind, P)
    try:
        set_config("qp_full_lds_max_d", 100)
        in_global.solve()
    finally:
        set_config("qp_full_lds_max_d", 0)
    assert_same_state(in_lds, in_global)
    assert_equals_run(in_global, qc.cached_run(kind, n, d, 0, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("n, d", [(10, 20), (130, 65)])
def test_input_forms(hip, n, d, kind, dtype):
    import torch

    P = qc.problem(n, d, 0, dtype)
    R = qc.cached_run(kind, n, d, 0, dtype)
    assert np.array_equal(P.quad, P.quad.T)  # X'X as numpy forms it: the i-th row and the i-th column are the same slice
    quad_c = np.ascontiguousarray(P.quad)
    assert quad_c.flags.c_contiguous and not quad_c.flags.f_contiguous
    keep = quad_c.copy()
    s = make_state(kind, P, quad=quad_c)
    s.solve()
    assert_equals_run(s, R)
    assert np.array_equal(quad_c, keep)
    # the restatement on the C-ordered buffer reads the same slices
    x, grad = np.zeros(d, dtype=P.dtype), P.v.copy()
    iters, _ = qc.solve(kind, quad_c, qc.penalties(P, kind), P.y_var, qc.MAX_ITERS, qc.tol_for(dtype), x, grad)
    assert iters == s.iters and same_bits(x, s.x) and same_bits(grad, s.grad)

    t = torch.from_numpy(keep.copy()).to("cuda")
    for quad_t in (t, t.t()):  # C- and F-contiguous views of one buffer
        s = make_state(kind, P, quad=quad_t)
        assert s.quad is quad_t
        s.solve()
        assert_equals_run(s, R)
    assert np.array_equal(t.cpu().numpy(), keep)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", qc.KINDS)
def test_solve_many_mixed_dimensions(hip, kind, dtype):
    """All seven shapes x seeds 0-2 in one call: wave and block forms side by side."""
    cases = [(n, d, seed) for (n, d) in qc.SHAPES for seed in qc.SEEDS]
    alone = [make_state(kind, qc.problem(n, d, seed, dtype)) for (n, d, seed) in cases]
    for s in alone:
        s.solve()
    batch = [make_state(kind, qc.problem(n, d, seed, dtype)) for (n, d, seed) in cases]
    opt.solve_many(batch)
    for a, b in zip(alone, batch):
        assert_same_state(a, b)
    assert len({b.time_elapsed for b in batch}) == 1 and batch[0].time_elapsed > 0
    # the same batch in another order: no problem's result depends on the others
    again = [make_state(kind, qc.problem(n, d, seed, dtype)) for (n, d, seed) in cases[::-1]]
    opt.solve_many(again)
    for a, b in zip(alone[::-1], again):
        assert_same_state(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", qc.KINDS)
def test_solve_many_300_problems(hip, kind, dtype):
    """More workgroups than one wave of the grid."""
    n, d = 10, 20
    assert len(qc.BATCH_SEEDS) == 300
    alone = [make_state(kind, qc.problem(n, d, seed, dtype)) for seed in qc.BATCH_SEEDS]
    for s in alone:
        s.solve()
    batch = [make_state(kind, qc.problem(n, d, seed, dtype)) for seed in qc.BATCH_SEEDS]
    opt.solve_many(batch)
    for a, b in zip(alone, batch):
        assert_same_state(a, b)
    for seed in (0, 150, 299):  # and a few of them against the restatement
        assert_equals_run(batch[qc.BATCH_SEEDS.index(seed)], qc.cached_run(kind, n, d, seed, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", qc.KINDS)
def test_max_iters(hip, kind, dtype):
    n, d = 10, 20
    P = qc.problem(n, d, 0, dtype)
    R = qc.cached_run(kind, n, d, 0, dtype, None, 1)
    assert not R.converged and R.iters == 1
    message = f"adelie_core solver: {CLASSES[kind].__name__}: max iterations reached!"
    s = make_state(kind, P, max_iters=1)
    with pytest.raises(RuntimeError, match=re.escape(message)):
        s.solve()
    assert s.iters == 1
    assert_equals_run(s, R)

    k = 2
    batch = [make_state(kind, qc.problem(n, d, seed, dtype), max_iters=1 if i == k else qc.MAX_ITERS)
             for i, seed in enumerate((1, 2, 0, 1))]
    with pytest.raises(RuntimeError, match=re.escape(message)) as e:
        opt.solve_many(batch)
    assert re.search(r"\[2\]", str(e.value))
    assert_equals_run(batch[k], R)
    for i, seed in ((0, 1), (1, 2), (3, 1)):
        assert_equals_run(batch[i], qc.cached_run(kind, n, d, seed, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nnqp_zero_diagonal(hip, dtype):
    n, d, i = 10, 20, 5
    P = qc.problem(n, d, 0, dtype)
    quad = P.quad.copy()
    quad[i, :] = 0
    quad[:, i] = 0
    x0 = np.zeros(d, dtype=P.dtype)
    x0[i] = 0.25
    g0 = P.v.copy()  # v - Q x0: column i of Q is zero
    x, grad = x0.copy(), g0.copy()
    iters, converged = qc.solve("nnqp", quad, (), P.y_var, qc.MAX_ITERS, qc.tol_for(dtype), x, grad)
    assert converged and x[i] == x0[i]
    s = opt.StateNNQPFull(quad, qc.MAX_ITERS, qc.tol_for(dtype), x0.copy(), g0.copy())
    s.solve()
    assert s.x[i] == x0[i] and s.grad[i] == g0[i]
    assert s.iters == iters and same_bits(s.x, x) and same_bits(s.grad, grad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("n, d", [(10, 3), (10, 20), (130, 65)])
def test_warm_start(hip, n, d, kind, dtype):
    """A second .solve() on a solved state is one sweep.  That sweep may still move coordinates by less than the threshold (the
    restatement does, on every case here but nnqp at (10, 3)), so the bits to expect are those of the restatement's own second
    solve; where the restatement's second solve changes nothing, nothing changes here."""
    P = qc.problem(n, d, 0, dtype)
    R = qc.cached_run(kind, n, d, 0, dtype)
    s = make_state(kind, P)
    s.solve()
    x1, g1 = s.x.copy(), s.grad.copy()
    s.solve()
    assert s.iters == 1
    x, grad = R.x.copy(), R.grad.copy()
    iters, converged = qc.solve(kind, P.quad, qc.penalties(P, kind), P.y_var, qc.MAX_ITERS, R.tol, x, grad)
    assert converged and iters == 1
    assert same_bits(s.x, x) and same_bits(s.grad, grad)
    if same_bits(x, R.x) and same_bits(grad, R.grad):
        assert same_bits(s.x, x1) and same_bits(s.grad, g1)
    if kind == "nnqp" and d == 3:
        assert same_bits(s.x, x1) and same_bits(s.grad, g1)
